"""CapturedStream replays the streamed render block by block as a captured HIP graph, and silent_state materialises the
state a first block's ``state=None`` stands for.

"Eager" below is ``render_grafx(state=, return_state=True)`` started from ``silent_state(...)``.  Captured and eager run the
same kernels on the same arguments and no forward kernel accumulates with float atomics, so every captured-vs-eager
comparison is torch.equal (the standard tests/test_gpu_captured_render.py holds CapturedRender to).  Comparisons with the
one-call render (under exact_convolution_scope(True), as in tests/test_gpu_render_state.py) and between a render from
silent_state and one from ``state=None`` -- which may take other convolution kernels -- are conftest.assert_close at the
standing 1e-5 of the peak.  Sizes are those of tests/test_gpu_render_state.py (batch 2, stereo, a 256-tap equaliser, a
1001-tap reverb, ballistics compressors), in blocks of 512 (shorter than the reverb's history), 64 (shorter than both
histories) and 1."""
import pytest
import torch
import torch.nn as nn

from conftest import assert_close
from test_gpu_render_state import B, C, _chain_graph, _comp, _console, _eq, _one_call, _parameters, _render_data, _reverb

pytestmark = pytest.mark.gpu

CHAIN = ["in", "eq", "compressor", "reverb", "mix", "out"]


def _signal(n_src, length, seed, batch=B):
    shape = (n_src, C, length) if batch is None else (batch, n_src, C, length)
    return (0.3 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).cuda()


def _chain_setup(seed, length):
    procs = {"eq": _eq(), "compressor": _comp(), "reverb": _reverb()}
    G = _chain_graph(CHAIN)
    return procs, _signal(1, length, seed + 1), _parameters(procs, G, seed), _render_data(G)


def _eager(procs, x, params, rd, n, blocks, state=None, first=0, **kw):
    """Eager blocks ``first .. first + blocks`` of length n, from ``state`` (None: silent_state) -> (ys, bufs, states)."""
    from grafx_amd.render import render_grafx, silent_state

    ys, bufs, states = [], [], []
    with torch.no_grad():
        if state is None:
            state = silent_state(procs, x[..., :n], params, rd)
        for k in range(first, first + blocks):
            y, _, buf, state = render_grafx(procs, x[..., k * n : (k + 1) * n], params, rd, state=state, return_state=True, **kw)
            ys.append(y)
            bufs.append(buf)
            states.append(state)
    return ys, bufs, states


def _replay(stream, x, n, blocks, first=0):
    """The same blocks through the captured stream (its outputs are static: cloned)."""
    ys, bufs = [], []
    for k in range(first, first + blocks):
        y, inter, buf = stream(x[..., k * n : (k + 1) * n])
        assert inter == []
        ys.append(y.clone())
        bufs.append(None if buf is None else buf.clone())
    return ys, bufs


def _leaves(carry):
    from grafx_amd.processors.core._buffer_io import carry_leaves

    return carry_leaves(carry)


def _assert_same_state(got, want, what):
    assert got.samples == want.samples and got.steps == want.steps and got.batch == want.batch, what
    assert set(got.carries) == set(want.carries), what
    for i in want.carries:
        a, b = _leaves(got.carries[i]), _leaves(want.carries[i])
        assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b)), f"{what}: carry of step {i}"


def _steps_of(rd, node_type):
    return [i for i in range(1, rd.max_order + 1) if rd.iter_list[i].node_type == node_type]


# ---------------------------------------------------------------------------------------------------- 1 (and 4): the chain
@pytest.mark.parametrize("n, blocks", [(512, 8), (64, 6), (1, 3)])
def test_chain_replays_the_eager_blocks(n, blocks):
    """in -> equaliser (fsm) -> compressor (ballistics) -> reverb -> mix -> out: the output and every buffer row of every
    block bit for bit, the sample count, the state leaf by leaf, the hoisted designs, and the whole against one call."""
    from grafx_amd.render import CapturedStream

    procs, x, params, rd = _chain_setup(101, n * blocks)
    want_ys, want_bufs, want_states = _eager(procs, x, params, rd, n, blocks)
    stream = CapturedStream(procs, x[..., :n], params, rd)
    assert stream.samples == 0
    assert set(stream.designed) == set(_steps_of(rd, "eq") + _steps_of(rd, "reverb"))
    assert not set(stream.designed) & set(_steps_of(rd, "compressor"))
    for k in range(blocks):
        y, inter, buf = stream(x[..., k * n : (k + 1) * n])
        assert inter == [] and stream.samples == (k + 1) * n
        assert torch.equal(y, want_ys[k]), f"block {k}: output"
        assert buf.shape == want_bufs[k].shape
        for row in range(buf.shape[1]):
            assert torch.equal(buf[:, row], want_bufs[k][:, row]), f"block {k}: buffer row {row}"
        _assert_same_state(stream.state(), want_states[k], f"after block {k}")
    one_y, _, one_buf = _one_call(procs, x, params, rd)
    assert_close(torch.cat(want_ys, -1).cpu(), one_y.cpu(), 1e-5, f"chain in blocks of {n}: output vs one call")
    assert_close(torch.cat(want_bufs, -1).cpu(), one_buf.cpu(), 1e-5, f"chain in blocks of {n}: buffer vs one call")


# ---------------------------------------------------------------------------------------------------- 2: silent_state
def test_silent_state_stands_for_none():
    """A block rendered from silent_state against the same block from state=None: the output within 1e-5 (a history takes
    the state kernels, no history may take another convolution route), the compressor's envelope and the recursive
    equaliser's filter state leaving the block bit for bit (their kernels read zi[row] where they used the constant)."""
    from grafx_amd.render import RenderState, render_grafx, silent_state

    procs, x, params, rd = _chain_setup(111, 512)
    with torch.no_grad():
        silent = silent_state(procs, x, params, rd)
        assert isinstance(silent, RenderState) and silent.samples == 0
        y0, _, buf0, s0 = render_grafx(procs, x, params, rd, return_state=True)
        y1, _, buf1, s1 = render_grafx(procs, x, params, rd, state=silent, return_state=True)
    assert s0.samples == s1.samples == 512 and set(silent.carries) == set(s0.carries)
    for i, c in s0.carries.items():
        assert [t.shape for t in _leaves(silent.carries[i])] == [t.shape for t in _leaves(c)]
    (comp,) = _steps_of(rd, "compressor")
    assert torch.equal(silent.carries[comp], torch.ones_like(silent.carries[comp]))
    assert not silent.carries[_steps_of(rd, "eq")[0]].any() and not silent.carries[_steps_of(rd, "reverb")[0]].any()
    assert_close(y1.cpu(), y0.cpu(), 1e-5, "chain from silent_state vs from None: output")
    assert_close(buf1.cpu(), buf0.cpu(), 1e-5, "chain from silent_state vs from None: buffer")
    assert torch.equal(s1.carries[comp], s0.carries[comp])

    procs = {"eq": _eq(), "buseq": _eq("lfilter"), "compressor": _comp(), "reverb": _reverb()}
    G = _console()
    rd, params, x = _render_data(G), _parameters(procs, G, 113), _signal(8, 512, 114)
    with torch.no_grad():
        y0, _, _, s0 = render_grafx(procs, x, params, rd, return_state=True)
        y1, _, _, s1 = render_grafx(procs, x, params, rd, state=silent_state(procs, x, params, rd), return_state=True)
    assert_close(y1.cpu(), y0.cpu(), 1e-5, "console from silent_state vs from None: output")
    for i in _steps_of(rd, "buseq") + _steps_of(rd, "compressor"):
        assert torch.equal(s1.carries[i], s0.carries[i]), f"console: carry of step {i} ({rd.iter_list[i].node_type})"


# ---------------------------------------------------------------------------------------------------- 3 (and 4): the console
def _first_order():
    """One first-order recursive section per row on IIRFilter(order=1, backend="lfilter"): its leaving state has a zeroed
    second entry, which the filter forms with a constant -- made on the device, or the block could not be captured."""
    from grafx_amd.processors.core.iir import BiquadStream, IIRFilter

    class FirstOrder(BiquadStream, nn.Module):
        def __init__(self):
            super().__init__()
            self.biquad = IIRFilter(order=1, backend="lfilter")

        def forward(self, input_signals, Bs, a1, **block):
            As = torch.stack([torch.ones_like(a1), 0.9 * torch.tanh(a1)], -1)
            return self.biquad(input_signals, Bs.unsqueeze(1), As.unsqueeze(1), **block)

        def parameter_size(self):
            return {"Bs": (1, 2), "a1": 1}

    return FirstOrder().cuda()


@pytest.mark.parametrize("variant", ["shared_rows", "output_only", "unbatched"])
def test_console_replays_the_eager_blocks(variant):
    """The 8-strip / 2-bus console with an lfilter equaliser on the buses (whose steps are not hoisted), six blocks of 64:
    batch-shared parameters, keep_signal_buffer=False (the third return is None), an unbatched (n, C, L) input."""
    from grafx_amd.render import CapturedStream

    n, blocks = 64, 6
    procs = {"eq": _eq(), "buseq": _eq("lfilter"), "compressor": _comp(), "reverb": _reverb()}
    G = _console()
    rd, params = _render_data(G), _parameters(procs, G, 121)
    x = _signal(8, n * blocks, 122, batch=None if variant == "unbatched" else B)
    keep = variant != "output_only"
    want_ys, want_bufs, want_states = _eager(procs, x, params, rd, n, blocks, keep_signal_buffer=keep)
    stream = CapturedStream(procs, x[..., :n], params, rd, keep_signal_buffer=keep)
    assert set(stream.designed) == set(_steps_of(rd, "eq") + _steps_of(rd, "reverb"))
    assert len(_steps_of(rd, "buseq")) >= 1 and not set(stream.designed) & set(_steps_of(rd, "buseq"))
    got_ys, got_bufs = _replay(stream, x, n, blocks)
    for k in range(blocks):
        assert torch.equal(got_ys[k], want_ys[k]), f"console ({variant}), block {k}: output"
        if keep:
            assert torch.equal(got_bufs[k], want_bufs[k]), f"console ({variant}), block {k}: buffer"
        else:
            assert got_bufs[k] is None and want_bufs[k] is None
    _assert_same_state(stream.state(), want_states[-1], f"console ({variant})")
    assert stream.state().batch == (None if variant == "unbatched" else B)
    one_y = _one_call(procs, x, params, rd)[0]
    assert_close(torch.cat(want_ys, -1).cpu(), one_y.cpu(), 1e-5, f"console ({variant}): output vs one call")


def test_first_order_recursive_section_replays_the_eager_blocks():
    """in -> IIRFilter(order=1, backend="lfilter") -> out, per-row parameters expanded over the batch: the replaced
    constant of the first-order state.  Four blocks of 64; the state's second entries are zero."""
    from grafx_amd.render import CapturedStream

    n, blocks = 64, 4
    procs = {"first": _first_order()}
    G = _chain_graph(["in", "first", "out"])
    rd, params, x = _render_data(G), _parameters(procs, G, 125), _signal(1, n * blocks, 126)
    want_ys, want_bufs, want_states = _eager(procs, x, params, rd, n, blocks)
    stream = CapturedStream(procs, x[..., :n], params, rd)
    assert stream.designed == ()
    got_ys, got_bufs = _replay(stream, x, n, blocks)
    assert all(torch.equal(a, b) for a, b in zip(got_ys, want_ys)) and all(torch.equal(a, b) for a, b in zip(got_bufs, want_bufs))
    _assert_same_state(stream.state(), want_states[-1], "first-order section")
    (carry,) = _leaves(stream.state().carries[_steps_of(rd, "first")[0]])
    assert carry.shape[-1] == 2 and carry[..., 0].any() and not carry[..., 1].any()
    assert_close(torch.cat(want_ys, -1).cpu(), _one_call(procs, x, params, rd)[0].cpu(), 1e-5, "first-order: vs one call")


# ---------------------------------------------------------------------------------------------------- 5: new parameters
def test_parameters_change_between_blocks():
    """update_parameters after block 3, then five more blocks: the eager stream given the new parameters from block 4 on,
    bit for bit (histories and envelopes carry on) -- and not the run without the update."""
    from grafx_amd.render import CapturedStream

    n = 512
    procs, x, p0, rd = _chain_setup(131, 8 * n)
    torch.manual_seed(132)
    p1 = {t: {k: v + 0.2 * torch.randn_like(v) for k, v in d.items()} for t, d in p0.items()}
    first_ys, _, first_states = _eager(procs, x, p0, rd, n, 3)
    then_ys, _, then_states = _eager(procs, x, p1, rd, n, 5, state=first_states[-1], first=3)
    stay_ys, _, _ = _eager(procs, x, p0, rd, n, 5, state=first_states[-1], first=3)
    stream = CapturedStream(procs, x[..., :n], p0, rd)
    got = _replay(stream, x, n, 3)[0]
    stream.update_parameters(p1)
    got += _replay(stream, x, n, 5, first=3)[0]
    for k, (a, b) in enumerate(zip(got, first_ys + then_ys)):
        assert torch.equal(a, b), f"block {k}"
    _assert_same_state(stream.state(), then_states[-1], "after the update")
    assert not torch.equal(got[3], stay_ys[0]) and not torch.equal(got[7], stay_ys[4])


# ---------------------------------------------------------------------------------------------------- 6: reset, state round trips
def test_reset_and_state_round_trips():
    from grafx_amd.render import CapturedStream, render_grafx

    n = 512
    procs, x, params, rd = _chain_setup(141, 9 * n)
    want_ys, _, want_states = _eager(procs, x, params, rd, n, 9)
    stream = CapturedStream(procs, x[..., :n], params, rd)
    first = _replay(stream, x, n, 8)[0]
    assert stream.samples == 8 * n
    stream.reset()
    assert stream.samples == 0
    again = _replay(stream, x, n, 8)[0]
    assert all(torch.equal(a, b) for a, b in zip(first, again)) and all(torch.equal(a, b) for a, b in zip(first, want_ys))
    # three eager blocks, then five captured ones from their state, which the replays leave alone
    loaded = want_states[2]
    kept = {i: [t.clone() for t in _leaves(c)] for i, c in loaded.carries.items()}
    stream.load_state(loaded)
    assert stream.samples == 3 * n
    rest = _replay(stream, x, n, 5, first=3)[0]
    assert all(torch.equal(a, b) for a, b in zip(rest, want_ys[3:8]))
    assert loaded.samples == 3 * n
    assert all(torch.equal(a, b) for i, c in loaded.carries.items() for a, b in zip(_leaves(c), kept[i], strict=True))
    # ... and the captured stream's state continues in the eager render
    handed = stream.state()
    _assert_same_state(handed, want_states[7], "state() after eight blocks")
    with torch.no_grad():
        y9, _, _, s9 = render_grafx(procs, x[..., 8 * n :], params, rd, state=handed, return_state=True)
    assert torch.equal(y9, want_ys[8])
    _assert_same_state(s9, want_states[8], "the eager block after state()")
    # a stream constructed from a state starts there
    resumed = CapturedStream(procs, x[..., :n], params, rd, state=want_states[2])
    assert resumed.samples == 3 * n and torch.equal(resumed(x[..., 3 * n : 4 * n])[0], want_ys[3])


# ---------------------------------------------------------------------------------------------------- 7: a container
def test_a_container_replays_the_eager_blocks():
    """SerialChain(BiquadFilter (fsm), Compressor (ballistics)) inside a graph: a tuple carry with a history and an
    envelope, four blocks of 512."""
    from grafx_amd.processors import BiquadFilter, SerialChain
    from grafx_amd.render import CapturedStream

    n, blocks = 512, 4
    biquad = BiquadFilter(num_filters=2, backend="fsm", flashfftconv=False, fsm_fir_len=256)
    procs = {"strip": SerialChain({"biquad": biquad, "comp": _comp()}).cuda()}
    G = _chain_graph(["in", "strip", "out"])
    rd, params, x = _render_data(G), _parameters(procs, G, 151), _signal(1, n * blocks, 152)
    want_ys, want_bufs, want_states = _eager(procs, x, params, rd, n, blocks)
    (step,) = _steps_of(rd, "strip")
    assert isinstance(want_states[-1].carries[step], tuple) and len(_leaves(want_states[-1].carries[step])) == 2
    stream = CapturedStream(procs, x[..., :n], params, rd)
    got_ys, got_bufs = _replay(stream, x, n, blocks)
    assert all(torch.equal(a, b) for a, b in zip(got_ys, want_ys)) and all(torch.equal(a, b) for a, b in zip(got_bufs, want_bufs))
    _assert_same_state(stream.state(), want_states[-1], "container")


# ---------------------------------------------------------------------------------------------------- 8: refusals
def test_refusals():
    """The eager path's refusals, raised by the constructor before anything is captured; a wrong block and a wrong state
    are refused by the call and leave the stream where it was."""
    from grafx_amd.render import CapturedStream, render_grafx

    n = 512
    procs, x, params, rd = _chain_setup(161, 2 * n)
    block = x[..., :n]
    with pytest.raises(ValueError, match=r"'compressor'.*iir_len"):
        CapturedStream(dict(procs, compressor=_comp("iir")), block, params, rd)
    wants = {t: {k: v.clone() for k, v in d.items()} for t, d in params.items()}
    wants["eq"]["log_gain"].requires_grad_()
    with pytest.raises(NotImplementedError, match="gradients"):
        CapturedStream(procs, block, wants, rd)
    with pytest.raises(ValueError, match="HIP path"):
        CapturedStream(procs, block.cpu(), params, rd)
    with torch.no_grad():
        other = render_grafx(procs, torch.cat([block, block[:1]]), params, rd, return_state=True)[3]
    with pytest.raises(ValueError, match="batch size 3.*batch size 2"):
        CapturedStream(procs, block, params, rd, state=other)
    want_ys, _, want_states = _eager(procs, x, params, rd, n, 2)
    stream = CapturedStream(procs, block, params, rd)
    assert torch.equal(stream(block)[0], want_ys[0])
    with pytest.raises(ValueError, match="511"):
        stream(x[..., : n - 1])
    with pytest.raises(ValueError, match="batch size 3.*batch size 2"):
        stream.load_state(other)
    with pytest.raises(ValueError, match="RenderState"):
        stream.load_state(other.carries)
    assert stream.samples == n
    assert torch.equal(stream(x[..., n:])[0], want_ys[1])
    _assert_same_state(stream.state(), want_states[1], "after the refusals")
