"""render_grafx(state=, return_state=): a graph rendered block by block is the graph rendered in one call, and the
history= / return_history= keywords of the frequency-sampled ("fsm") filters that make a default equaliser streamable.

The one-call reference runs under exact_convolution_scope(True): a stateful FIR call is the linear convolution by
definition, and the reference's odd-length aliasing has no block form.  Blocks are compared with the one call by
conftest.assert_close at the project's standing 1e-5 of the peak; the carried histories and the unchanged stateless
surface are compared bit for bit.  Shapes are the smallest at which the bookkeeping can go wrong: batch 2, stereo, a
256-tap equaliser, a 1001-tap reverb, 4095 samples cut into 1536 + 1 + 511 + 2047 (a one-sample block, blocks shorter than
the longest history of 1000 samples, odd lengths)."""
import warnings

import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

B, C, N_FSM, N_REV = 2, 2, 256, 1001
CUTS = (1536, 1, 511, 2047)
L = sum(CUTS)


def _exact():
    from grafx_amd.processors.core.convolution import exact_convolution_scope

    return exact_convolution_scope(True)


def _render_data(G):
    from grafx_amd.data import convert_to_tensor
    from grafx_amd.render import prepare_render, reorder_for_fast_render

    return prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam")).to("cuda")


def _parameters(procs, G, seed):
    """{type: {name: (nodes of the type, ...)}} (nested for containers), std 0.3, on the GPU."""
    from grafx_amd.utils import create_empty_parameters

    torch.manual_seed(seed)

    def plain(tree):
        return {k: plain(v) for k, v in tree.items()} if hasattr(tree, "items") else tree.detach().cuda()

    return plain(create_empty_parameters(procs, G, std=0.3))


def _signal(n_src, seed, batch=B):
    shape = (n_src, C, L) if batch is None else (batch, n_src, C, L)
    return (0.3 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).cuda()


def _eq(backend="fsm", channel="stereo"):
    from grafx_amd.processors import ParametricEqualizer

    return ParametricEqualizer(num_filters=4, processor_channel=channel, backend=backend, flashfftconv=False,
                               fsm_fir_len=N_FSM).cuda()


def _comp(smoother="ballistics"):
    from grafx_amd.processors import Compressor

    return Compressor(energy_smoother=smoother, iir_len=255, flashfftconv=False).cuda()


def _reverb():
    from grafx_amd.processors import STFTMaskedNoiseReverb

    return STFTMaskedNoiseReverb(ir_len=N_REV, flashfftconv=False).cuda()


def _chain_graph(types):
    from grafx_amd.data import GRAFX, NodeConfigs

    G = GRAFX(config=NodeConfigs(sorted(set(types) - {"in", "out", "mix"})))
    G.add_serial_chain(list(types))
    return G


def _console(n_ch=8, n_bus=2):
    """tests/test_routing_golden.py::build_console with an equaliser type of their own on the buses."""
    from grafx_amd.data import GRAFX, NodeConfigs

    G = GRAFX(config=NodeConfigs(["eq", "buseq", "compressor", "reverb"]))
    out_id = G.add("out")
    buses = [G.add("mix") for _ in range(n_bus)]
    send = G.add("mix")
    for ch in range(n_ch):
        _, last = G.add_serial_chain(["in", "eq", "compressor"])
        G.connect(last, buses[ch // (n_ch // n_bus)])
        G.connect(last, send)
    for b in buses:
        e, c = G.add("buseq"), G.add("compressor")
        G.connect(b, e)
        G.connect(e, c)
        G.connect(c, out_id)
    r = G.add("reverb")
    G.connect(send, r)
    G.connect(r, out_id)
    return G


def _one_call(procs, x, params, rd):
    from grafx_amd.render import render_grafx

    with torch.no_grad(), _exact(), warnings.catch_warnings():
        warnings.simplefilter("ignore")     # (a graph of containers takes the generic loop in its one call, and says so)
        return render_grafx(procs, x, params, rd)


def _blocks(procs, x, params, rd, cuts=CUTS, state=None, **kw):
    """The render in blocks (strided slices of x, as they are) -> (outputs, buffers, states after every block)."""
    from grafx_amd.render import render_grafx
    from grafx_amd.render.graph import GenericRenderPathWarning

    ys, bufs, states, pos = [], [], [], 0
    with torch.no_grad(), _exact(), warnings.catch_warnings():
        warnings.simplefilter("error", GenericRenderPathWarning)
        for n in cuts:
            y, inter, buf, state = render_grafx(procs, x[..., pos : pos + n], params, rd, state=state, return_state=True, **kw)
            assert inter == [] and y.shape[-1] == n
            ys.append(y.clone())
            bufs.append(buf)
            states.append(state)
            pos += n
    return ys, bufs, states


# ---------------------------------------------------------------------------------------------------- 1: a chain
def test_chain_blocks_equal_the_one_call_render():
    """in -> ParametricEqualizer (fsm) -> Compressor (ballistics) -> STFTMaskedNoiseReverb -> mix -> out: the output, every
    row of the signal buffer and the sample count."""
    from grafx_amd.render import RenderState

    procs = {"eq": _eq(), "compressor": _comp(), "reverb": _reverb()}
    G = _chain_graph(["in", "eq", "compressor", "reverb", "mix", "out"])
    rd, params, x = _render_data(G), _parameters(procs, G, 1), _signal(1, 2)
    want_y, _, want_buf = _one_call(procs, x, params, rd)
    ys, bufs, states = _blocks(procs, x, params, rd)
    assert all(isinstance(s, RenderState) for s in states)
    assert [s.samples for s in states] == [1536, 1537, 2048, 4095]
    assert_close(torch.cat(ys, -1).cpu(), want_y.cpu(), 1e-5, "chain: output")
    got_buf = torch.cat(bufs, -1)
    for row in range(want_buf.shape[1]):
        assert_close(got_buf[:, row].cpu(), want_buf[:, row].cpu(), 1e-5, f"chain: buffer row {row}")
    # per step: the equaliser's and the reverb's histories are the last N - 1 samples of what they read
    by_type = {t: states[-1].carries[i + 1] for i, (t, _) in enumerate(states[-1].steps) if t in procs}
    assert tuple(by_type["eq"].shape) == (B, C, N_FSM - 1) and tuple(by_type["reverb"].shape) == (B, C, N_REV - 1)
    assert torch.equal(by_type["eq"].view(B, 1, C, -1), x[..., L - (N_FSM - 1) :])
    assert tuple(by_type["compressor"].shape) == (B, 1, 1)


# ---------------------------------------------------------------------------------------------------- 2: the console
@pytest.mark.parametrize("variant", ["shared_rows", "output_only", "unbatched"])
def test_console_ballistics_blocks_equal_the_one_call_render(variant):
    """The 8-strip / 2-bus console with ballistics compressors, fsm equalisers on the strips and an lfilter equaliser on
    the buses; its routing sums run as gather-sums of their own.  ``shared_rows``: a (B, n, C, L) input, the per-node
    parameters shared by the batch; ``output_only``: the same with keep_signal_buffer=False; ``unbatched``: (n, C, L)."""
    procs = {"eq": _eq(), "buseq": _eq("lfilter"), "compressor": _comp(), "reverb": _reverb()}
    G = _console()
    rd, params = _render_data(G), _parameters(procs, G, 3)
    x = _signal(8, 4, batch=None if variant == "unbatched" else B)
    want_y, _, want_buf = _one_call(procs, x, params, rd)
    ys, bufs, states = _blocks(procs, x, params, rd, keep_signal_buffer=variant != "output_only")
    assert states[-1].samples == L and states[-1].batch == (None if variant == "unbatched" else B)
    assert_close(torch.cat(ys, -1).cpu(), want_y.cpu(), 1e-5, f"console ({variant}): output")
    if variant == "output_only":
        assert all(b is None for b in bufs)
        return
    got_buf = torch.cat(bufs, -1)
    node_dim = got_buf.ndim - 3
    for row in range(want_buf.shape[node_dim]):
        assert_close(got_buf.select(node_dim, row).cpu(), want_buf.select(node_dim, row).cpu(), 1e-5,
                     f"console ({variant}): buffer row {row}")


# ---------------------------------------------------------------------------------------------------- 3: one type, two steps
def test_a_type_spread_over_two_steps_keeps_one_carry_per_step():
    """equaliser -> compressor -> equaliser of the same type: two render steps of type "eq", each with its own history.
    Swapping the two by hand changes the next block, so the comparison would see a mix-up."""
    from grafx_amd.render import RenderState, render_grafx

    procs = {"eq": _eq(), "compressor": _comp()}
    G = _chain_graph(["in", "eq", "compressor", "eq", "out"])
    rd, params, x = _render_data(G), _parameters(procs, G, 5), _signal(1, 6)
    eq_steps = [i for i in range(1, rd.max_order + 1) if rd.iter_list[i].node_type == "eq"]
    assert len(eq_steps) == 2
    want_y, _, want_buf = _one_call(procs, x, params, rd)
    ys, bufs, states = _blocks(procs, x, params, rd)
    assert_close(torch.cat(ys, -1).cpu(), want_y.cpu(), 1e-5, "eq-compressor-eq: output")
    assert_close(torch.cat(bufs, -1).cpu(), want_buf.cpu(), 1e-5, "eq-compressor-eq: buffer")
    first = states[0]
    a, b = (first.carries[i] for i in eq_steps)
    assert a.shape == b.shape and not torch.equal(a, b)
    swapped = RenderState(first.batch, first.channels, first.device, first.steps,
                          {**first.carries, eq_steps[0]: b, eq_steps[1]: a}, first.samples)
    with torch.no_grad(), _exact():
        y_swapped = render_grafx(procs, x[..., 1536:2048], params, rd, state=swapped, return_state=True)[0]
        y_right = render_grafx(procs, x[..., 1536:2048], params, rd, state=first, return_state=True)[0]
    want = want_y[..., 1536:2048]
    assert_close(y_right.cpu(), want.cpu(), 1e-5, "eq-compressor-eq: the block after the first")
    assert float((y_swapped - want).abs().max()) > 1e-3 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------------- 4: containers
def test_containers_carry_their_childrens_carries():
    """SerialChain(equaliser, compressor) -> DryWet(reverb) inside a graph: the carry of a container is the tuple of its
    children's carries."""
    from grafx_amd.processors import DryWet, SerialChain

    procs = {"strip": SerialChain({"eq": _eq(), "comp": _comp()}).cuda(), "wet": DryWet(_reverb(), external_param=False).cuda()}
    G = _chain_graph(["in", "strip", "wet", "out"])
    rd, params, x = _render_data(G), _parameters(procs, G, 7), _signal(1, 8)
    want_y, _, want_buf = _one_call(procs, x, params, rd)
    ys, bufs, states = _blocks(procs, x, params, rd)
    assert_close(torch.cat(ys, -1).cpu(), want_y.cpu(), 1e-5, "containers: output")
    assert_close(torch.cat(bufs, -1).cpu(), want_buf.cpu(), 1e-5, "containers: buffer")
    strip, wet = (states[-1].carries[i + 1] for i, (t, _) in enumerate(states[-1].steps) if t in procs)
    assert isinstance(strip, tuple) and len(strip) == 2 and isinstance(wet, tuple) and len(wet) == 1
    assert tuple(strip[0].shape) == (B, C, N_FSM - 1) and tuple(wet[0].shape) == (B, C, N_REV - 1)


# ---------------------------------------------------------------------------------------------------- 5: fsm alone
def _coefficients(R, Cf, K, seed):
    """Stable second-order sections (pole radius 0.3 .. 0.8, so the 256 sampled taps hold the whole response)."""
    g = torch.Generator().manual_seed(seed)
    r = 0.3 + 0.5 * torch.rand(R, Cf, K, generator=g)
    th = 0.2 + 2.5 * torch.rand(R, Cf, K, generator=g)
    As = torch.stack([torch.ones_like(r), -2 * r * torch.cos(th), r * r], -1)
    Bs = torch.randn(R, Cf, K, 3, generator=g) * 0.5 + torch.tensor([1.0, 0.0, 0.0])
    return Bs, As


def _fsm_cases():
    from grafx_amd.processors import BiquadFilter, IIRFilter

    R = 3
    Bs, As = _coefficients(R, C, 2, 11)
    g = torch.Generator().manual_seed(12)
    yield "IIRFilter", IIRFilter(order=2, backend="fsm", flashfftconv=False, fsm_fir_len=N_FSM), C, \
        {"Bs": Bs.cuda(), "As": As.cuda()}, lambda x: x
    m = BiquadFilter(num_filters=2, backend="fsm", flashfftconv=False, fsm_fir_len=N_FSM).cuda()
    yield "BiquadFilter", m, C, {"Bs": torch.randn(R, 2, 3, generator=g).cuda(), "A1_pre": 0.3 * torch.randn(R, 2, generator=g).cuda(),
                                 "A2_pre": 0.3 * torch.randn(R, 2, generator=g).cuda()}, lambda x: x
    from grafx_amd.processors.core.midside import lr_to_ms

    for channel in ("mono", "stereo", "midside"):
        m = _eq("fsm", channel)
        p = {k: 0.3 * torch.randn(R, 1 if channel == "mono" else 2, 4, generator=g).cuda() for k in ("w0", "q_inv", "log_gain")}
        yield f"ParametricEqualizer-{channel}", m, C, p, (lr_to_ms if channel == "midside" else (lambda x: x))


@pytest.mark.parametrize("case", range(5), ids=["IIRFilter", "BiquadFilter", "peq-mono", "peq-stereo", "peq-midside"])
def test_fsm_filters_stream_through_an_input_history(case):
    """Blocks against one call, and the leaving history = the last N - 1 samples the convolution read, bit for bit."""
    name, m, Cin, p, reads = list(_fsm_cases())[case]
    x = (0.5 * torch.randn(3, Cin, L, generator=torch.Generator().manual_seed(20 + case))).cuda()
    with torch.no_grad(), _exact():
        whole = m(x, **p)
        out, pos, hist = [], 0, None
        for n in CUTS:
            y, hist = m(x[..., pos : pos + n].contiguous(), **p, history=hist, return_history=True)
            pos += n
            out.append(y)
            assert tuple(hist.shape) == (3, Cin, N_FSM - 1)
            assert torch.equal(hist, reads(x)[..., pos - (N_FSM - 1) : pos]), f"{name}: history after {pos} samples"
        # a history without return_history: the plain output
        y_only = m(x[..., :100].contiguous(), **p, history=torch.zeros(3, Cin, N_FSM - 1, device="cuda"))
    assert_close(torch.cat(out, -1).cpu(), whole.cpu(), 1e-5, f"{name}: blocks vs one call")
    assert isinstance(y_only, torch.Tensor)
    assert_close(y_only.cpu(), whole[..., :100].cpu(), 1e-5, f"{name}: a history without return_history")


@pytest.mark.parametrize("shared", [False, True], ids=["rows", "shared"])
def test_prepared_equaliser_spectra_take_a_history(shared):
    """ParametricEqualizer.prepare() + render_into(_prepared=, history=) on strided (B, n, C, L) views: what the render's
    side stream would hand it is usable with a history, per row and shared by the batch."""
    m, n = _eq(), 3
    g = torch.Generator().manual_seed(31)
    p = {k: 0.3 * torch.randn(n if shared else B * n, 2, 4, generator=g).cuda() for k in ("w0", "q_inv", "log_gain")}
    extra = {"_shared_rows": n} if shared else {}
    x = (0.5 * torch.randn(B, n + 1, C, L, generator=g)).cuda()
    with torch.no_grad(), _exact():
        prep = m.prepare(**p, **extra)
        assert prep is not None
        whole = torch.empty(B, n, C, L, device="cuda")
        m.render_into(x[:, 1:], whole, **extra, **p)
        got = torch.full((B, n + 1, C, L), float("nan"), device="cuda")
        pos, hist = 0, None
        for k in CUTS:
            _, hist = m.render_into(x[:, 1:, :, pos : pos + k], got[:, :n, :, pos : pos + k], _prepared=prep, history=hist,
                                    return_history=True, **extra, **p)
            pos += k
    assert torch.isnan(got[:, n]).all()
    assert torch.equal(hist.view(B, n, C, -1), x[:, 1:, :, L - (N_FSM - 1) :])
    assert_close(got[:, :n].cpu(), whole.cpu(), 1e-5, "prepared spectra with a history")


def _fsm_taps64(Bs, As, N):
    """The frequency-sampled taps (reference core/iir.py:147-150) in float64 torch ops."""
    k = torch.arange(N // 2 + 1, dtype=torch.float64)
    d = torch.arange(3, dtype=torch.float64)
    delays = torch.exp(-1j * (d[:, None] * k[None, :]) / N * 2 * torch.pi)
    resp = ((Bs.unsqueeze(-1) * delays).sum(-2) / (As.unsqueeze(-1) * delays).sum(-2)).prod(-2)
    return torch.fft.irfft(resp, n=N, dim=-1)


def test_fsm_gradients_of_a_two_block_chain():
    """x, the coefficients and the entering history of IIRFilter(backend="fsm") from random cotangents of both blocks'
    outputs and of the last history, against float64 autograd of the same chain: 1e-5, the bound
    tests/test_gpu_fftconv_state.py::test_gradients_of_a_two_block_chain holds the same convolution to."""
    from grafx_amd.processors import IIRFilter

    m = IIRFilter(order=2, backend="fsm", flashfftconv=False, fsm_fir_len=N_FSM)
    g = torch.Generator().manual_seed(41)
    R, L1, L2, N = 2, 700, 801, N_FSM
    x1, x2 = torch.randn(R, C, L1, generator=g), torch.randn(R, C, L2, generator=g)
    Bs, As = _coefficients(R, C, 2, 42)
    zi = torch.randn(R, C, N - 1, generator=g)
    w1, w2, wz = torch.randn(R, C, L1, generator=g), torch.randn(R, C, L2, generator=g), torch.randn(R, C, N - 1, generator=g)

    def native(x, Bs, As, z):
        return m(x, Bs, As, history=z, return_history=True)

    def ref64(x, Bs, As, z):
        h = _fsm_taps64(Bs, As, N)
        xx = torch.cat([z, x], -1)
        n = 1 << (xx.shape[-1] + N).bit_length()
        full = torch.fft.irfft(torch.fft.rfft(xx, n=n) * torch.fft.rfft(h, n=n), n=n)
        return full[..., N - 1 : N - 1 + x.shape[-1]], xx[..., xx.shape[-1] - (N - 1) :]

    def chain(x1, x2, Bs, As, zi, block):
        y1, z1 = block(x1, Bs, As, zi)
        y2, z2 = block(x2, Bs, As, z1)
        return y1, y2, z2

    leaves = [t.cuda().requires_grad_() for t in (x1, x2, Bs, As, zi)]
    y1, y2, z2 = chain(*leaves, native)
    got = torch.autograd.grad((y1 * w1.cuda()).sum() + (y2 * w2.cuda()).sum() + (z2 * wz.cuda()).sum(), leaves)
    leaves64 = [t.double().requires_grad_() for t in (x1, x2, Bs, As, zi)]
    r1, r2, rz = chain(*leaves64, ref64)
    want = torch.autograd.grad((r1 * w1.double()).sum() + (r2 * w2.double()).sum() + (rz * wz.double()).sum(), leaves64)
    assert_close(y1.detach().cpu(), r1.detach(), 1e-5, "fsm y block 1")
    assert_close(y2.detach().cpu(), r2.detach(), 1e-5, "fsm y block 2")
    assert torch.equal(z2.detach().cpu(), rz.detach().float())
    for name, a, b in zip(("grad x1", "grad x2", "grad Bs", "grad As", "grad history"), got, want):
        assert_close(a.cpu(), b, 1e-5, f"fsm {name}")


@pytest.mark.parametrize("kind", ["peq-stereo", "peq-midside", "biquad"])
def test_fsm_processor_gradients_of_blocks_equal_the_one_call_gradients(kind):
    """ParametricEqualizer / BiquadFilter with gradients go through autograd.convolve(state=): the parameter and input
    gradients of a two-block chain are those of the one call."""
    _, m, Cin, p, _ = list(_fsm_cases())[{"biquad": 1, "peq-stereo": 3, "peq-midside": 4}[kind]]
    x = (0.5 * torch.randn(3, Cin, 1500, generator=torch.Generator().manual_seed(51))).cuda()
    w = torch.randn(3, Cin, 1500, generator=torch.Generator().manual_seed(52)).cuda()

    def grads(run):
        xs = x.clone().requires_grad_()
        ps = {k: v.clone().requires_grad_() for k, v in p.items()}
        with _exact():
            y = run(xs, ps)
        return y.detach(), torch.autograd.grad((y * w).sum(), [xs, *ps.values()])

    def blocks(xs, ps):
        y1, h = m(xs[..., :699], **ps, return_history=True)
        y2 = m(xs[..., 699:], **ps, history=h)
        return torch.cat([y1, y2], -1)

    y_whole, g_whole = grads(lambda xs, ps: m(xs, **ps))
    y_blocks, g_blocks = grads(blocks)
    assert_close(y_blocks.cpu(), y_whole.cpu(), 1e-5, f"{kind}: output with gradients")
    for name, a, b in zip(["x", *p], g_blocks, g_whole):
        assert_close(a.cpu(), b.cpu(), 1e-5, f"{kind}: gradient of {name}")


def test_fsm_keeps_refusing_state_and_the_recursive_backends_refuse_history():
    from grafx_amd.processors import BiquadFilter, IIRFilter

    x = torch.randn(2, C, 64, device="cuda")
    Bs, As = (t.cuda() for t in _coefficients(2, C, 1, 61))
    with pytest.raises(ValueError, match="no recursive state.*recursive backends"):
        IIRFilter(backend="fsm", flashfftconv=False, fsm_fir_len=N_FSM)(x, Bs, As, return_state=True)
    with pytest.raises(ValueError, match="no recursive state.*recursive backends"):
        _eq()(x, **{k: torch.zeros(2, 2, 4, device="cuda") for k in ("w0", "q_inv", "log_gain")}, return_state=True)
    for backend in ("lfilter", "ssm"):
        with pytest.raises(ValueError, match="history.*frequency-sampled.*state"):
            IIRFilter(backend=backend)(x, Bs, As, return_history=True)
        with pytest.raises(ValueError, match="history.*frequency-sampled.*state"):
            IIRFilter(backend=backend)(x, Bs, As, history=torch.zeros(2, C, N_FSM - 1, device="cuda"))
    with pytest.raises(ValueError, match="history.*frequency-sampled.*state"):
        BiquadFilter(num_filters=1, backend="lfilter")(x, torch.randn(2, 1, 3, device="cuda"), torch.zeros(2, 1, device="cuda"),
                                                        torch.zeros(2, 1, device="cuda"), return_history=True)
    with pytest.raises(ValueError, match="state must be a float32 tensor of shape"):
        IIRFilter(backend="fsm", flashfftconv=False, fsm_fir_len=N_FSM)(x, Bs, As, history=torch.zeros(2, C, 7, device="cuda"))


# ---------------------------------------------------------------------------------------------------- 6: refusals
class _PlainGain(torch.nn.Module):
    def forward(self, input_signals, log_gain):
        return input_signals * torch.exp(log_gain)[..., None]

    def render_into(self, x4, out4, log_gain):
        out4.copy_(x4 * torch.exp(log_gain).view(*x4.shape[:2], -1, 1))

    def parameter_size(self):
        return {"log_gain": 2}


def test_refusals_leave_the_buffer_and_the_state_alone():
    from grafx_amd.render import RenderState, render_grafx

    good = {"eq": _eq(), "compressor": _comp(), "reverb": _reverb()}
    G = _chain_graph(["in", "eq", "compressor", "reverb", "mix", "out"])
    rd, params, x = _render_data(G), _parameters(good, G, 71), _signal(1, 72)
    block = x[..., :300]
    with torch.no_grad(), _exact():
        _, _, _, state = render_grafx(good, block, params, rd, return_state=True)
    kept = {i: c.clone() for i, c in state.carries.items()}

    def unchanged():
        assert state.samples == 300 and set(state.carries) == set(kept)
        assert all(torch.equal(state.carries[i], kept[i]) for i in kept)
        assert torch.equal(x, x_before)

    x_before = x.clone()
    # the truncated one-pole smoother: refused by node type, with the processor's own reason, before any launch
    bad = dict(good, compressor=_comp("iir"))
    for st in (None, state):
        with torch.no_grad(), pytest.raises(ValueError, match=r"'compressor'.*iir_len"):
            render_grafx(bad, block, params, rd, state=st, return_state=True)
        unchanged()
    # a processor without the block protocol: by name
    G2 = _chain_graph(["in", "gain", "out"])
    rd2 = _render_data(G2)
    with torch.no_grad(), pytest.raises(ValueError, match=r"'gain' \(_PlainGain\) has no stream_block"):
        render_grafx({"gain": _PlainGain()}, block, {"gain": {"log_gain": torch.zeros(1, 2, device="cuda")}}, rd2,
                     return_state=True)
    # a state made for another batch size, another channel count, another graph
    with torch.no_grad(), pytest.raises(ValueError, match="batch size 2.*batch size 3"):
        render_grafx(good, torch.cat([block, block[:1]]), params, rd, state=state, return_state=True)
    with torch.no_grad(), pytest.raises(ValueError, match="batch size 2.*unbatched"):
        render_grafx(good, block[0], params, rd, state=state, return_state=True)
    G3 = _chain_graph(["in", "eq", "compressor", "eq", "out"])
    with torch.no_grad(), pytest.raises(ValueError, match="steps|render step"):
        render_grafx(good, block, _parameters(good, G3, 73), _render_data(G3), state=state, return_state=True)
    with torch.no_grad(), pytest.raises(ValueError, match="RenderState"):
        render_grafx(good, block, params, rd, state=kept, return_state=True)
    unchanged()
    # gradients through a streamed graph are a later feature
    wants = {t: {k: v.clone() for k, v in d.items()} for t, d in params.items()}
    wants["eq"]["log_gain"].requires_grad_()
    with pytest.raises(NotImplementedError, match="gradients"):
        render_grafx(good, block, wants, rd, state=state, return_state=True)
    with pytest.raises(NotImplementedError, match="gradients"):
        render_grafx(good, block.clone().requires_grad_(), params, rd, return_state=True)
    unchanged()
    assert isinstance(state, RenderState)


def test_a_compressor_without_a_smoother_is_memoryless():
    """Compressor(energy_smoother=None) raises for state= in a plain call (no state to carry); in a streamed graph it is a
    memoryless stage."""
    procs = {"compressor": _comp(None)}
    G = _chain_graph(["in", "compressor", "out"])
    rd, params, x = _render_data(G), _parameters(procs, G, 81), _signal(1, 82)
    want_y, _, _ = _one_call(procs, x, params, rd)
    ys, _, states = _blocks(procs, x, params, rd)
    assert_close(torch.cat(ys, -1).cpu(), want_y.cpu(), 1e-5, "smoother-less compressor")
    assert all(c is None for c in states[-1].carries.values())


# ---------------------------------------------------------------------------------------------------- 7: unchanged surface
def test_the_stateless_surface_is_unchanged():
    """Without the new arguments: three return values, and the same bits as the first block of a streamed render."""
    from grafx_amd.render import render_grafx

    procs = {"eq": _eq(), "compressor": _comp(), "reverb": _reverb()}
    G = _chain_graph(["in", "eq", "compressor", "reverb", "mix", "out"])
    rd, params, x = _render_data(G), _parameters(procs, G, 91), _signal(1, 92)
    with torch.no_grad(), _exact():
        plain = render_grafx(procs, x, params, rd)
        streamed = render_grafx(procs, x, params, rd, return_state=True)
        with_none = render_grafx(procs, x, params, rd, state=None, return_state=False)
    assert len(plain) == 3 and len(streamed) == 4 and len(with_none) == 3
    assert streamed[3].samples == L
    assert torch.equal(plain[0], streamed[0])
    assert torch.equal(plain[2], streamed[2])
