"""STFTMaskedNoiseReverb under gradients: the taps come from the native node autograd.StftReverbIrFn (inference kernel
forward, gfx_stft_reverb_ir_bwd_f32 backward) at n_fft = 384 / hop = 192, from the torch chain at any other transform size.
Module calls (every channel mode, gain envelope, fresh noise per row, compute_ir, a two-block stream) and graphs rendered by
render_grafx, parameter and input gradients against float64 autograd of the oracle on the CPU at the project's 1e-5 of each
gradient's own peak.  All lengths keep L + N - 1 even, where the reference's convolution is the linear one."""
import pytest
import torch

from conftest import assert_close
from reverb_float64 import taps64

pytestmark = pytest.mark.gpu

R, IR_LEN, L = 2, 1536, 2049


def _nodes(y):
    """Names of every autograd node reachable from y."""
    seen, todo, names = set(), [y.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


def _assert_native(y):
    names = _nodes(y)
    assert "StftReverbIrFnBackward" in names and "IrdftFnBackward" not in names, sorted(names)


def _module(channel="pseudo_midside", genv=False, **kw):
    from grafx_amd.processors import STFTMaskedNoiseReverb

    return STFTMaskedNoiseReverb(ir_len=IR_LEN, processor_channel=channel, gain_envelope=genv, flashfftconv=False, **kw).cuda()


def _inputs(m, seed, rows=R, length=L):
    gen = torch.Generator().manual_seed(seed)
    C = 1 if m.processor_channel == "mono" else 2
    x = torch.randn(rows, C, length, generator=gen)
    p = {k: torch.randn(rows, *shape, generator=gen) for k, shape in m.parameter_size().items()}
    w = torch.randn(rows, 2, length, generator=gen)
    return x, p, w


def _oracle(m, noise=None):
    import oracle

    o = oracle.OracleSTFTMaskedNoiseReverb(ir_len=m.ir_len, processor_channel=m.processor_channel, n_fft=m.n_fft,
                                           hop_length=m.hop_length, gain_envelope=m.gain_envelope)
    if noise is not None:
        o.noise_stft = noise.detach().cpu()
    return o


def _compare(m, x, p, w, what, noise=None, scope=None):
    """m(x, **p).backward(w) against the oracle in float64: input and parameter gradients."""
    from contextlib import nullcontext

    xg = x.cuda().requires_grad_()
    pg = {k: v.cuda().requires_grad_() for k, v in p.items()}
    with scope if scope is not None else nullcontext():
        y = m(xg, **pg)
        _assert_native(y)
        got = torch.autograd.grad(y, [xg, *pg.values()], w.cuda())
    x64 = x.double().requires_grad_()
    p64 = {k: v.double().requires_grad_() for k, v in p.items()}
    y64 = _oracle(m, noise)(x64, **p64)
    want = torch.autograd.grad(y64, [x64, *p64.values()], w.double())
    assert_close(y.detach().cpu().double(), y64.detach(), 1e-5, f"{what}: output")
    for name, a, b in zip(["input", *p], got, want):
        assert_close(a.cpu().double(), b, 1e-5, f"{what}: gradient of {name}")


@pytest.mark.parametrize("genv", [False, True])
@pytest.mark.parametrize("channel", ["mono", "stereo", "midside", "pseudo_midside"])
def test_module_gradients(channel, genv):
    from grafx_amd.processors.core.convolution import exact_convolution_scope

    m = _module(channel, genv)
    x, p, w = _inputs(m, 1 + genv)
    _compare(m, x, p, w, f"{channel}, gain envelope {genv}", scope=exact_convolution_scope(True))


def test_module_gradients_under_the_default_aliasing():
    m = _module("pseudo_midside", True)
    x, p, w = _inputs(m, 3)
    _compare(m, x, p, w, "default convolution setting")


def test_module_gradients_with_fresh_noise_per_row():
    """fixed_noise=False: the node saves the noise its forward drew; the reference gets the same noise (captured)."""
    from grafx_amd.processors.core.convolution import exact_convolution_scope

    m = _module("pseudo_midside", True, fixed_noise=False)
    torch.manual_seed(4)
    noise = m.sample_noise(R, torch.device("cuda"))
    drawn = []
    m.sample_noise = lambda n, device: drawn.append(n) or noise
    x, p, w = _inputs(m, 4)
    _compare(m, x, p, w, "fresh noise per row", noise=noise, scope=exact_convolution_scope(True))
    assert drawn == [R]


def test_compute_ir_gradients():
    m = _module("midside", True)
    _, p, _ = _inputs(m, 5)
    gh = torch.randn(R, 2, IR_LEN, generator=torch.Generator().manual_seed(6))
    pg = {k: v.cuda().requires_grad_() for k, v in p.items()}
    ir = m.compute_ir(**pg)
    _assert_native(ir)
    with torch.no_grad():
        assert torch.equal(ir.detach(), m.compute_ir(**{k: v.detach() for k, v in pg.items()}))
    got = torch.autograd.grad(ir, list(pg.values()), gh.cuda())
    p64 = {k: v.double().requires_grad_() for k, v in p.items()}
    ir64 = taps64(m.noise_stft, m.window, p64["init_log_magnitude"], p64["delta_log_magnitude"],
                  p64["gain_env_log_magnitude"], IR_LEN, False, False)
    want = torch.autograd.grad(ir64, list(p64.values()), gh.double())
    for name, a, b in zip(p, got, want):
        assert_close(a.cpu().double(), b, 1e-5, f"compute_ir: gradient of {name}")


def test_two_block_stream_gradients():
    """forward(state=, return_state=True) twice with gradients: both blocks, the parameters and the entering state, with
    cotangents on both outputs and on the leaving state, against the float64 linear convolution of the whole."""
    m = _module("pseudo_midside", True)
    L1, L2, N = 1025, 1024, IR_LEN
    x, p, w = _inputs(m, 7, length=L1 + L2)
    gen = torch.Generator().manual_seed(8)
    zi, wz = torch.randn(R, 2, N - 1, generator=gen), torch.randn(R, 2, N - 1, generator=gen)
    leaves = [t.cuda().requires_grad_() for t in (x[..., :L1], x[..., L1:], zi, *p.values())]
    pg = dict(zip(p, leaves[3:]))
    y1, s1 = m(leaves[0], **pg, state=leaves[2], return_state=True)
    y2, s2 = m(leaves[1], **pg, state=s1, return_state=True)
    _assert_native(y2)
    loss = (torch.cat([y1, y2], -1) * w.cuda()).sum() + (s2 * wz.cuda()).sum()
    got = torch.autograd.grad(loss, leaves)

    leaves64 = [t.double().requires_grad_() for t in (x[..., :L1], x[..., L1:], zi, *p.values())]
    p64 = dict(zip(p, leaves64[3:]))
    h = taps64(m.noise_stft, m.window, p64["init_log_magnitude"], p64["delta_log_magnitude"],
               p64["gain_env_log_magnitude"], IR_LEN, True, True)
    whole = torch.cat([leaves64[2], leaves64[0], leaves64[1]], -1)  # history, block 1, block 2
    n = 1 << (whole.shape[-1] + N).bit_length()
    full = torch.fft.irfft(torch.fft.rfft(whole, n=n) * torch.fft.rfft(h, n=n), n=n)
    y64 = full[..., N - 1 : N - 1 + L1 + L2]
    s64 = whole[..., whole.shape[-1] - (N - 1):]
    want = torch.autograd.grad((y64 * w.double()).sum() + (s64 * wz.double()).sum(), leaves64)
    assert_close(torch.cat([y1, y2], -1).detach().cpu().double(), y64.detach(), 1e-5, "stream: output")
    assert_close(s2.detach().cpu().double(), s64.detach(), 1e-5, "stream: leaving state")
    for name, a, b in zip(["block 1", "block 2", "entering state", *p], got, want):
        assert_close(a.cpu().double(), b, 1e-5, f"stream: gradient of {name}")


def test_other_transform_sizes_keep_the_torch_chain():
    from grafx_amd.processors import STFTMaskedNoiseReverb

    m = STFTMaskedNoiseReverb(ir_len=1500, n_fft=256, hop_length=128, flashfftconv=False).cuda()
    x, p, w = _inputs(m, 9)
    xg = x.cuda().requires_grad_()
    pg = {k: v.cuda().requires_grad_() for k, v in p.items()}
    y = m(xg, **pg)
    names = _nodes(y)
    assert "IrdftFnBackward" in names and "StftReverbIrFnBackward" not in names, sorted(names)
    got = torch.autograd.grad(y, [xg, *pg.values()], w.cuda())
    x64 = x.double().requires_grad_()
    p64 = {k: v.double().requires_grad_() for k, v in p.items()}
    want = torch.autograd.grad(_oracle(m)(x64, **p64), [x64, *p64.values()], w.double())
    for name, a, b in zip(["input", *p], got, want):
        assert_close(a.cpu().double(), b, 1e-5, f"n_fft 256: gradient of {name}")


def test_midside_inference_blocks_write_the_given_buffer():
    """processor_channel="midside" without gradients, with state= and _out=: the block is written into _out, the state
    that comes back is the last ir_len - 1 samples of the mid/side signal fed in (zeros before the first), and two blocks
    concatenate to the one-call output under exact convolution, at the 1e-5 of the peak of the stream tests of
    test_gpu_render_state.py.  400 taps are 3 frames; 1000 samples cut at 333, the first block shorter than the history."""
    from grafx_amd.processors import STFTMaskedNoiseReverb
    from grafx_amd.processors.core.convolution import exact_convolution_scope
    from grafx_amd.processors.core.midside import lr_to_ms

    rows, N, length, cut = 3, 400, 1000, 333
    m = STFTMaskedNoiseReverb(ir_len=N, processor_channel="midside", flashfftconv=False).cuda()
    x, p, _ = _inputs(m, 10, rows=rows, length=length)
    x, p = x.cuda(), {k: v.cuda() for k, v in p.items()}
    with torch.no_grad(), exact_convolution_scope(True):
        want = m(x, **p)
        out = torch.full_like(x, float("nan"))
        y1, s1 = m(x[..., :cut], **p, _out=out[..., :cut], return_state=True)
        y2, s2 = m(x[..., cut:], **p, _out=out[..., cut:], state=s1, return_state=True)
    assert y1.data_ptr() == out.data_ptr() and y2.data_ptr() == out[..., cut:].data_ptr()
    assert torch.equal(y1, out[..., :cut]) and torch.equal(y2, out[..., cut:])
    fed = torch.cat([x.new_zeros(rows, 2, N - 1), lr_to_ms(x)], -1)
    assert tuple(s1.shape) == tuple(s2.shape) == (rows, 2, N - 1)
    assert torch.equal(s1, fed[..., cut : cut + N - 1]) and torch.equal(s2, fed[..., length:])
    assert_close(out.cpu(), want.cpu(), 1e-5, "midside blocks into _out against the one call")


# ------------------------------------------------------------------------------------------------ through render_grafx
B, LR, N_REV, N_FSM, N_IIR = 2, 4096, 1501, 257, 255


def _graph(kind):
    from grafx_amd.data import GRAFX, NodeConfigs

    if kind == "chain":
        G = GRAFX(config=NodeConfigs(["eq", "reverb"]))
        G.add_serial_chain(["in", "eq", "reverb", "out"])
        return G
    from test_routing_golden import build_console

    return build_console(8, 2)


def _processors(kind, per_row):
    import oracle
    from grafx_amd.processors import Compressor, ParametricEqualizer, STFTMaskedNoiseReverb

    class PerRowReverb(STFTMaskedNoiseReverb):
        """Takes the batch-expanded parameters: one parameter row, and one impulse response, per signal row."""
        accepts_shared_params = False

    reverb = (PerRowReverb if per_row else STFTMaskedNoiseReverb)(ir_len=N_REV, flashfftconv=False).cuda()
    hip = {"eq": ParametricEqualizer(num_filters=4, flashfftconv=False, fsm_fir_len=N_FSM).cuda(), "reverb": reverb}
    cpu = {"eq": oracle.OracleParametricEqualizer(num_filters=4, fsm_fir_len=N_FSM),
           "reverb": oracle.OracleSTFTMaskedNoiseReverb(ir_len=N_REV)}
    if kind == "console":
        hip["compressor"] = Compressor(energy_smoother="iir", iir_len=N_IIR, flashfftconv=False).cuda()
        cpu["compressor"] = oracle.OracleCompressor(energy_smoother="iir", iir_len=N_IIR)
    return hip, cpu


_REFERENCE = {}


def _reference(kind):
    """Inputs of the graph and the float64 oracle render's parameter gradients, computed once per graph."""
    if kind not in _REFERENCE:
        from grafx_amd.data import convert_to_tensor
        from grafx_amd.render import prepare_render, render_grafx, reorder_for_fast_render
        from grafx_amd.utils import create_empty_parameters

        G = _graph(kind)
        hip, cpu = _processors(kind, False)
        torch.manual_seed(21)
        tree = create_empty_parameters(hip, G, std=0.3)
        params = {t: {k: v.detach().clone() for k, v in d.items()} for t, d in tree.items()}
        n_src = 1 if kind == "chain" else 8
        x = 0.3 * torch.randn(B, n_src, 2, LR)
        w = torch.randn(B, 1, 2, LR)
        rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam"))
        p64 = {t: {k: v.double().requires_grad_() for k, v in d.items()} for t, d in params.items()}
        y64 = render_grafx(cpu, x.double(), p64, rd)[0]
        leaves = [v for d in p64.values() for v in d.values()]
        grads = torch.autograd.grad((y64.reshape(w.shape) * w.double()).sum(), leaves)
        _REFERENCE[kind] = (G, params, x, w, y64.detach(), grads)
    return _REFERENCE[kind]


@pytest.mark.parametrize("per_row", [False, True], ids=["batch_shared", "per_row"])
@pytest.mark.parametrize("kind", ["chain", "console"])
def test_training_through_render_grafx(kind, per_row, monkeypatch):
    from grafx_amd import ops
    from grafx_amd.data import convert_to_tensor
    from grafx_amd.render import prepare_render, render_grafx, reorder_for_fast_render

    # the render's backward hides its stages behind one node of its own: that the reverb's taps are differentiated by the
    # native kernel is seen at the wrapper the node calls (rows of every call)
    native_rows, native = [], ops.stft_reverb_ir_bwd

    def counted(grad_ir, *args, **kw):
        native_rows.append(grad_ir.shape[0])
        return native(grad_ir, *args, **kw)

    monkeypatch.setattr(ops, "stft_reverb_ir_bwd", counted)
    G, params, x, w, y64, want = _reference(kind)
    hip, _ = _processors(kind, per_row)
    rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam")).to("cuda")
    pg = {t: {k: v.cuda().requires_grad_() for k, v in d.items()} for t, d in params.items()}
    y = render_grafx(hip, x.cuda(), pg, rd)[0]
    with torch.no_grad():
        y_inference = render_grafx(hip, x.cuda(), {t: {k: v.detach() for k, v in d.items()} for t, d in pg.items()}, rd)[0]
    what = f"{kind}, {'per-row' if per_row else 'batch-shared'} parameters"
    assert_close(y.detach().cpu().double().reshape(y64.shape), y64, 1e-5, f"{what}: output")
    leaves = [v for d in pg.values() for v in d.values()]
    got = torch.autograd.grad((y.reshape(w.shape) * w.cuda()).sum(), leaves)
    names = [f"{t}.{k}" for t, d in pg.items() for k in d]
    for name, a, b in zip(names, got, want):
        assert_close(a.cpu().double(), b, 1e-5, f"{what}: gradient of {name}")
    assert native_rows == [B if per_row else 1], native_rows    # one reverb node: one call, over its parameter rows
    # the forward under gradients is the inference kernel
    assert torch.equal(y.detach(), y_inference), f"{what}: {(y.detach() - y_inference).abs().max().item():.3e}"
