"""FilteredNoiseShapingReverb under gradients: the taps come from the native node autograd.NoiseShapingIrFn (inference kernel
forward, gfx_noise_shaping_ir_bwd_f32 backward) -- in compute_ir un-normalised, in forward normalised; every channel mode,
with and without fade-in, both noise_randomness values, a two-block stream and a graph rendered by render_grafx.  Gradients
against the reference's arrays (g19) or float64 autograd of the formula on the CPU (noise_shaping_float64.py: taps,
normalize_impulse, mid/side and the reference's FFT convolution in double), at the project's 1e-5 of each gradient's own
peak.  With 600 taps L = 1024 makes L + N - 1 odd (the reference's aliased convolution), L = 1023 makes it even (linear)."""
import pytest
import torch

from conftest import assert_close, assert_parity
from noise_shaping_float64 import reverb64, taps64

pytestmark = pytest.mark.gpu

R, IR_LEN, BANDS = 2, 600, 3
NODE = "NoiseShapingIrFnBackward"


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


def _module(channel="midside", fade=False, randomness="fixed", ir_len=IR_LEN, bands=BANDS):
    from grafx_amd.processors import FilteredNoiseShapingReverb

    return FilteredNoiseShapingReverb(ir_len=ir_len, num_bands=bands, processor_channel=channel, noise_randomness=randomness,
                                      use_fade_in=fade, flashfftconv=False).cuda()


def _inputs(m, seed, length, rows=R):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, m.num_channels, length, generator=gen)
    p = {k: torch.randn(rows, *shape, generator=gen) for k, shape in m.parameter_size().items()}
    w = torch.randn(rows, m.num_channels, length, generator=gen)
    return x, p, w


def _leaves(p):
    return {k: v.cuda().requires_grad_() for k, v in p.items()}


# ------------------------------------------------------------------------------------------------ the reference's arrays
def test_g19_case_trains_on_the_native_node(golden):
    import grafx_amd.processors as P
    from test_gpu_training_paths import G19, _call, _graph_nodes, _module as g19_module, _specs

    g = golden(G19)
    tag = "FilteredNoiseShapingReverb_midside_fade"
    spec = _specs(g)[tag]
    m = g19_module(P, spec["cls"], spec["kwargs"], spec["inner"]).cuda()
    assert m.filtered_noise.shape == g[f"{tag}_noise"].shape
    with torch.no_grad():
        m.filtered_noise.copy_(g[f"{tag}_noise"])
    x = g[spec["x"]].cuda().requires_grad_()
    p = {k: g[f"{tag}_p_{k}"].cuda().requires_grad_() for k in spec["leaves"]}
    y = _call(m, x, p)
    nodes = _graph_nodes(y)
    for name in (NODE, "LinearConvFnBackward", "OddAliasFnBackward"):
        assert name in nodes, sorted(nodes)
    grads = torch.autograd.grad((y * g[spec["w"]].cuda()).sum(), [x, *p.values()])
    assert_parity(y.detach().cpu(), g[f"{tag}_y32"], g[f"{tag}_y64"], 1e-5, f"{tag} y")
    for k, got in zip(["x", *p], grads):
        assert_parity(got.cpu(), g[f"{tag}_g32_{k}"], g[f"{tag}_g64_{k}"], 1e-5, f"{tag} grad {k}")


# ------------------------------------------------------------------------------------------------ against float64
def _reference64(m, x, p, w, exact=False):
    x64 = x.double().requires_grad_()
    p64 = {k: v.double().requires_grad_() for k, v in p.items()}
    y64 = reverb64(x64, m.filtered_noise[0], p64["log_decay"], p64["log_gain"], p64.get("log_fade_in"),
                   p64.get("z_fade_in_gain"), m.min_decay, m.max_decay, m.processor_channel, exact)
    return y64.detach(), torch.autograd.grad(y64, [x64, *p64.values()], w.double())


@pytest.mark.parametrize("length", [1024, 1023], ids=["aliased", "linear"])
@pytest.mark.parametrize("fade", [False, True], ids=["no_fade", "fade"])
@pytest.mark.parametrize("channel", ["mono", "stereo", "midside"])
def test_module_gradients(channel, fade, length):
    m = _module(channel, fade)
    x, p, w = _inputs(m, 1 + fade + 2 * length, length)
    xg, pg = x.cuda().requires_grad_(), _leaves(p)
    y = m(xg, **pg)
    assert NODE in _nodes(y), sorted(_nodes(y))
    got = torch.autograd.grad(y, [xg, *pg.values()], w.cuda())
    y64, want = _reference64(m, x, p, w)
    what = f"{channel}, fade {fade}, L {length}"
    assert_close(y.detach().cpu().double(), y64, 1e-5, f"{what}: output")
    for name, a, b in zip(["input", *p], got, want):
        assert_close(a.cpu().double(), b, 1e-5, f"{what}: gradient of {name}")


@pytest.mark.parametrize("fade", [False, True], ids=["no_fade", "fade"])
def test_the_model_trains_on_the_taps_it_serves(fade):
    m = _module("midside", fade)
    _, p, _ = _inputs(m, 5, 8)
    pg = _leaves(p)
    args = [pg["log_decay"], pg["log_gain"], pg.get("log_fade_in"), pg.get("z_fade_in_gain")]
    taps = m._taps(*args, True)
    ir = m.compute_ir(**pg)
    assert NODE in _nodes(taps) and NODE in _nodes(ir)
    with torch.no_grad():
        assert torch.equal(taps.detach(), m._taps(*args, True))
        assert torch.equal(ir.detach(), m.compute_ir(**pg))
    # compute_ir is un-normalised; its gradient against float64
    gh = torch.randn(R, 2, IR_LEN, generator=torch.Generator().manual_seed(6))
    got = torch.autograd.grad(ir, list(pg.values()), gh.cuda())
    p64 = {k: v.double().requires_grad_() for k, v in p.items()}
    ir64 = taps64(m.filtered_noise[0], p64["log_decay"], p64["log_gain"], p64.get("log_fade_in"), p64.get("z_fade_in_gain"),
                  m.min_decay, m.max_decay, False)
    assert_close(ir.detach().cpu().double(), ir64.detach(), 1e-5, "compute_ir")
    for name, a, b in zip(p, got, torch.autograd.grad(ir64, list(p64.values()), gh.double())):
        assert_close(a.cpu().double(), b, 1e-5, f"compute_ir: gradient of {name}")
    # the formula kept as torch ops is the same function
    with torch.no_grad():
        assert_close(m.torch_compute_ir(**pg).cpu(), ir.detach().cpu(), 1e-5, "torch_compute_ir")


def test_pseudo_random_backward_sees_the_window_of_its_forward():
    """Seeded alike, two calls cut the same window and give the same gradients: those of a "fixed" module whose buffer is that
    window -- also when another call has cut another window between the forward and its backward."""
    a, b = _module("stereo", True, "pseudo-random"), _module("stereo", True)
    assert a.filtered_noise.shape[-1] == 5 * IR_LEN
    torch.manual_seed(12)
    start = int(torch.randint(0, 4 * IR_LEN, (1,)))
    with torch.no_grad():
        b.filtered_noise.copy_(a.filtered_noise[..., start:start + IR_LEN])
    x, p, w = _inputs(a, 13, 1023)

    def run(m, seed, disturb=False):
        xg, pg = x.cuda().requires_grad_(), _leaves(p)
        torch.manual_seed(seed)
        y = m(xg, **pg)
        if disturb:
            torch.manual_seed(seed + 1)
            assert not torch.equal(m(xg, **pg).detach(), y.detach())
        return y.detach(), torch.autograd.grad(y, [xg, *pg.values()], w.cuda())

    y_fixed, want = run(b, 0)
    for disturb in (False, True):
        y, got = run(a, 12, disturb)
        assert torch.equal(y, y_fixed)
        for name, g1, g2 in zip(["input", *p], got, want):
            assert torch.equal(g1, g2), name


def test_two_block_stream_gradients():
    """forward(state=, return_state=True) under gradients: the parameter gradients of two blocks sum to the one-call
    gradients (the linear convolution of the whole: set_exact_convolution(True))."""
    from grafx_amd.processors.core.convolution import exact_convolution_scope

    m = _module("midside", True)
    L1, L2 = 513, 510
    x, p, w = _inputs(m, 7, L1 + L2)
    xc, wc = x.cuda(), w.cuda()
    with exact_convolution_scope(True):
        pg = _leaves(p)
        y = m(xc, **pg)
        want = torch.autograd.grad(y, list(pg.values()), wc)
        pg = _leaves(p)
        y1, s1 = m(xc[..., :L1], **pg, return_state=True)
        y2, s2 = m(xc[..., L1:], **pg, state=s1, return_state=True)
        assert NODE in _nodes(y1) and NODE in _nodes(y2)
        g1 = torch.autograd.grad(y1, list(pg.values()), wc[..., :L1])
        g2 = torch.autograd.grad(y2, list(pg.values()), wc[..., L1:])
    assert tuple(s2.shape) == (R, 2, IR_LEN - 1)
    assert_close(torch.cat([y1, y2], -1).detach().cpu(), y.detach().cpu(), 1e-5, "stream: output")
    for name, a, b, c in zip(p, g1, g2, want):
        assert_close((a + b).cpu(), c.cpu(), 1e-5, f"stream: gradient of {name}")
    y64, want64 = _reference64(m, x, p, w, exact=True)
    for name, a, b, c in zip(p, g1, g2, want64[1:]):
        assert_close((a + b).cpu().double(), c, 1e-5, f"stream: gradient of {name} against float64")


def test_training_through_render_grafx(monkeypatch):
    """in -> reverb -> out at batch 2: the render's parameter gradients are the direct module call's.  The render's backward
    hides its stages behind one node of its own: that the taps are differentiated by the native kernel is seen at the
    wrapper the node calls."""
    from grafx_amd import ops
    from grafx_amd.data import GRAFX, NodeConfigs, convert_to_tensor
    from grafx_amd.render import prepare_render, render_grafx, reorder_for_fast_render
    from grafx_amd.utils import create_empty_parameters

    calls, native = [], ops.noise_shaping_ir_bwd

    def counted(grad_ir, *args, **kw):
        calls.append(grad_ir.shape[0])
        return native(grad_ir, *args, **kw)

    monkeypatch.setattr(ops, "noise_shaping_ir_bwd", counted)
    B, L = 2, 1024
    G = GRAFX(config=NodeConfigs(["reverb"]))
    G.add_serial_chain(["in", "reverb", "out"])
    m = _module("midside", True)
    hip = {"reverb": m}
    torch.manual_seed(21)
    tree = create_empty_parameters(hip, G, std=0.3)
    params = {k: v.detach().clone() for k, v in tree["reverb"].items()}
    x, w = 0.3 * torch.randn(B, 1, 2, L), torch.randn(B, 1, 2, L)
    rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam")).to("cuda")
    pg = _leaves(params)
    y = render_grafx(hip, x.cuda(), {"reverb": pg}, rd)[0]
    got = torch.autograd.grad((y.reshape(w.shape) * w.cuda()).sum(), list(pg.values()))
    assert len(calls) == 1, calls
    direct = _leaves(params)
    yd = m(x.cuda()[:, 0], **{k: v.repeat(B, 1, 1) for k, v in direct.items()})
    assert NODE in _nodes(yd)
    want = torch.autograd.grad((yd * w.cuda()[:, 0]).sum(), list(direct.values()))
    assert_close(y.detach().cpu().reshape(yd.shape), yd.detach().cpu(), 1e-5, "render: output")
    for name, a, b in zip(params, got, want):
        assert_close(a.cpu(), b.cpu(), 1e-5, f"render: gradient of {name}")


def test_the_tape_holds_no_envelope_tensor():
    """compute_ir(...).backward(g) at R = 8, C = 2, K = 8, ir_len = 4096 raises the peak of allocated memory by less than one
    (R, C, K, ir_len) float32 tensor (2 MiB): the chain of torch ops held several, the node holds (R, C, ir_len) ones."""
    Rm, C, K, T = 8, 2, 8, 4096
    m = _module("stereo", True, ir_len=T, bands=K)
    gen = torch.Generator().manual_seed(3)
    p = _leaves({k: torch.randn(Rm, *shape, generator=gen) for k, shape in m.parameter_size().items()})
    g = torch.randn(Rm, C, T, generator=gen).cuda()
    m.compute_ir(**p).backward(g)          # warm-up: the library, the allocator's pools
    for v in p.values():
        v.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ir = m.compute_ir(**p)
    assert NODE in _nodes(ir)
    ir.backward(g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise over compute_ir + backward: {rise} bytes; one envelope tensor: {Rm * C * K * T * 4}")
    assert all(v.grad is not None for v in p.values())
    assert rise < Rm * C * K * T * 4, rise
