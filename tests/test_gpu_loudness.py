"""The loudness meter on the GPU against its float64 definition (tests/loudness_float64.py): the sub-block energies and their
gradient at the shapes where the kernels can go wrong, the module end to end, the normaliser, the guarantees on bits,
memory and layouts, and the refusals of the ops wrappers."""
import math

import pytest
import torch
from conftest import assert_close, assert_close_rows

import loudness_float64 as f64

pytestmark = pytest.mark.gpu
TOL = 1e-5
LU = 1e-4            # 10 log10(1 + 2e-5) rounded up: what an error of 1e-5 in the energies can cost
PATTERNS = ("ones", "random", "runs")


def ident(shape):
    return "{}/{}/{}".format(*shape[:3])


# ------------------------------------------------------------------------------------------------ 1: the energies
@pytest.mark.parametrize("kind", f64.KINDS)
@pytest.mark.parametrize("shape", f64.SHAPES, ids=ident)
def test_energies_match_float64(shape, kind):
    from grafx_amd import ops

    hop, L, C, fs = shape
    got = ops.kweight_energy(f64.signal(*shape, kind).cuda(), f64.coef(fs), hop)
    want = f64.energies(*shape, kind)
    assert got.shape == (f64.ROWS, C, L // hop) and got.dtype == torch.float64
    assert_close_rows(got, want, TOL, f"energies {ident(shape)} {kind}")      # every row-channel against its own peak block


def test_energies_of_a_strided_slice_of_a_render_buffer():
    from grafx_amd import ops

    hop, L, C, fs = f64.STRIDED
    x = f64.signal(*f64.STRIDED, "bass", rows=4)
    buf = torch.randn(2, 4, C, L + 8, device="cuda")
    view = buf[:, 1:3, :, 4:L + 4]                      # (B, n, C, L) inside a larger buffer: batch and rows with strides of their own
    view.copy_(x.view(2, 2, C, L))
    got = ops.kweight_energy(view, f64.coef(fs), hop)
    assert_close_rows(got, f64.energies(*f64.STRIDED, "bass", rows=4), TOL, "energies of a strided view")
    assert torch.equal(got, ops.kweight_energy(x.cuda(), f64.coef(fs), hop))         # the vector loads change no bit


def test_many_row_channels():
    """66000 row-channels: beyond what a second grid dimension takes.  Row-dependent data; the energies of every row and
    the gradient of the rows at either end and around 65536 against float64."""
    from grafx_amd import ops

    hop, L, C, fs = f64.MANY
    x = f64.signal(*f64.MANY, "noise", rows=66000)
    xg = x.cuda()
    got = ops.kweight_energy(xg, f64.coef(fs), hop)
    assert_close_rows(got, f64.energies(*f64.MANY, "noise", rows=66000), TOL, "energies of 66000 rows")
    c = f64.cotangent(*f64.MANY, "random", rows=66000)
    grad = ops.kweight_energy_bwd(xg, f64.coef(fs), c.cuda(), hop)
    rows = torch.cat([torch.arange(0, 70), torch.arange(65500, 65610), torch.arange(65930, 66000)])
    assert_close_rows(grad[rows.cuda()], f64.energy_grad_of(x[rows], fs, hop, c[rows]), TOL, "gradient among 66000 rows")
    assert torch.equal(grad[rows.cuda()], ops.kweight_energy_bwd(xg[rows.cuda()], f64.coef(fs), c[rows].cuda(), hop))
    two = ops.kweight_energy(xg.view(33000, 2, L), f64.coef(fs), hop)                 # the same rows as stereo pairs
    assert torch.equal(two.view(66000, 1, -1), got)


# ------------------------------------------------------------------------------------------------ 2: the gradient
@pytest.mark.parametrize("pattern,kind", list(zip(PATTERNS, f64.KINDS)))
@pytest.mark.parametrize("shape", f64.SHAPES, ids=ident)
def test_gradient_matches_float64(shape, pattern, kind):
    from grafx_amd import ops

    hop, L, C, fs = shape
    x = f64.signal(*shape, kind).cuda()
    got = ops.kweight_energy_bwd(x, f64.coef(fs), f64.cotangent(*shape, pattern).cuda(), hop)
    want = f64.energy_grad(*shape, kind, pattern)
    assert got.shape == x.shape and got.dtype == torch.float32
    assert_close_rows(got, want, TOL, f"gradient {ident(shape)} {kind} {pattern}")
    tail = (L // hop) * hop
    assert torch.count_nonzero(got[..., tail:]) == 0 and torch.count_nonzero(want[..., tail:]) == 0   # exactly 0.0


def test_gradient_accumulates_and_writes_a_strided_out_in_place():
    from grafx_amd import ops

    shape = f64.SHAPES[4]                                  # 800 / 16037 / 2
    hop, L, C, fs = shape
    x, c = f64.signal(*shape, "bass").cuda(), f64.cotangent(*shape, "random").cuda()
    want = f64.energy_grad(*shape, "bass", "random")
    plain = ops.kweight_energy_bwd(x, f64.coef(fs), c, hop)
    buf = torch.randn(f64.ROWS, 3, C, L + 3, device="cuda")
    before = buf.clone()
    out = buf[:, 1:2, :, 3:]                               # (B, 1, C, L) inside a larger buffer, rows off the 16-byte grid
    assert ops.kweight_energy_bwd(x, f64.coef(fs), c, hop, out=out) is out
    assert torch.equal(out.reshape(plain.shape), plain)
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:, 1:2, :, 3:] = False
    assert torch.equal(buf[keep], before[keep])            # nothing beside the view is written
    start = torch.randn_like(plain)
    acc = start.clone()
    ops.kweight_energy_bwd(x, f64.coef(fs), c, hop, out=acc, accumulate=True)
    assert_close_rows(acc - start, want, TOL, "accumulated gradient")
    assert torch.equal(acc, start + plain)
    with pytest.raises(ValueError, match="accumulate"):
        ops.kweight_energy_bwd(x, f64.coef(fs), c, hop, accumulate=True)


# ------------------------------------------------------------------------------------------------ 3: the module
def graph_nodes(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo += [nxt for nxt, _ in fn.next_functions]
    return {type(fn).__name__ for fn in seen}


@pytest.mark.parametrize("fs", f64.GATING_RATES)
def test_module_matches_float64_on_the_gating_signal(fs):
    from grafx_amd.loudness import IntegratedLoudness

    case = f64.gating_case(fs)
    meter = IntegratedLoudness(fs)
    x = case["x"].cuda().unsqueeze(0).requires_grad_(True)          # (1, 2, L)
    got = meter(x)
    print(f"{fs} Hz: {float(got.detach()):.6f} LUFS, float64 {float(case['loudness']):.6f}")
    assert got.shape == (1,) and got.dtype == torch.float32
    assert abs(float(got.detach()) - float(case["loudness"])) <= LU
    nodes = graph_nodes(got)
    assert "KWeightEnergyFnBackward" in nodes and not [n for n in nodes if "Biquad" in n or "Cascade" in n], nodes
    got.sum().backward()
    assert_close(x.grad[0], case["dx"], TOL, f"input gradient at {fs} Hz")
    blocks = meter.block_loudness(x.detach())
    assert blocks.shape == (1, 37)
    assert (blocks[0].double().cpu() - case["blocks"]).abs().max() <= LU
    # two-dimensional input and leading dimensions beyond the row map's two
    assert abs(float(meter(x.detach()[0])) - float(case["loudness"])) <= LU
    many = meter(x.detach().expand(2, 1, 3, 1, *x.shape[-2:]))
    assert many.shape == (2, 1, 3, 1) and bool((many == got.detach()).all())


# ------------------------------------------------------------------------------------------------ 4: the normaliser
@pytest.mark.parametrize("detach_gain", [False, True])
def test_normalize_lands_on_the_target(detach_gain):
    from grafx_amd.loudness import IntegratedLoudness, loudness_normalize

    fs, target = 8000, -23.0
    meter = IntegratedLoudness(fs)
    loud = f64.gating_case(fs)["x"]
    x = torch.stack([loud, torch.zeros_like(loud), 0.25 * f64.gating_case(fs, seed=2)["x"]]).cuda().requires_grad_(True)
    y = loudness_normalize(x, target, meter, detach_gain=detach_gain)
    level = meter(y.detach())
    assert abs(float(level[0]) - target) <= LU and abs(float(level[2]) - target) <= LU
    assert level[1] == -math.inf and torch.equal(y[1], x[1])         # a silent item comes back unchanged
    y.square().sum().backward()
    assert torch.isfinite(x.grad).all() and torch.count_nonzero(x.grad[0]) > 0 and torch.count_nonzero(x.grad[1]) == 0


# ------------------------------------------------------------------------------------------------ 5: guarantees
def test_equal_bits_from_call_to_call_and_for_a_row_computed_alone():
    from grafx_amd import ops

    for shape in (f64.SHAPES[2], f64.SHAPES[5], f64.SHAPES[6]):       # LDS sums, wave sums, a finishing wave of 69 parts
        hop, L, C, fs = shape
        x, c = f64.signal(*shape, "bass").cuda(), f64.cotangent(*shape, "random").cuda()
        e1, e2 = ops.kweight_energy(x, f64.coef(fs), hop), ops.kweight_energy(x, f64.coef(fs), hop)
        g1, g2 = ops.kweight_energy_bwd(x, f64.coef(fs), c, hop), ops.kweight_energy_bwd(x, f64.coef(fs), c, hop)
        assert torch.equal(e1, e2) and torch.equal(g1, g2)
        ws = torch.full((ops.kweight_energy_ws_bytes(f64.ROWS, C, L) + 64,), 0xff, dtype=torch.uint8, device="cuda")
        assert torch.equal(ops.kweight_energy(x, f64.coef(fs), hop, ws=ws), e1)        # a reused workspace of any content
        assert torch.equal(ops.kweight_energy_bwd(x, f64.coef(fs), c, hop, ws=ws), g1)
        for r in range(f64.ROWS):
            assert torch.equal(ops.kweight_energy(x[r:r + 1], f64.coef(fs), hop), e1[r:r + 1])
            assert torch.equal(ops.kweight_energy_bwd(x[r:r + 1], f64.coef(fs), c[r:r + 1], hop), g1[r:r + 1])


def test_forward_and_backward_hold_no_second_signal():
    """Forward + backward at (8, 2, 262144) raise the peak allocation by at most 1.1 x bytes(x) + 1 MiB: the gradient and
    the per-tile states, no filtered signal."""
    from grafx_amd.loudness import IntegratedLoudness

    meter = IntegratedLoudness(48000)
    x = torch.randn(8, 2, 262144, device="cuda").requires_grad_(True)
    nbytes = x.numel() * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    meter(x).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise {rise} bytes = {rise / nbytes:.3f} x bytes(x)")
    assert rise <= 1.1 * nbytes + (1 << 20)
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_a_registered_grad_sink_receives_the_gradient():
    from grafx_amd import autograd as diff
    from grafx_amd import ops

    shape = f64.SHAPES[3]
    hop, L, C, fs = shape
    buf = torch.zeros(f64.ROWS, 2, C, L, device="cuda")
    x = f64.signal(*shape, "noise").cuda().requires_grad_(True)
    c = f64.cotangent(*shape, "random").cuda()
    dest = buf[:, 1]
    with diff.grad_sink(x, dest) as sink:
        e = diff.KWeightEnergyFn.apply(x, f64.coef(fs), hop)
        (g,) = torch.autograd.grad((e * c).sum(), x)
        assert sink.writes == 1
    assert g.data_ptr() == dest.data_ptr() and torch.equal(dest, ops.kweight_energy_bwd(x.detach(), f64.coef(fs), c, hop))
    assert torch.count_nonzero(buf[:, 0]) == 0


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_ops_refuse_bad_arguments():
    from grafx_amd import ops

    coef = f64.coef(48000)
    x = torch.randn(2, 2, 1000, device="cuda")
    c = torch.ones(2, 2, 10, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.kweight_energy(x.cpu(), coef, 100)
    with pytest.raises(TypeError, match="float32"):
        ops.kweight_energy(x.double(), coef, 100)
    for hop in (0, 1001, -3, 100.0):
        with pytest.raises(ValueError, match="hop"):
            ops.kweight_energy(x, coef, hop)
        with pytest.raises(ValueError, match="hop"):
            ops.kweight_energy_bwd(x, coef, c, hop)
    for bad in (coef[0], coef.reshape(5, 2), torch.ones(2, 6, dtype=torch.float64), [1.0] * 10):
        with pytest.raises(ValueError, match="coef"):
            ops.kweight_energy(x, bad, 100)
    with pytest.raises(ValueError, match="coef"):
        ops.kweight_energy(x, coef.cuda(), 100)
    with pytest.raises(ValueError, match="finite"):
        ops.kweight_energy(x, torch.where(coef == coef[1, 4], math.nan, coef), 100)
    with pytest.raises(TypeError, match="genergy"):
        ops.kweight_energy_bwd(x, coef, c.float(), 100)
    with pytest.raises(ValueError, match="genergy"):
        ops.kweight_energy_bwd(x, coef, c[..., :9], 100)
    with pytest.raises(ValueError, match="out"):
        ops.kweight_energy_bwd(x, coef, c, 100, out=torch.empty(2, 2, 999, device="cuda"))
    with pytest.raises(ValueError, match="share memory"):
        ops.kweight_energy_bwd(x, coef, c, 100, out=x)
    nbytes = ops.kweight_energy_ws_bytes(2, 2, 1000)
    with pytest.raises(ValueError, match="workspace"):
        ops.kweight_energy(x, coef, 100, ws=torch.empty(nbytes - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="workspace"):
        ops.kweight_energy(x, coef, 100, ws=torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")[8:])
    with pytest.raises(ValueError, match="share memory"):
        ops.kweight_energy(x, coef, 100, ws=x.view(torch.uint8).view(-1))
    with pytest.raises(ValueError, match="share memory"):
        ops.kweight_energy_bwd(x, coef, c, 100, ws=c.view(torch.uint8).view(-1))
    buf = torch.empty(nbytes + 4 * x.numel(), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="share memory"):
        ops.kweight_energy_bwd(x, coef, c, 100, out=buf[:4 * x.numel()].view(torch.float32).view(x.shape), ws=buf[16:])
