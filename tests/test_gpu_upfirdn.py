"""The polyphase FIR on the GPU against its float64 definition (tests/upfirdn_float64.py): the forward at the smallest shapes
that break a wrong kernel, layouts, the guarantees on bits, many rows, a row whose indices pass 2^31, the adjoint, the
refusals of the ops wrapper, and the Resample module.  Ratios are written orig/new = down/up, as the filter design takes them."""
import functools
import math

import numpy as np
import pytest
import torch
from conftest import assert_close_rows

import upfirdn_float64 as f64

pytestmark = pytest.mark.gpu
TOL = 1e-5
C = 2


def design(orig, new):
    h, up, down, offset = f64.sinc_kernel(orig, new)
    return f64.taps32(h), up, down, offset


# name -> ((taps as float64 of their float32 values, float32 tensor), up, down, offset, L)
@functools.lru_cache(maxsize=None)
def geometry(name):
    if name == "identity":
        return f64.taps32([1.0]), 1, 1, 0, 777
    if name in ("4/1 causal", "4/1 anticausal"):
        taps, up, down, _ = design(4, 1)
        return taps, up, down, 0 if name == "4/1 causal" else len(taps[0]) - 1, 1000
    orig, new, L = {"1/4": (1, 4, 5), "2/1": (2, 1, 101), "3/2": (3, 2, 333), "147/160": (147, 160, 700),
                    "441/160": (441, 160, 3000)}[name]
    return (*design(orig, new), L)


CASES = ("identity", "1/4", "2/1", "3/2", "147/160", "441/160", "4/1 causal", "4/1 anticausal")
TAPS = {"identity": 1, "1/4": 49, "2/1": 25, "3/2": 37, "147/160": 1939, "441/160": 5345, "4/1 causal": 49, "4/1 anticausal": 49}


@functools.lru_cache(maxsize=None)
def case(name, kind, L=None, n_out=None):
    """-> (x float32 on the CPU, taps float32 on the CPU, up, down, offset, the float64 result); computed once, never written."""
    (h64, h32), up, down, offset, L0 = geometry(name)
    x64, x32 = f64.KINDS[kind]((f64.ROWS, C, L0 if L is None else L), seed=len(name) + 7 * (L or 0))
    return x32, h32, up, down, offset, torch.from_numpy(f64.upfirdn(x64, h64, up, down, offset, n_out))


# ------------------------------------------------------------------------------------------------ 1: forward
@pytest.mark.parametrize("kind", sorted(f64.KINDS))
@pytest.mark.parametrize("name", CASES)
def test_forward_matches_float64(name, kind):
    from grafx_amd import ops

    x, h, up, down, offset, want = case(name, kind)
    assert h.numel() == TAPS[name]
    got = ops.upfirdn(x.cuda(), h.cuda(), up, down, offset)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert got.shape[-1] == -(-(x.shape[-1] * up + h.numel() - 1 - offset) // down)
    assert_close_rows(got, want, TOL, f"upfirdn {name} {kind}")
    if name == "identity":
        assert torch.equal(got.cpu(), x)                     # the bits of x


@pytest.mark.parametrize("name,L", [("1/4", 523), ("2/1", 4128)])
@pytest.mark.parametrize("tiles,extra", [(1, -1), (1, 0), (1, 1), (2, 1)])
def test_output_lengths_around_the_tile(name, L, tiles, extra):
    from grafx_amd import ops

    M = tiles * ops.UPFIRDN_TILE + extra
    x, h, up, down, offset, want = case(name, "tone", L, M)
    assert M <= f64.default_n_out(L, h.numel(), up, down, offset)          # every output has taps under it
    got = ops.upfirdn(x.cuda(), h.cuda(), up, down, offset, n_out=M)
    assert got.shape == (f64.ROWS, C, M)
    assert_close_rows(got, want, TOL, f"upfirdn {name} M={M}")


def test_outputs_beyond_the_signal_are_exactly_zero():
    from grafx_amd import ops

    x, h, up, down, offset, _ = case("147/160", "noise")
    live = f64.default_n_out(x.shape[-1], h.numel(), up, down, offset)
    M = live + 2 * ops.UPFIRDN_TILE + 300                                    # a partly dead tile, then wholly dead ones
    want = case("147/160", "noise", None, M)[-1]
    got = ops.upfirdn(x.cuda(), h.cuda(), up, down, offset, n_out=M)
    assert_close_rows(got, want, TOL, "upfirdn beyond the signal")
    assert torch.count_nonzero(got[..., live:]) == 0 and torch.count_nonzero(want[..., live:]) == 0
    assert torch.count_nonzero(got[..., live - 8:live]) > 0


@pytest.mark.parametrize("up,down,N,offset,L", [(3, 1000, 50, 49, 200000), (1024, 1024, 16384, 16383, 100), (1, 1, 16384, 5, 40),
                                                (4, 1, 1, 0, 300), (4, 3, 3, 2, 500), (1024, 7, 5, 4, 9), (257, 255, 600, 0, 700)])
def test_the_ends_of_the_supported_range(up, down, N, offset, L):
    """The largest ratios and tap counts: a tile taken in passes of 16 outputs (down / up = 333), the taps beyond 64 KiB of
    LDS, and passes of one output under 16384 taps; fewer taps than phases, so that some outputs have no tap at all; a ratio
    above the 256 lanes.  Noise taps; at most 40 non-zero products per output, as in the other cases."""
    from grafx_amd import ops

    h64, h32 = f64.taps32(f64.noise((N,), seed=N)[0])
    x64, x32 = f64.noise((f64.ROWS, 1, L), seed=L)
    got = ops.upfirdn(x32.cuda(), h32.cuda(), up, down, offset)
    assert_close_rows(got, torch.from_numpy(f64.upfirdn(x64, h64, up, down, offset)), TOL, f"upfirdn {up}/{down}, {N} taps")


# ------------------------------------------------------------------------------------------------ 2: layouts
def test_strided_views_accumulate_and_aliasing():
    from grafx_amd import ops

    x, h, up, down, offset, want = case("3/2", "tone")
    L, M = x.shape[-1], want.shape[-1]
    xg, hg = x.cuda(), h.cuda()
    plain = ops.upfirdn(xg, hg, up, down, offset)
    src = torch.randn(1, 4, C, L + 8, device="cuda")
    view = src[:, 1:3, :, 3:L + 3]                           # (B, n, C, L) inside a larger buffer, rows off the 16-byte grid
    view.copy_(xg.view(1, 2, C, L))
    assert view.data_ptr() % 16 != 0
    buf = torch.randn(1, 3, C, M + 5, device="cuda")
    before = buf.clone()
    out = buf[:, 0:2, :, 1:M + 1]
    assert ops.upfirdn(view, hg, up, down, offset, out=out) is out
    assert torch.equal(out.reshape(plain.shape), plain)      # the bits of the contiguous call
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:, 0:2, :, 1:M + 1] = False
    assert torch.equal(buf[keep], before[keep])              # nothing beside the view is written
    start = torch.randn_like(plain)
    acc = start.clone()
    ops.upfirdn(xg, hg, up, down, offset, out=acc, accumulate=True)
    assert torch.equal(acc, start + plain)
    with pytest.raises(ValueError, match="accumulate"):
        ops.upfirdn(xg, hg, up, down, offset, accumulate=True)
    # an out that overlaps x or h is refused before any launch
    both = torch.zeros(f64.ROWS, C, L + M, device="cuda")
    with pytest.raises(ValueError, match="share memory"):
        ops.upfirdn(both[..., :L], hg, up, down, offset, out=both[..., L - 1:L - 1 + M])
    flat = torch.zeros(f64.ROWS * C * M + h.numel(), device="cuda")
    with pytest.raises(ValueError, match="share memory"):
        ops.upfirdn(xg, flat[-h.numel() - 1:-1], up, down, offset, out=flat[:f64.ROWS * C * M].view(f64.ROWS, C, M))
    assert torch.count_nonzero(both) == 0 and torch.count_nonzero(flat) == 0
    with pytest.raises(ValueError, match="out"):
        ops.upfirdn(xg, hg, up, down, offset, out=torch.empty(f64.ROWS, C, M - 1, device="cuda"))


# ------------------------------------------------------------------------------------------------ 3: guarantees on bits
@pytest.mark.parametrize("name", ["147/160", "2/1"])
def test_equal_bits_from_call_to_call_and_for_a_row_computed_alone(name):
    from grafx_amd import ops

    x, h, up, down, offset, _ = case(name, "noise")
    xg, hg = x.cuda(), h.cuda()
    y1, y2 = ops.upfirdn(xg, hg, up, down, offset), ops.upfirdn(xg, hg, up, down, offset)
    assert torch.equal(y1, y2)
    for r in range(f64.ROWS):
        assert torch.equal(ops.upfirdn(xg[r:r + 1], hg, up, down, offset), y1[r:r + 1])
    assert torch.equal(ops.upfirdn(xg[:, 1:], hg, up, down, offset), y1[:, 1:])


def test_many_row_channels():
    """66000 row-channels, beyond what a second grid dimension takes: the rows at either end and around 65536."""
    from grafx_amd import ops

    (h64, h32), up, down, offset, _ = geometry("1/4")
    x64, x32 = f64.noise((66000, 1, 64), seed=11)
    got = ops.upfirdn(x32.cuda(), h32.cuda(), up, down, offset)
    rows = torch.cat([torch.arange(0, 70), torch.arange(65500, 65610), torch.arange(65930, 66000)])
    want = torch.from_numpy(f64.upfirdn(x64[rows.numpy()], h64, up, down, offset))
    assert_close_rows(got[rows.cuda()], want, TOL, "upfirdn among 66000 rows")
    two = ops.upfirdn(x32.cuda().view(33000, 2, 64), h32.cuda(), up, down, offset)      # the same rows as stereo pairs
    assert torch.equal(two.view(66000, 1, -1), got)


def test_a_long_row_whose_indices_pass_2_to_the_31():
    """One row of 14 000 000 samples, 147/160: m down of the last tile is 2.24e9.  The last 4096 outputs against the direct
    float64 sum over those outputs only."""
    from grafx_amd import ops

    (h64, h32), up, down, offset, _ = geometry("147/160")
    L = 14_000_000
    x32 = torch.randn(1, 1, L, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    M = -(-L * up // down)
    assert (M - 1) * down > 2 ** 31
    got = ops.upfirdn(x32.cuda(), h32.cuda(), up, down, offset, n_out=M)
    assert got.shape == (1, 1, M)
    ms = range(M - 4096, M)
    tail = x32[..., L - 8192:].double().numpy()              # every sample those outputs reach, and the end of the signal
    shift = (L - 8192) * up                                  # m down + offset - k up with k counted from L - 8192
    assert (M - 4096) * down + offset - (len(h64) - 1) >= shift
    want = f64.upfirdn_direct(tail, h64, up, down, offset - shift, ms)
    assert_close_rows(got[..., M - 4096:], torch.from_numpy(want), TOL, "the last 4096 outputs of a 14 M row")


# ------------------------------------------------------------------------------------------------ 4: the adjoint
@pytest.mark.parametrize("name", ["1/4", "2/1", "3/2", "147/160", "441/160"])
def test_backward_is_the_float64_adjoint(name):
    from grafx_amd import autograd as diff

    x, h, up, down, offset, want = case(name, "noise")
    (h64, _), *_ = geometry(name)
    g64, g32 = f64.noise(tuple(want.shape), seed=3)
    xg = x.cuda().requires_grad_(True)
    y = diff.UpfirdnFn.apply(xg, h.cuda(), up, down, offset, want.shape[-1])
    assert_close_rows(y.detach(), want, TOL, f"UpfirdnFn forward {name}")
    (grad,) = torch.autograd.grad(y, xg, g32.cuda())
    assert grad.shape == x.shape and grad.dtype == torch.float32
    assert_close_rows(grad, torch.from_numpy(f64.adjoint(g64, h64, up, down, offset, x.shape[-1])), TOL, f"adjoint {name}")
    lhs = float((y.detach().double().cpu() * torch.from_numpy(g64)).sum())
    rhs = float((x.double() * grad.double().cpu()).sum())
    scale = float((y.detach().double().cpu() * torch.from_numpy(g64)).abs().sum())
    print(f"{name}: <upfirdn(x), g> = {lhs:.9e}, <x, grad> = {rhs:.9e}")
    # 1e-5 relative: of the value, and never tighter than the float32 rounding of the terms the value is the sum of
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1e-2 * scale)


def graph_nodes(t):
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo += [nxt for nxt, _ in fn.next_functions]
    return [type(fn).__name__ for fn in seen]


def test_resample_is_one_native_node_and_honours_a_grad_sink():
    from grafx_amd import autograd as diff
    from grafx_amd import ops
    from grafx_amd.resample import Resample

    mod = Resample(44100, 48000).cuda()
    x = f64.noise((f64.ROWS, C, 700), seed=2)[1].cuda().requires_grad_(True)
    y = mod(x)
    nodes = graph_nodes(y)
    assert nodes.count("UpfirdnFnBackward") == 1 and not [n for n in nodes if "onv" in n], nodes
    g = torch.randn_like(y)
    buf = torch.zeros(f64.ROWS, 2, C, 700, device="cuda")
    with diff.grad_sink(x, buf[:, 1]) as sink:
        (grad,) = torch.autograd.grad(y, x, g)
        assert sink.writes == 1
    assert grad.data_ptr() == buf[:, 1].data_ptr() and torch.count_nonzero(buf[:, 0]) == 0
    assert torch.equal(buf[:, 1], ops.upfirdn(g, mod.taps.flip(0), mod.down, mod.up, mod.taps.numel() - 1 - mod.offset, n_out=700))
    with pytest.raises(ValueError, match="taps get no gradient"):
        diff.UpfirdnFn.apply(x, mod.taps.clone().requires_grad_(True), mod.up, mod.down, mod.offset, 10)


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_ops_refuse_bad_arguments():
    from grafx_amd import ops

    x = torch.randn(2, 2, 100, device="cuda")
    h = torch.randn(49, device="cuda")
    with pytest.raises(RuntimeError, match="CPU tensor"):    # the signal: as everywhere in the product path
        ops.upfirdn(x.cpu(), h, 4, 1)
    with pytest.raises(TypeError, match="on the GPU"):
        ops.upfirdn(x, h.cpu(), 4, 1)
    with pytest.raises(TypeError, match="float32"):
        ops.upfirdn(x, h.double(), 4, 1)
    with pytest.raises(TypeError, match="float32"):
        ops.upfirdn(x.double(), h, 4, 1)
    for offset in (-1, 49, 1.0):
        with pytest.raises(ValueError, match="offset"):
            ops.upfirdn(x, h, 4, 1, offset)
        with pytest.raises(ValueError, match="offset"):
            ops.upfirdn_absmax(x, h, 4, 1, offset)
    for bad in (0, 1025, -3, 2.0):
        with pytest.raises(ValueError, match="up="):
            ops.upfirdn(x, h, bad, 1)
        with pytest.raises(ValueError, match="down="):
            ops.upfirdn(x, h, 1, bad)
        with pytest.raises(ValueError, match="down="):
            ops.upfirdn_absmax(x, h, 1, bad)
    with pytest.raises(ValueError, match="taps"):
        ops.upfirdn(x, torch.zeros(16385, device="cuda"), 4, 1)
    with pytest.raises(ValueError, match="taps"):
        ops.upfirdn(x, h.view(7, 7), 4, 1)
    with pytest.raises(ValueError, match="n_out"):
        ops.upfirdn(x, h, 4, 1, n_out=0)


# ------------------------------------------------------------------------------------------------ 6: the module
@pytest.mark.parametrize("orig,new", [(44100, 48000), (48000, 16000), (44100, 44100), (1, 4)])
def test_resample_output_length(orig, new):
    from grafx_amd.resample import Resample, resample

    mod = Resample(orig, new).cuda()
    assert mod.taps.is_cuda and mod.taps.dtype == torch.float32
    for shape in ((2, 1001), (3, 2, 1000), (2, 2, 1, 777), (2, 1, 2, 1, 50)):
        x = torch.randn(*shape, device="cuda")
        y = mod(x)
        assert y.shape == (*shape[:-1], math.ceil(shape[-1] * new / orig))
        assert (y is x) == (orig == new)
        assert torch.equal(resample(x, orig, new), y)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        mod(torch.randn(2, 100))


def test_resample_reads_a_strided_view_in_place():
    from grafx_amd.resample import Resample

    mod = Resample(48000, 16000).cuda()
    buf = torch.randn(2, 4, C, 1000 + 8, device="cuda")
    view = buf[:, 1:3, :, 3:1003]
    assert torch.equal(mod(view), mod(view.contiguous()))


def test_resample_of_a_passband_tone():
    """A 0.05 fs tone, 147/160: the GPU against the yardstick at 1e-5; the yardstick itself holds the analytically resampled
    tone to the accuracy of the design (5e-4, the deviation of its passband gain from 1), away from the ends."""
    from grafx_amd.resample import Resample

    L = 2000
    x = torch.sin(2.0 * math.pi * 0.05 * torch.arange(L, dtype=torch.float64)).float().view(1, 1, L)
    h, up, down, offset = f64.sinc_kernel(44100, 48000)
    M = -(-L * up // down)
    want = f64.upfirdn(x.double().numpy(), f64.taps32(h)[0], up, down, offset, M)
    got = Resample(44100, 48000).cuda()(x.cuda())
    assert_close_rows(got, torch.from_numpy(want), TOL, "Resample of a tone")
    tone = np.sin(2.0 * math.pi * 0.05 * np.arange(M) * down / up)
    inner = slice(20, M - 20)
    print(f"yardstick against the analytic tone: {np.abs(want[0, 0, inner] - tone[inner]).max():.3e}; "
          f"GPU: {np.abs(got[0, 0].double().cpu().numpy()[inner] - tone[inner]).max():.3e}")
    assert np.abs(want[0, 0, inner] - tone[inner]).max() <= 1e-3


def test_resample_refuses_a_ratio_beyond_the_kernel():
    from grafx_amd.resample import Resample

    with pytest.raises(ValueError, match="44100/44101"):
        Resample(44100, 44101)
