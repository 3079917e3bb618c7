"""gfx_noise_shaping_ir_bwd_f32 (ops.noise_shaping_ir_bwd), the adjoint of the filtered-noise-shaping tap synthesis: the
gradients of log_decay, log_gain, log_fade_in and z_fade_in_gain against float64 autograd of the formula
(noise_shaping_float64.py) at the project's 1e-5 of each gradient's own peak; randn parameters, randn noise, randn
cotangents, the decay range of test_gpu_many_rows.py for short responses.

The kernel takes 2048 samples of one row-channel per workgroup, 256 at a time, so the lengths are: one sample, one past a
256 boundary, 700 (one partly filled workgroup, at the band limit K = 64), 1501 (the g19 shape, no multiple of anything) and
9000 (five workgroups per row-channel, the last one partly filled).

One bound needs a word.  The gradient through the normalisation is T1 - T2 = s G[gh] - (s^3 / C) <gh, ir> G[ir], G[v] the
un-normalised gradient against v.  Where gh is (nearly) parallel to ir in a row the two terms cancel: with one channel and
one tap they cancel to 1e-12 of their size (h = sign(ir) whatever the parameters), and neither any function of the float32
inputs ir and row_gain nor the float64 arbiter itself (2^-53 / 1e-12 = 1e-4) is determined to 1e-5 of what is left.  So the
error allowed is the larger of the issue's 1e-5 of the gradient's peak and 16 roundings of float32 (2^-20 = 9.5e-7) of the
peak of |T1| + |T2|: s, s^3, the dot product, and per sum the exponent, exp, and three products, each at most an ulp or two.
For every case but the one-tap one the first is the larger and the bound is the issue's, asserted by conftest.assert_close."""
import itertools

import pytest
import torch

from conftest import assert_close
from noise_shaping_float64 import tap_gradients64, taps64

pytestmark = pytest.mark.gpu

LO, HI = -0.2, -0.005
NAMES = ("log_decay", "log_gain", "log_fade_in", "z_fade_in_gain")
CASES = [(3, 2, 4, 1501), (2, 1, 1, 1), (2, 2, 3, 257), (1, 2, 64, 700), (2, 2, 12, 9000)]
G19 = CASES[0]
ROUNDINGS = 16 * 2.0 ** -24


def _inputs(R, C, K, ir_len, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + R + 7 * C + 31 * K + ir_len)
    noise = torch.randn(C, K, ir_len, generator=gen).cuda()
    p = {k: torch.randn(R, C, K, generator=gen).cuda() for k in NAMES}
    gh = torch.randn(R, C, ir_len, generator=gen).cuda()
    return noise, p, gh


def _params(p, fade):
    return {k: v for k, v in p.items() if fade or k in NAMES[:2]}


def _native(noise, p, gh, fade, normalise, **kw):
    from grafx_amd import ops

    q = _params(p, fade)
    ir = gain = None
    if normalise:
        ir = ops.noise_shaping_ir(noise, q["log_decay"], q["log_gain"], q.get("log_fade_in"), q.get("z_fade_in_gain"),
                                  gh.shape[-1], LO, HI)
        gain = torch.rsqrt((ir * ir).sum(-1, keepdim=True).mean(-2, keepdim=True) + 1e-12)
    return ops.noise_shaping_ir_bwd(gh, noise, q["log_decay"], q["log_gain"], q.get("log_fade_in"), q.get("z_fade_in_gain"),
                                    LO, HI, ir=ir, row_gain=gain, **kw)


def _terms64(noise, q, gh):
    """Peak per parameter of |T1| + |T2|, the two terms the normalised gradient is the difference of (module docstring)."""
    q64 = {k: v.detach().cpu().double() for k, v in q.items()}
    ir = taps64(noise, q64["log_decay"], q64["log_gain"], q64.get("log_fade_in"), q64.get("z_fade_in_gain"), LO, HI, False)
    gh = gh.detach().cpu().double()
    s = torch.rsqrt(ir.square().sum(-1, keepdim=True).mean(-2, keepdim=True) + 1e-12)
    b = s ** 3 / ir.shape[1] * (gh * ir).sum((-1, -2), keepdim=True)
    t1, t2 = tap_gradients64(noise, q, s * gh, LO, HI, False), tap_gradients64(noise, q, b * ir, LO, HI, False)
    return {k: float((t1[k].abs() + t2[k].abs()).max()) for k in q}


def _check(noise, p, gh, fade, normalise, what):
    q = _params(p, fade)
    got = _native(noise, p, gh, fade, normalise)
    want = tap_gradients64(noise, q, gh, LO, HI, normalise)
    assert list(got) == list(q)
    terms = _terms64(noise, q, gh) if normalise else {}
    for k in q:
        assert torch.isfinite(got[k]).all(), f"{what}: {k}"
        g64 = got[k].cpu().double()
        floor = ROUNDINGS * terms.get(k, 0.0)
        print(f"{what}: {k}: peak {float(want[k].abs().max()):.3e}, worst error {float((g64 - want[k]).abs().max()):.3e}, "
              f"float32 floor of the cancelling terms {floor:.3e}")
        if floor <= 1e-5 * float(want[k].abs().max()):
            assert_close(g64, want[k], 1e-5, f"{what}: {k}")
        else:   # the terms cancel beyond what float32 inputs determine
            assert float((g64 - want[k]).abs().max()) <= floor, f"{what}: {k}"


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("fade", [False, True], ids=["no_fade", "fade"])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(shape, fade, normalise):
    noise, p, gh = _inputs(*shape)
    _check(noise, p, gh, fade, normalise, f"{shape}, fade {fade}, normalised {normalise}")


def test_more_bands_than_the_kernel_holds_raise():
    from grafx_amd._lib import GfxError

    noise, p, gh = _inputs(1, 1, 65, 300)
    with pytest.raises((ValueError, GfxError)):
        _native(noise, p, gh, True, False)


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "normalised"])
def test_every_subset_of_the_gradients_is_the_full_call(normalise):
    noise, p, gh = _inputs(*G19)
    full = _native(noise, p, gh, True, normalise)
    assert tuple(full) == NAMES
    for n in range(1, 4):
        for want in itertools.combinations(NAMES, n):
            got = _native(noise, p, gh, True, normalise, want=want)
            assert tuple(got) == want
            for k in want:
                assert torch.equal(got[k], full[k]), (want, k)
    assert tuple(_native(noise, p, gh, False, normalise, want=NAMES)) == NAMES[:2]   # a parameter not given is skipped
    with pytest.raises(ValueError):
        _native(noise, p, gh, True, normalise, want=("log_gain", "noise"))


def test_run_to_run_bits_on_a_recycled_workspace():
    from grafx_amd import ops

    shape = CASES[4]
    noise, p, gh = _inputs(*shape)
    ws = torch.empty(ops.noise_shaping_ir_bwd_ws_bytes(*shape), dtype=torch.uint8, device="cuda")
    first = _native(noise, p, gh, True, True, ws=ws)
    ws.fill_(0xFF)   # (a NaN pattern: nothing of the previous call may be read back)
    second = _native(noise, p, gh, True, True, ws=ws)
    third = _native(noise, p, gh, True, True)
    for k in NAMES:
        assert torch.equal(first[k], second[k]) and torch.equal(first[k], third[k])


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "normalised"])
def test_a_row_does_not_depend_on_the_other_rows(normalise):
    noise, p, gh = _inputs(*G19)
    together = _native(noise, p, gh, True, normalise)
    for r in range(G19[0]):
        alone = _native(noise, {k: v[r:r + 1] for k, v in p.items()}, gh[r:r + 1], True, normalise)
        for k in NAMES:
            assert torch.equal(together[k][r:r + 1], alone[k]), (r, k)


def test_noise_window_into_the_pseudo_random_buffer():
    """noise_stride: a window at a non-zero offset of a (C, K, 5 ir_len) buffer against a contiguous copy of it."""
    R, C, K, ir_len = G19
    _, p, gh = _inputs(*G19)
    buffer = torch.randn(C, K, 5 * ir_len, generator=torch.Generator().manual_seed(3)).cuda()
    window = buffer[..., 1237:1237 + ir_len]
    assert not window.is_contiguous()
    for normalise in (False, True):
        a = _native(window, p, gh, True, normalise)
        b = _native(window.contiguous(), p, gh, True, normalise)
        for k in NAMES:
            assert torch.equal(a[k], b[k]), k
    _check(window, p, gh, True, True, "window into the long buffer")
    from grafx_amd import ops

    with pytest.raises(ValueError, match="noise"):   # the check of noise_shaping_ir: not a view of a band-split buffer
        ops.noise_shaping_ir_bwd(gh, buffer.transpose(0, 1)[:C, :K, :ir_len], p["log_decay"], p["log_gain"], None, None, LO, HI)


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("name", ["log_decay", "log_fade_in", "z_fade_in_gain"])
def test_saturated_parameters_have_a_zero_gradient(name, normalise):
    """Row 0 of the parameter at +100, row 1 at -100, row 2 as drawn: everything finite, exactly 0 where sigmoid' is 0."""
    noise, p, gh = _inputs(*G19)
    p = dict(p)
    p[name] = p[name].clone()
    p[name][0], p[name][1] = 100.0, -100.0
    got = _native(noise, p, gh, True, normalise)
    for k in NAMES:
        assert torch.isfinite(got[k]).all(), k
    assert float(got[name][:2].abs().max()) == 0.0
    assert float(got[name][2].abs().max()) > 0.0
    want = tap_gradients64(noise, p, gh, LO, HI, normalise)
    for k in NAMES:
        assert_close(got[k].cpu().double(), want[k], 1e-5, f"{name} saturated: {k}")


def test_more_row_channels_than_one_launch_takes():
    """R C = 65 538 > 65 535: the entry splits the launches on a channel boundary.  Against float64, and the same bits as the
    rows computed in two halves."""
    R, C, K, ir_len = 32769, 2, 1, 8
    noise, p, gh = _inputs(R, C, K, ir_len)
    for normalise in (False, True):
        _check(noise, p, gh, True, normalise, f"32769 rows, normalised {normalise}")
        whole = _native(noise, p, gh, True, normalise)
        for lo, hi in ((0, 16385), (16385, R)):
            half = _native(noise, {k: v[lo:hi] for k, v in p.items()}, gh[lo:hi], True, normalise)
            for k in NAMES:
                assert torch.equal(whole[k][lo:hi], half[k]), (lo, k)


def test_more_rows_than_one_call_takes():
    """ops.noise_shaping_ir_bwd passes 65 536 rows per call: the rows on either side of the seam come out as on their own."""
    from grafx_amd import ops

    R = ops.NS_BWD_ROWS + 3
    noise, p, gh = _inputs(R, 1, 1, 2)
    whole = _native(noise, p, gh, True, True)
    sl = slice(ops.NS_BWD_ROWS - 3, R)
    part = _native(noise, {k: v[sl] for k, v in p.items()}, gh[sl], True, True)
    for k in NAMES:
        assert torch.equal(whole[k][sl], part[k]), k


def test_on_a_side_stream():
    noise, p, gh = _inputs(*CASES[4])
    want = _native(noise, p, gh, True, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _native(noise, p, gh, True, True)
    side.synchronize()
    for k in NAMES:
        assert torch.equal(got[k], want[k]), k


def test_workspaces_the_wrapper_refuses():
    from grafx_amd import ops

    noise, p, gh = _inputs(*G19)
    need = ops.noise_shaping_ir_bwd_ws_bytes(*G19)
    assert gh.numel() * 4 >= need
    with pytest.raises(ValueError, match="share memory"):     # a workspace cut from the gradient it reads
        _native(noise, p, gh, True, False, ws=gh.view(-1).view(torch.uint8))
    with pytest.raises(ValueError, match="share memory"):
        _native(noise, p, gh, True, False, ws=noise.view(-1).view(torch.uint8))
    with pytest.raises(ValueError, match="uint8"):            # the wrong dtype
        _native(noise, p, gh, True, False, ws=torch.empty(need, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="uint8"):            # too few bytes
        _native(noise, p, gh, True, False, ws=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):                           # the taps without their gains
        ops.noise_shaping_ir_bwd(gh, noise, p["log_decay"], p["log_gain"], None, None, LO, HI, ir=gh)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")   # ... and one it takes
    a, b = _native(noise, p, gh, True, False, ws=ws), _native(noise, p, gh, True, False)
    for k in NAMES:
        assert torch.equal(a[k], b[k])
