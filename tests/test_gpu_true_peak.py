"""The true-peak meter against its float64 definition (tests/upfirdn_float64.py): the peak and the index of
ops.upfirdn_absmax, ties, silence, the standard's example, the gradient through the arg-max, the normaliser, and the
refusals of the workspace.  The size query needs no GPU."""
import functools
import math

import numpy as np
import pytest
import torch
from conftest import assert_close_rows

import upfirdn_float64 as f64

gpu = pytest.mark.gpu
TOL = 1e-5
UP = 4
TILE = 1024          # ops.UPFIRDN_TILE (asserted below); the shapes are parameters, read before the library is


@functools.lru_cache(maxsize=None)
def taps():
    h, up, down, offset = f64.sinc_kernel(1, UP)
    assert (len(h), up, down, offset) == (49, UP, 1, 24)
    return (*f64.taps32(h), offset)


def check_peaks(got_peak, got_index, x64, what):
    """The peaks at 1e-5 of the float64 ones; the index is the float64 one wherever the runner-up there lies more than
    1e-5 below the peak, and in any case names an output that attains the peak within 1e-5."""
    h64, _, offset = taps()
    peak, index, y = f64.peak(x64, h64, UP, 1, offset, UP * x64.shape[-1])
    assert got_peak.shape == peak.shape and got_index.shape == index.shape and got_index.dtype == torch.int64
    assert_close_rows(got_peak[..., None], torch.from_numpy(peak)[..., None], TOL, what)
    a, gi = np.abs(y), got_index.cpu().numpy()
    assert (np.take_along_axis(a, gi[..., None], -1)[..., 0] >= peak * (1 - TOL)).all()
    np.put_along_axis(a, index[..., None], 0.0, -1)
    clear = a.max(-1) < peak * (1 - TOL)
    assert clear.any() and (gi[clear] == index[clear]).all(), what


@gpu
@pytest.mark.parametrize("kind", sorted(f64.KINDS))
@pytest.mark.parametrize("L,C", [(5, 1), (1000, 2), (TILE // 4 + 3, 2)])
def test_peak_and_index_match_float64(L, C, kind):
    from grafx_amd import ops

    assert ops.UPFIRDN_TILE == TILE
    _, h32, offset = taps()
    x64, x32 = f64.KINDS[kind]((f64.ROWS, C, L), seed=L + C)
    peak, index = ops.upfirdn_absmax(x32.cuda(), h32.cuda(), UP, 1, offset, n_out=UP * L)
    check_peaks(peak, index, x64, f"true peak {L}/{C} {kind}")
    y = ops.upfirdn(x32.cuda(), h32.cuda(), UP, 1, offset, n_out=UP * L)         # the same tiles, written
    assert torch.equal(peak, y.abs().amax(-1)) and torch.equal(index, y.abs().argmax(-1))
    ws = torch.full((ops.upfirdn_absmax_ws_bytes(f64.ROWS, C, UP * L) + 64,), 0xff, dtype=torch.uint8, device="cuda")
    again = ops.upfirdn_absmax(x32.cuda(), h32.cuda(), UP, 1, offset, n_out=UP * L, ws=ws)   # a reused workspace of any content
    assert torch.equal(again[0], peak) and torch.equal(again[1], index)


@gpu
def test_peak_of_a_strided_slice_of_a_render_buffer():
    from grafx_amd.loudness import TruePeak

    L = 1000
    x64, x32 = f64.noise_and_tone((2, 2, 2, L), seed=9)
    buf = torch.randn(2, 4, 2, L + 8, device="cuda")
    view = buf[:, 1:3, :, 3:L + 3]
    view.copy_(x32.cuda())
    meter = TruePeak().cuda()
    peaks = meter.channel_peaks(view)
    assert peaks.shape == (2, 2, 2)
    assert torch.equal(peaks, meter.channel_peaks(x32.cuda()))
    h64, _, offset = taps()
    want = f64.peak(x64, h64, UP, 1, offset, UP * L)[0]
    assert_close_rows(peaks[..., None], torch.from_numpy(want)[..., None], TOL, "channel peaks of a strided view")
    level = meter(view)
    assert level.shape == (2, 2) and level.dtype == torch.float32
    assert (level.double().cpu() - torch.from_numpy(20.0 * np.log10(want.max(-1)))).abs().max() <= 1e-4   # 20 log10(1 + 1e-5)


@gpu
def test_two_identical_impulses_give_the_index_of_the_first():
    from grafx_amd import ops

    _, h32, offset = taps()
    x = torch.zeros(1, 2, 600, device="cuda")
    x[0, 0, 10] = x[0, 0, 300] = 0.5                       # outputs 40 and 1200: two tiles
    x[0, 1, 17] = x[0, 1, 40] = x[0, 1, 599] = -0.25        # one tile, and the last sample
    peak, index = ops.upfirdn_absmax(x, h32.cuda(), UP, 1, offset, n_out=UP * 600)
    assert index.tolist() == [[40, 68]]
    assert torch.equal(peak, torch.tensor([[0.5, 0.25]], device="cuda") * h32[offset])


@gpu
def test_a_silent_item_reads_minus_infinity_with_a_zero_gradient():
    from grafx_amd import ops
    from grafx_amd.loudness import TruePeak

    x = f64.noise((3, 2, 500), seed=4)[1]
    x[1] = 0.0
    x = x.cuda().requires_grad_(True)
    meter = TruePeak().cuda()
    level = meter(x)
    assert level[1] == -math.inf and torch.isfinite(level[[0, 2]]).all()
    peak, index = ops.upfirdn_absmax(x.detach(), meter.taps, UP, 1, meter.offset, n_out=UP * 500)
    assert torch.count_nonzero(peak[1]) == 0 and torch.count_nonzero(index[1]) == 0
    loss = torch.where(torch.isfinite(level), level, torch.zeros_like(level)).sum()
    assert torch.isfinite(loss)
    loss.backward()
    assert torch.isfinite(x.grad).all() and torch.count_nonzero(x.grad[1]) == 0 and torch.count_nonzero(x.grad[0]) > 0
    x.grad = None
    meter(x).sum().backward()                                # -inf in the sum: still no NaN in the gradient
    assert torch.isfinite(x.grad).all() and torch.count_nonzero(x.grad[1]) == 0


@gpu
def test_the_example_of_the_standard():
    """sin(2 pi n / 4 + pi / 4): every sample is +-0.7071, a sample peak of -3.01 dB; the true peak is within 0.1 dB of
    0 dBTP (the float64 yardstick gives -0.03 dB with the default taps).  The tone is the standard's steady one: it is faded
    in and out over 64 samples, because a tone switched on at full level is another signal, whose reconstruction overshoots
    at the onset (+0.10 dBTP in float64 with these taps, at the tenth output)."""
    from grafx_amd.loudness import TruePeak

    L = 1000
    ramp = 0.5 - 0.5 * torch.cos(math.pi * (torch.arange(64, dtype=torch.float64) + 0.5) / 64.0)
    fade = torch.cat([ramp, torch.ones(L - 128, dtype=torch.float64), ramp.flip(0)])
    x = (fade * torch.sin(2.0 * math.pi * torch.arange(L, dtype=torch.float64) / 4.0 + math.pi / 4.0)).float().view(1, 1, L)
    assert abs(20.0 * math.log10(float(x.abs().max())) + 3.0103) <= 1e-3
    h64, _, offset = taps()
    want = 20.0 * math.log10(float(f64.peak(x.double().numpy(), h64, UP, 1, offset, UP * L)[0].max()))
    got = float(TruePeak().cuda()(x.cuda()))
    print(f"true peak of the standard's example: {got:.4f} dBTP, float64 {want:.4f}")
    assert abs(want) <= 0.1 and abs(got - want) <= 1e-4 and abs(got) <= 0.1
    assert abs(want + 0.03) <= 0.005


def yardstick_level(x, h, offset):
    """20 log10 of the largest |y| over an item's channels, y the 4x oversampled x: float64 torch ops on the CPU."""
    L, N = x.shape[-1], h.numel()
    z = torch.zeros(*x.shape[:-1], L * UP, dtype=torch.float64)
    z[..., ::UP] = x
    z = torch.nn.functional.pad(z, (N - 1 - offset, offset))
    y = torch.nn.functional.conv1d(z.reshape(-1, 1, z.shape[-1]), h.flip(0).view(1, 1, N)).view(*x.shape[:-1], L * UP)
    return 20.0 * torch.log10(y.abs().amax((-2, -1))), y


@gpu
def test_gradient_through_the_arg_max_matches_float64_autograd():
    from grafx_amd.loudness import TruePeak

    h64, h32, offset = taps()
    x32 = 0.1 * f64.noise((3, 2, 300), seed=8)[1]
    for b, (c, k, v) in enumerate(((0, 3, 2.0), (1, 150, -3.0), (0, 299, 2.5))):      # a clear peak: at either end, in the middle
        x32[b, c, k] += v
    x64 = x32.double().requires_grad_(True)
    level, y = yardstick_level(x64, torch.from_numpy(h64), offset)
    assert np.abs(y.detach().numpy() - f64.upfirdn(x32.double().numpy(), h64, UP, 1, offset, UP * 300)).max() <= 1e-12
    top = y.detach().abs().flatten(1).topk(2).values
    assert (top[:, 0] - top[:, 1] >= 1e-3 * top[:, 0]).all()       # a float32 arg-max cannot legitimately differ
    level.sum().backward()
    x = x32.cuda().requires_grad_(True)
    got = TruePeak().cuda()(x)
    assert (got.detach().double().cpu() - level.detach()).abs().max() <= 1e-4
    got.sum().backward()
    assert_close_rows(x.grad.flatten(1), x64.grad.flatten(1), TOL, "gradient of the true-peak level")
    assert int(torch.count_nonzero(x.grad)) <= 3 * math.ceil(49 / UP)


@gpu
@pytest.mark.parametrize("detach_gain", [False, True])
def test_normalize_lands_on_the_target(detach_gain):
    from grafx_amd.loudness import TruePeak, true_peak_normalize

    target = -1.0
    meter = TruePeak().cuda()
    x = f64.noise_and_tone((3, 2, 2000), seed=6)[1]
    x[1] = 0.0
    x[2] *= 0.01
    x = x.cuda().requires_grad_(True)
    y = true_peak_normalize(x, target, meter, detach_gain=detach_gain)
    level = meter(y.detach())
    assert abs(float(level[0]) - target) <= 1e-3 and abs(float(level[2]) - target) <= 1e-3
    assert level[1] == -math.inf and torch.equal(y[1], x[1])          # a silent item comes back unchanged
    y.square().sum().backward()
    assert torch.isfinite(x.grad).all() and torch.count_nonzero(x.grad[0]) > 0 and torch.count_nonzero(x.grad[1]) == 0


@gpu
def test_custom_taps_and_refusals():
    from grafx_amd import ops
    from grafx_amd.loudness import TruePeak

    _, h32, offset = taps()
    x = f64.noise((2, 2, 400), seed=1)[1].cuda()
    assert torch.equal(TruePeak(taps=h32).cuda()(x), TruePeak().cuda()(x))     # 49 taps: (N - 1) // 2 is the design's offset
    assert TruePeak(taps=[0.25, 0.5, 1.0, 0.5]).offset == 1
    with pytest.raises(ValueError, match="oversample"):
        TruePeak(oversample=0)
    with pytest.raises(ValueError, match="taps"):
        TruePeak(taps=torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        TruePeak()(x.cpu())
    hg = h32.cuda()
    nbytes = ops.upfirdn_absmax_ws_bytes(2, 2, 1600)
    with pytest.raises(ValueError, match="workspace"):
        ops.upfirdn_absmax(x, hg, UP, 1, offset, n_out=1600, ws=torch.empty(nbytes - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="workspace"):
        ops.upfirdn_absmax(x, hg, UP, 1, offset, n_out=1600, ws=torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")[8:])
    with pytest.raises(ValueError, match="share memory"):
        ops.upfirdn_absmax(x, hg, UP, 1, offset, n_out=1600, ws=x.view(torch.uint8).view(-1))


def test_the_workspace_query_needs_no_gpu():
    from grafx_amd import ops

    assert ops.UPFIRDN_TILE == TILE
    assert ops.upfirdn_absmax_ws_bytes(2, 2, TILE + 1) == 2 * 2 * 2 * 16
    for bad in ((0, 2, 100), (2, 0, 100), (2, 2, 0), (-1, 2, 100), (2, -2, 100), (2, 2, -100)):
        assert ops.upfirdn_absmax_ws_bytes(*bad) == 0, bad
