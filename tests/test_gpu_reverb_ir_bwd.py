"""gfx_stft_reverb_ir_bwd_f32 (ops.stft_reverb_ir_bwd), the adjoint of the FFT form of the STFT-masked-noise tap synthesis:
g_init, g_delta and g_gain_env against float64 autograd of the formula spelled with torch.istft (reverb_float64.py), at the
project's 1e-5 of each gradient's own peak; randn parameters, randn cotangents.

The kernel takes 16 frames per workgroup, so the lengths are the forward's: T = 2 (one partly filled workgroup), the first
length off the hop, T = 16 exactly and one sample into the next block, a mid-range length, T = 32 and one sample on.  At
T = 16 the last frame of a full workgroup is the last frame of the row; 3264 / 3265 (T = 18) put a workgroup boundary
inside the row with a second, partly filled workgroup behind it."""
import pytest
import torch

from conftest import assert_close
from reverb_float64 import tap_gradients64

pytestmark = pytest.mark.gpu

LENGTHS = [193, 400, 2880, 2881, 3001, 3264, 3265, 5952, 5953]


def _setup(ir_len, R, genv, seed):
    from grafx_amd.processors import STFTMaskedNoiseReverb

    m = STFTMaskedNoiseReverb(ir_len=ir_len, gain_envelope=genv, flashfftconv=False).cuda()
    gen = torch.Generator().manual_seed(seed)
    init = torch.randn(R, 2, m.num_bins, generator=gen).cuda()
    delta = torch.randn(R, 2, m.num_bins, generator=gen).cuda()
    g = torch.randn(R, 2, m.num_frames, generator=gen).cuda() if genv else None
    gh = torch.randn(R, 2, ir_len, generator=gen).cuda()
    return m, init, delta, g, gh


def _native(m, noise, init, delta, g, gh, ms_lr, normalise, **kw):
    from grafx_amd import ops

    basis = m._istft_basis(init.device)
    ir, gain = ops.stft_reverb_ir(noise, init, delta, g, m.window, basis, m.ir_len, m.hop_length, ms_lr, schedule="fft")
    return ops.stft_reverb_ir_bwd(gh, noise, init, delta, g, m.window, basis, m.hop_length, ms_lr,
                                  ir=ir if normalise else None, row_gain=gain if normalise else None, **kw)


def _check(m, noise, init, delta, g, gh, ms_lr, normalise, what):
    got = _native(m, noise, init, delta, g, gh, ms_lr, normalise)
    want = tap_gradients64(noise, m.window, init, delta, g, gh, m.ir_len, ms_lr, normalise)
    assert (got[2] is None) == (g is None)
    for name, a, b in zip(("g_init", "g_delta", "g_gain_env"), got, want):
        assert torch.isfinite(a).all(), f"{what}: {name}"
        assert_close(a.cpu().double(), b, 1e-5, f"{what}: {name}")


@pytest.mark.parametrize("genv", [False, True])
@pytest.mark.parametrize("ir_len", LENGTHS)
def test_kernel_against_float64(ir_len, genv):
    m, init, delta, g, gh = _setup(ir_len, 3, genv, ir_len)
    for ms_lr in (True, False):
        for normalise in (True, False):
            _check(m, m.noise_stft, init, delta, g, gh, ms_lr, normalise,
                   f"ir_len {ir_len}, ms_to_lr {ms_lr}, gain envelope {genv}, normalised {normalise}")


def test_kernel_against_float64_at_the_default_length():
    m, init, delta, g, gh = _setup(60000, 1, True, 7)
    _check(m, m.noise_stft, init, delta, g, gh, True, True, "ir_len 60000")


def test_fresh_noise_per_row():
    """noise_rows = R: every row's gradient is what that row gives alone with its own noise."""
    m, init, delta, g, gh = _setup(3001, 3, True, 5)
    torch.manual_seed(5)
    noise = m.sample_noise(3, torch.device("cuda"))
    _check(m, noise, init, delta, g, gh, True, True, "noise per row")
    all_rows = _native(m, noise, init, delta, g, gh, True, True)
    for r in range(3):
        sl = slice(r, r + 1)
        alone = _native(m, noise[sl].contiguous(), init[sl], delta[sl], g[sl], gh[sl], True, True)
        for a, b in zip(all_rows, alone):
            assert torch.equal(a[sl], b)


def test_run_to_run_bits_on_a_recycled_workspace():
    from grafx_amd import ops

    m, init, delta, g, gh = _setup(5953, 3, True, 9)
    ws = torch.empty(ops.stft_reverb_ir_bwd_ws_bytes(3, 5953), dtype=torch.uint8, device="cuda")
    first = _native(m, m.noise_stft, init, delta, g, gh, True, True, ws=ws)
    ws.fill_(0xFF)   # (a NaN pattern: nothing of the previous call may be read back)
    second = _native(m, m.noise_stft, init, delta, g, gh, True, True, ws=ws)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # a workspace cut from the gradient the call reads, and one on the host: refused before any launch
    before = gh.clone()
    with pytest.raises(ValueError, match="share memory"):
        _native(m, m.noise_stft, init, delta, g, gh, True, True, ws=gh.view(torch.uint8).view(-1)[:ws.numel()])
    assert torch.equal(gh, before)
    with pytest.raises(ValueError, match="workspace"):
        _native(m, m.noise_stft, init, delta, g, gh, True, True, ws=ws.cpu())


def test_more_rows_than_one_launch_takes():
    """ops.stft_reverb_ir_bwd splits 32 780 rows into launches of 32 767 as the forward does: the rows on either side of the
    seam come out as they do in a call of their own."""
    R, ir_len = 32780, 400
    m, init, delta, g, gh = _setup(ir_len, R, True, 11)
    got = _native(m, m.noise_stft, init, delta, g, gh, True, True)
    for lo in (0, 32760, R - 10):
        sl = slice(lo, lo + 10)
        alone = _native(m, m.noise_stft, init[sl], delta[sl], g[sl], gh[sl], True, True)
        for a, b in zip(got, alone):
            assert torch.equal(a[sl], b)


def test_arguments_the_entry_refuses():
    from grafx_amd import ops
    from grafx_amd._lib import GfxError
    from grafx_amd.processors import STFTMaskedNoiseReverb

    m = STFTMaskedNoiseReverb(ir_len=1500, n_fft=256, hop_length=128, flashfftconv=False).cuda()
    p = torch.zeros(1, 2, m.num_bins, device="cuda")
    gh = torch.zeros(1, 2, 1500, device="cuda")
    with pytest.raises(GfxError):   # no backward for the matrix-core schedule's transform sizes
        ops.stft_reverb_ir_bwd(gh, m.noise_stft, p, p, None, m.window, m._istft_basis(p.device), 128, True)
    m, init, delta, g, gh = _setup(400, 1, False, 1)
    with pytest.raises(ValueError):  # the taps without their gain
        ops.stft_reverb_ir_bwd(gh, m.noise_stft, init, delta, None, m.window, m._istft_basis(init.device), 192, True,
                               ir=gh)
    with pytest.raises(ValueError):  # a workspace that is too small
        ops.stft_reverb_ir_bwd(gh, m.noise_stft, init, delta, None, m.window, m._istft_basis(init.device), 192, True,
                               ws=torch.empty(16, dtype=torch.uint8, device="cuda"))
