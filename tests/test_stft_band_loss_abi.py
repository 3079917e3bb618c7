"""The STFT loss on a filterbank scale without a GPU: its C entries are declared, bound and exported and refuse bad arguments
before any launch; the mel and A-weighting formulas agree with their numpy restatement; filterbank_bands returns the band
structure of every table entry and tells a staircase from what is none; the module's torch formula with filterbanks agrees
with the float64 yardstick on the CPU; and the inputs of the GPU tests keep clear of the jumps of the gradient."""
import math
import os

import numpy as np
import pytest
import torch
from conftest import assert_close

import stft_band_loss_float64 as b64
import stft_loss_float64 as f64
from abi_checks import device_pointer, entries_match, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gfx_stft_band_loss_sums_f32", "gfx_stft_band_loss_bwd_f32")
TABLE = ([("mel", n) for n in b64.MEL_BANDS] + [(name, n) for name in b64.ANY for n in (128, 512, 2048)] + [("htk", 512)])


def test_the_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "grafx_amd.h")).read()
    for said in ("Staircase contract", "caller's to guarantee", "n_bins outside"):
        assert said in header
    entries_match(ENTRIES)


def test_entries_refuse_bad_arguments_before_any_launch():
    """As for the plain entries (tests/test_stft_loss_abi.py): every check comes before the first launch, so the refusals
    need no GPU (abi_checks.device_pointer)."""
    from grafx_amd import _lib

    lib = _lib.lib()
    R, L, n_fft, hop, n_bins = 3, 1000, 128, 32, 8
    need = lib.gfx_stft_loss_ws_bytes(R, L, n_fft, hop)
    assert need > 0
    p, _held = device_pointer()
    rm = _lib.RowMap(R, 0, L, 0)
    empty = _lib.RowMap(0, 0, L, 0)
    sums = dict(pred=p, pmap=rm, target=p, tmap=rm, window=p, fb=p, row_lo=p, row_hi=p, n_bins=n_bins, sums=p, R=R, L=L,
                n_fft=n_fft, hop=hop, eps=1e-8, ws=p, ws_bytes=need, stream=None)
    bwd = dict(pred=p, pmap=rm, target=p, tmap=rm, window=p, fb=p, row_lo=p, row_hi=p, col_lo=p, col_hi=p, n_bins=n_bins,
               coef=p, gpred=p, gmap=rm, R=R, L=L, n_fft=n_fft, hop=hop, eps=1e-8, accumulate=0, ws=p, ws_bytes=need,
               stream=None)
    big = 1 << 20
    bad = {
        "no filterbank": dict(fb=None),
        "no row_lo": dict(row_lo=None),
        "no row_hi": dict(row_hi=None),
        "n_bins = 0": dict(n_bins=0),
        "negative n_bins": dict(n_bins=-1),
        "n_bins = n_fft / 2 + 2": dict(n_bins=n_fft // 2 + 2),
        # everything the plain entries refuse
        "no pred": dict(pred=None),
        "no target": dict(target=None),
        "no window": dict(window=None),
        "no workspace": dict(ws=None),
        "no rows": dict(R=0),
        "negative rows": dict(R=-3),
        "n_fft = 384, no power of two": dict(n_fft=384, ws_bytes=big),
        "n_fft = 64": dict(n_fft=64, ws_bytes=big),
        "n_fft = 4096": dict(n_fft=4096, L=5000, ws_bytes=big),
        "hop = 0": dict(hop=0, ws_bytes=big),
        "hop above n_fft": dict(hop=129, ws_bytes=big),
        "L = n_fft / 2": dict(L=64, ws_bytes=big),
        "eps = 0": dict(eps=0.0),
        "negative eps": dict(eps=-1e-8),
        "an empty pred row map": dict(pmap=empty),
        "an empty target row map": dict(tmap=empty),
    }
    only_sums = {"no sums": dict(sums=None)}
    only_bwd = {"no col_lo": dict(col_lo=None), "no col_hi": dict(col_hi=None), "no coefficients": dict(coef=None),
                "no gradient": dict(gpred=None), "an empty gradient row map": dict(gmap=empty)}
    refused(lib.gfx_stft_band_loss_sums_f32, sums, {**bad, **only_sums})
    refused(lib.gfx_stft_band_loss_bwd_f32, bwd, {**bad, **only_bwd})
    # the widest filterbank is accepted as far as the checks go: a workspace one byte short is the next refusal
    short = {f"a workspace one byte short, n_bins = {n}": dict(n_bins=n, ws_bytes=need - 1) for n in (n_bins, n_fft // 2 + 1)}
    refused(lib.gfx_stft_band_loss_sums_f32, sums, short, code=-2)
    refused(lib.gfx_stft_band_loss_bwd_f32, bwd, short, code=-2)


# ------------------------------------------------------------------------------------------------ the formulas
def test_mel_filterbank_and_a_weighting_equal_their_numpy_restatement():
    from grafx_amd.losses import a_weighting, mel_filterbank

    for n_fft, n_mels in b64.MEL_BANDS.items():
        got = mel_filterbank(b64.SAMPLE_RATE, n_fft, n_mels)
        want = b64.mel_numpy(b64.SAMPLE_RATE, n_fft, n_mels)
        assert got.dtype == torch.float32 and got.shape == (n_mels, n_fft // 2 + 1)
        assert np.abs(got.double().numpy() - want).max() <= 1e-6 * np.abs(want).max(), (n_fft, n_mels)
    for kwargs in (dict(htk=True, norm=None), dict(htk=True), dict(norm=None), dict(f_min=300.0, f_max=8000.0)):
        got, want = mel_filterbank(b64.SAMPLE_RATE, 512, 40, **kwargs), b64.mel_numpy(b64.SAMPLE_RATE, 512, 40, **kwargs)
        assert np.abs(got.double().numpy() - want).max() <= 1e-6 * np.abs(want).max(), kwargs
    assert float(mel_filterbank(b64.SAMPLE_RATE, 512, 40, norm=None).max()) <= 1.0
    for n_fft in (128, 2048):
        got, want = a_weighting(b64.SAMPLE_RATE, n_fft), b64.a_weighting_numpy(b64.SAMPLE_RATE, n_fft)
        assert got.dtype == torch.float32 and got.shape == (n_fft // 2 + 1,) and float(got[0]) == 0.0
        assert np.abs(got.double().numpy() - want).max() <= 1e-6 * np.abs(want).max()
    # a transform with a bin at 1 kHz exactly: gain 1 there
    assert abs(float(a_weighting(32000, 128)[4]) - 1.0) <= 1e-6


def test_the_mel_scales_at_their_landmarks():
    from grafx_amd import losses

    assert abs(float(losses._hz_to_mel(1000.0, htk=False)) - 15.0) <= 1e-12
    assert abs(float(b64.hz_to_mel(1000.0)) - 15.0) <= 1e-12
    htk_700 = 2595.0 * math.log10(2.0)
    assert abs(float(losses._hz_to_mel(700.0, htk=True)) - htk_700) <= 1e-9 and abs(float(b64.hz_to_mel(700.0, htk=True)) - htk_700) <= 1e-9
    for htk in (False, True):
        f = torch.tensor([0.0, 440.0, 999.0, 1000.0, 1001.0, 8000.0, 22050.0], dtype=torch.float64)
        assert torch.allclose(losses._mel_to_hz(losses._hz_to_mel(f, htk), htk), f, rtol=1e-12, atol=1e-9)


# ------------------------------------------------------------------------------------------------ the bands
@pytest.mark.parametrize("name,n_fft", TABLE, ids=[f"{n}-{s}" for n, s in TABLE])
def test_filterbank_bands_of_the_table(name, n_fft):
    from grafx_amd.losses import filterbank_bands

    W = b64.filterbank(name, n_fft)
    got = filterbank_bands(W)
    assert got is not None and len(got) == 4
    for g, want in zip(got, b64.bands_numpy(W.numpy())):
        assert g.dtype == torch.int32 and np.array_equal(g.numpy(), want)
    row_lo, row_hi, col_lo, col_hi = (g.numpy() for g in got)
    per_bin = col_hi - col_lo
    if name in ("mel", "htk"):
        assert per_bin.max() <= 2 and (per_bin == 0).sum() >= 1
    if name == "boxes":
        assert per_bin.max() == 5 and (row_hi - row_lo == 9).all()
    if name == "aweight":
        assert per_bin[0] == 0 and (per_bin[1:] == 1).all()
    if name == "one":
        assert W.shape[0] == 1 and row_lo[0] == 0 and row_hi[0] == n_fft // 2 + 1


def test_filterbank_bands_tells_what_is_no_staircase_and_refuses_what_has_no_logarithm():
    from grafx_amd.losses import filterbank_bands, mel_filterbank

    W = b64.filterbank("boxes", 128).clone()
    gap = W.clone()
    gap[3, 8] = 0.0                                          # row 3 covers 6 .. 14: a hole inside it
    assert filterbank_bands(gap) is None
    assert filterbank_bands(W.flip(0)) is None               # rows from the top down
    swapped = W.clone()
    swapped[[4, 5]] = swapped[[5, 4]]
    assert filterbank_bands(swapped) is None
    negative = W.clone()
    negative[7, 16] = -0.1
    with pytest.raises(ValueError, match="row 7"):
        filterbank_bands(negative)
    with pytest.raises(ValueError, match="row 0"):
        filterbank_bands(mel_filterbank(44100, 128, 64))     # 64 bands on 65 bins: rows without a bin
    with pytest.raises(ValueError, match="too many"):
        from grafx_amd.losses import MultiResolutionSTFTLoss
        MultiResolutionSTFTLoss((128,), (32,), scale="mel", n_bins=64, sample_rate=44100)


# ------------------------------------------------------------------------------------------------ torch_forward
def _stereo_half(n_fft, hop, L):
    target, noise = f64.draw(n_fft, hop, 4 * L, rows=1)
    target, noise = target.view(2, 2, L), noise.view(2, 2, L)
    return (0.5 * target + 0.02 * noise).requires_grad_(True), target


@pytest.mark.parametrize("case", ["mel", "perceptual", "mixed", "mel+perceptual"])
def test_torch_forward_with_filterbanks_agrees_with_float64_on_the_cpu(case):
    from grafx_amd.losses import MultiResolutionSTFTLoss

    (n1, h1, L, eps), (n2, h2) = f64.SHAPES[1], (512, 50)
    pred, target = _stereo_half(n1, h1, L)
    weights = dict(w_sc=1.0, w_log_mag=0.7, w_lin_mag=0.3, eps=eps, sum_and_difference=True)
    aw = {n: torch.from_numpy(b64.a_weighting_numpy(b64.SAMPLE_RATE, n)).float() for n in (n1, n2)}
    mel = {n: torch.from_numpy(b64.mel_numpy(b64.SAMPLE_RATE, n, 8)).float() for n in (n1, n2)}
    if case == "mel":
        module = MultiResolutionSTFTLoss((n1, n2), (h1, h2), scale="mel", n_bins=8, sample_rate=b64.SAMPLE_RATE, **weights)
        banks = [mel[n1], mel[n2]]
    elif case == "perceptual":
        module = MultiResolutionSTFTLoss((n1, n2), (h1, h2), perceptual_weighting=True, sample_rate=b64.SAMPLE_RATE, **weights)
        banks = [torch.diag(aw[n])[1:] for n in (n1, n2)]
    elif case == "mixed":
        W = b64.filterbank("boxes", n1)
        module = MultiResolutionSTFTLoss((n1, n2), (h1, h2), filterbanks=(W, None), **weights)
        banks = [W, None]
    else:
        module = MultiResolutionSTFTLoss((n1, n2), (h1, h2), scale="mel", n_bins=8, sample_rate=b64.SAMPLE_RATE,
                                         perceptual_weighting=True, **weights)
        banks = [mel[n] * aw[n] for n in (n1, n2)]
    assert not list(module.parameters()) and not module.state_dict() and module.staircase
    assert module.band_counts == [n // 2 + 1 if W is None else W.shape[0] for n, W in zip((n1, n2), banks)]
    loss = module.torch_forward(pred, target)
    loss.backward()
    want, want_grad = b64.loss_and_grad(pred.detach(), target, ((n1, h1, n1), (n2, h2, n2)), banks, 1.0, 0.7, 0.3, eps, True)
    assert_close(loss.detach().reshape(1), want.reshape(1), 1e-5, "torch_forward loss")
    assert_close(pred.grad, want_grad, 1e-5, "torch_forward gradient")


def test_identity_filterbank_is_the_plain_loss_in_torch_forward():
    from grafx_amd.losses import MultiResolutionSTFTLoss

    n_fft, hop, L, eps = f64.SHAPES[1]
    results = []
    for banks in (None, (b64.filterbank("identity", n_fft),)):
        pred, target = _stereo_half(n_fft, hop, L)
        module = MultiResolutionSTFTLoss((n_fft,), (hop,), w_lin_mag=0.3, eps=eps, filterbanks=banks)
        loss = module.torch_forward(pred, target)
        loss.backward()
        results.append((loss.detach().reshape(1), pred.grad))
    assert_close(results[1][0], results[0][0], 1e-6, "loss")
    assert_close(results[1][1], results[0][1], 1e-6, "gradient")


def test_module_refuses_contradicting_and_malformed_filterbanks():
    from grafx_amd.losses import MultiResolutionSTFTLoss

    W = b64.filterbank("boxes", 128)
    with pytest.raises(ValueError, match="not both"):
        MultiResolutionSTFTLoss((128,), (32,), filterbanks=(W,), scale="mel", n_bins=8, sample_rate=44100)
    with pytest.raises(ValueError, match="n_fft / 2 \\+ 1"):
        MultiResolutionSTFTLoss((256,), (64,), filterbanks=(W,))              # 65 columns for 129 bins
    with pytest.raises(ValueError, match="one entry"):
        MultiResolutionSTFTLoss((128, 256), (32, 64), filterbanks=(W,))
    with pytest.raises(ValueError, match="sample_rate"):
        MultiResolutionSTFTLoss((128,), (32,), perceptual_weighting=True)
    with pytest.raises(ValueError, match="sample_rate"):
        MultiResolutionSTFTLoss((128,), (32,), scale="mel", n_bins=8)
    with pytest.raises(ValueError, match="learnable"):
        MultiResolutionSTFTLoss((128,), (32,), filterbanks=(W.clone().requires_grad_(True),))
    # no staircase is no error: the module is built and takes the torch path
    assert not MultiResolutionSTFTLoss((128,), (32,), filterbanks=(W.flip(0),)).staircase


# ------------------------------------------------------------------------------------------------ screening
def test_the_inputs_keep_clear_of_the_jumps_of_the_gradient():
    """E and D are sums of absolute values over the bands: their gradients jump where Pm = Tm.  For every filterbank, shape
    and kind the GPU tests differentiate through E or D, the float64 bands stay some hundred float32 roundings away from
    that (a draw that misses gets another seed in stft_band_loss_float64.RESEED; the threshold does not move), no band is
    equal exactly, and the bins keep clear of the clamp as in the plain test."""
    for name, (n_fft, hop, L, eps), kind in b64.GRADIENT_CASES:
        pred, target = b64.inputs(name, n_fft, hop, L, kind)
        band, _ = f64.margins(pred, target, n_fft, hop, eps)
        gap, equal = b64.margins(pred, target, n_fft, hop, eps, b64.filterbank(name, n_fft))
        print(f"{name} {n_fft}/{hop}/{L} eps={eps:g} {kind}: clamp band {band:.2e}, band gap {gap:.2e}, equal bands {equal}")
        assert band >= 2e-5, (name, n_fft, hop, L, kind, band)
        assert equal == 0, (name, n_fft, hop, L, kind, equal)
        assert gap >= (1e-4 if kind == "noise" else 2e-5), (name, n_fft, hop, L, kind, gap)
