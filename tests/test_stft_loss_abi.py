"""The STFT loss without a GPU: its C entries are declared, bound and exported; the workspace query returns the size the
header documents; the entries refuse bad arguments before any launch; the inputs of the GPU tests keep clear of the points
where the loss's gradient jumps; and the module's torch formula agrees with the float64 yardstick on the CPU."""
import os

import pytest
import torch
from conftest import assert_close

import stft_loss_float64 as f64
from abi_checks import device_pointer, entries_match, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gfx_stft_loss_ws_bytes", "gfx_stft_loss_sums_f32", "gfx_stft_loss_bwd_f32")


def documented(R, L, n_fft, hop):
    """R * ceil((1 + L / hop) * n_fft / 16384) * 16 bytes: one quadruple of floats per row and run of 16384 / n_fft frames."""
    return R * -(-(1 + L // hop) * n_fft // 16384) * 16


def test_the_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "grafx_amd.h")).read()
    assert "gfx_stft_loss_ws_bytes = R * ceil((1 + L / hop) * n_fft / 16384) * 16 bytes" in header
    entries_match(ENTRIES)


def test_workspace_query_returns_the_documented_size():
    from grafx_amd import ops

    assert documented(3, 65, 128, 32) == 3 * 16 and documented(3, 20001, 512, 50) == 3 * 13 * 16
    for n_fft, hop, L, _ in f64.SHAPES:
        for R in (1, 3, 65537):
            assert ops.stft_loss_ws_bytes(R, L, n_fft, hop) == documented(R, L, n_fft, hop), (R, L, n_fft, hop)
    # 8 frames per workgroup at n_fft = 2048: the ninth frame starts a second run
    assert ops.stft_loss_ws_bytes(1, 7 * 512 + 511, 2048, 512) == 16 and ops.stft_loss_ws_bytes(1, 8 * 512, 2048, 512) == 32


def test_workspace_query_returns_zero_for_a_bad_argument():
    from grafx_amd import ops

    for R, L, n_fft, hop in ((0, 1000, 128, 32), (-1, 1000, 128, 32), (3, 64, 128, 32), (3, 0, 128, 32), (3, 1000, 64, 16),
                             (3, 5000, 4096, 1024), (3, 1000, 384, 96), (3, 1000, 128, 0), (3, 1000, 128, 129)):
        assert ops.stft_loss_ws_bytes(R, L, n_fft, hop) == 0, (R, L, n_fft, hop)


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every check of the two entries comes before their first launch, so the refusals need no GPU
    (abi_checks.device_pointer)."""
    from grafx_amd import _lib

    lib = _lib.lib()
    R, L, n_fft, hop = 3, 1000, 128, 32
    need = lib.gfx_stft_loss_ws_bytes(R, L, n_fft, hop)
    assert need == documented(R, L, n_fft, hop) > 0
    p, _held = device_pointer()
    rm = _lib.RowMap(R, 0, L, 0)
    empty = _lib.RowMap(0, 0, L, 0)
    sums = dict(pred=p, pmap=rm, target=p, tmap=rm, window=p, sums=p, R=R, L=L, n_fft=n_fft, hop=hop, eps=1e-8, ws=p,
                ws_bytes=need, stream=None)
    bwd = dict(pred=p, pmap=rm, target=p, tmap=rm, window=p, coef=p, gpred=p, gmap=rm, R=R, L=L, n_fft=n_fft, hop=hop,
               eps=1e-8, accumulate=0, ws=p, ws_bytes=need, stream=None)
    big = 1 << 20
    bad = {
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
    only_bwd = {"no coefficients": dict(coef=None), "no gradient": dict(gpred=None), "an empty gradient row map": dict(gmap=empty)}
    refused(lib.gfx_stft_loss_sums_f32, sums, {**bad, **only_sums})
    refused(lib.gfx_stft_loss_bwd_f32, bwd, {**bad, **only_bwd})
    short = {"a workspace one byte short": dict(ws_bytes=need - 1)}
    refused(lib.gfx_stft_loss_sums_f32, sums, short, code=-2)
    refused(lib.gfx_stft_loss_bwd_f32, bwd, short, code=-2)


def test_the_inputs_keep_clear_of_the_jumps_of_the_gradient():
    """E and D are sums of absolute values and the clamp is a switch: their gradients jump where |P| = |T| and where
    P.re^2 + P.im^2 = eps.  A float32 evaluation can only be held to 1e-5 of float64 where the float64 spectra stay some
    hundred float32 roundings away from both; the thresholds are those conditions (a seed that misses one is changed, not
    the threshold)."""
    for n_fft, hop, L, eps in f64.SHAPES:
        for kind in f64.KINDS:
            band, gap = f64.margins(*f64.inputs(n_fft, hop, L, kind), n_fft, hop, eps)
            print(f"{n_fft}/{hop}/{L} eps={eps:g} {kind}: clamp band {band:.2e}, magnitude gap {gap:.2e}")
            assert band >= 2e-5, (n_fft, hop, L, kind, band)
            if kind != "noise" and eps != 1e-8:
                assert gap >= 2e-5, (n_fft, hop, L, kind, gap)
            if kind == "noise" and (n_fft, hop, L, eps) in f64.SMALL:
                assert gap >= 1e-4, (n_fft, hop, L, kind, gap)


@pytest.mark.parametrize("sum_and_difference", [False, True])
def test_torch_forward_agrees_with_float64_on_the_cpu(sum_and_difference):
    from grafx_amd.losses import MultiResolutionSTFTLoss

    (n1, h1, L, eps), (n2, h2) = f64.SHAPES[1], (384, 96)     # 128/32/1000 and, on the same samples, a 300-sample window in 384
    target, noise = f64.draw(n1, h1, 4 * L, rows=1)
    target, noise = target.view(2, 2, L), noise.view(2, 2, L)
    pred = (0.5 * target + 0.02 * noise).requires_grad_(True)
    module = MultiResolutionSTFTLoss((n1, n2), (h1, h2), (n1, 300), w_sc=1.0, w_log_mag=0.7, w_lin_mag=0.3, eps=eps,
                                     sum_and_difference=sum_and_difference)
    assert not list(module.parameters())
    loss = module.torch_forward(pred, target)
    loss.backward()
    want, want_grad = f64.loss_and_grad(pred.detach(), target, ((n1, h1, n1), (n2, h2, 300)), 1.0, 0.7, 0.3, eps,
                                        sum_and_difference)
    assert_close(loss.detach().reshape(1), want.reshape(1), 1e-5, "torch_forward loss")
    assert_close(pred.grad, want_grad, 1e-5, "torch_forward gradient")


def test_identical_signals_give_zero_loss_and_zero_gradient_in_torch_forward():
    from grafx_amd.losses import MultiResolutionSTFTLoss

    target = f64.draw(128, 32, 1000)[0]
    pred = target.clone().requires_grad_(True)
    loss = MultiResolutionSTFTLoss((128,), (32,), w_lin_mag=1.0).torch_forward(pred, target)
    loss.backward()
    assert loss.item() == 0.0 and torch.count_nonzero(pred.grad) == 0 and torch.isfinite(pred.grad).all()


def test_module_refuses_cpu_tensors_on_the_native_path_and_a_target_that_requires_grad():
    from grafx_amd.losses import MultiResolutionSTFTLoss

    module = MultiResolutionSTFTLoss((128,), (32,))
    pred, target = f64.inputs(128, 32, 1000, "half")
    with pytest.raises(RuntimeError, match="CPU tensor"):
        module(pred, target)
    with pytest.raises(ValueError, match="target"):
        module(pred, target.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="shape"):
        module(pred, target[:, :-1])
