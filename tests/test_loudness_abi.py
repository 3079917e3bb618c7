"""The loudness meter without a GPU: its C entries are declared, bound and exported; the workspace query returns the size the
header documents; the entries refuse bad arguments before any launch; k_weighting reproduces the standard's table and the
yardstick; and the gating (plain torch ops) agrees with the float64 yardstick on the CPU, gradient included."""
import math
import os

import pytest
import torch

import loudness_float64 as f64
from abi_checks import device_pointer, entries_match, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gfx_kweight_energy_ws_bytes", "gfx_kweight_energy_f32", "gfx_kweight_energy_bwd_f32")
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
TABLE_B = ((1.53512485958697, -2.69169618940638, 1.19839281085285), (1.0, -2.0, 1.0))
TABLE_A = ((1.0, -1.69065929318241, 0.73248077421585), (1.0, -1.99004745483398, 0.99007225036621))


def test_the_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "grafx_amd.h")).read()
    assert "gfx_kweight_energy_ws_bytes = R * C * ceil(L / 1024) * 64 bytes" in header
    entries_match(ENTRIES)


def test_workspace_query_returns_the_documented_size():
    from grafx_amd import ops

    for R, C, L in ((1, 1, 1), (1, 1, 1024), (1, 1, 1025), (3, 2, 144001), (66000, 1, 520), (8, 2, 262144)):
        assert ops.kweight_energy_ws_bytes(R, C, L) == R * C * -(-L // 1024) * 64, (R, C, L)
    for bad in ((0, 2, 100), (2, 0, 100), (2, 2, 0), (-1, 2, 100), (2, -2, 100), (2, 2, -100)):
        assert ops.kweight_energy_ws_bytes(*bad) == 0, bad
    # forward + backward at (8, 2, 262144) stay below a tenth of the signal: the states are no second signal
    assert ops.kweight_energy_ws_bytes(8, 2, 262144) * 10 <= 8 * 2 * 262144 * 4


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every check of the two entries comes before their first launch, so the refusals need no GPU
    (abi_checks.device_pointer; the coefficients are host memory and are read)."""
    import ctypes

    from grafx_amd import _lib

    lib = _lib.lib()
    R, C, L, hop = 3, 2, 2000, 100
    need = lib.gfx_kweight_energy_ws_bytes(R, C, L)
    assert need == R * C * 2 * 64
    p, _held = device_pointer()

    def doubles(values):
        return (ctypes.c_double * 10)(*values)

    good = f64.coef(48000).reshape(-1).tolist()
    rm, empty = _lib.RowMap(R, 0, C * L, L), _lib.RowMap(0, 0, C * L, L)
    fwd = dict(x=p, xmap=rm, coef=doubles(good), energy=p, R=R, C=C, L=L, hop=hop, ws=p, ws_bytes=need, stream=None)
    bwd = dict(x=p, xmap=rm, coef=doubles(good), genergy=p, gx=p, gmap=rm, R=R, C=C, L=L, hop=hop, accumulate=0, ws=p,
               ws_bytes=need, stream=None)
    bad = {
        "no signal": dict(x=None),
        "no coefficients": dict(coef=None),
        "no workspace": dict(ws=None),
        "a workspace off the 16-byte grid": dict(ws=p + 8),
        "no rows": dict(R=0),
        "negative rows": dict(R=-3),
        "no channels": dict(C=0),
        "negative channels": dict(C=-2),
        "no samples": dict(L=0),
        "negative length": dict(L=-1000),
        "hop = 0": dict(hop=0),
        "negative hop": dict(hop=-100),
        "hop above L": dict(hop=L + 1),
        "an empty row map": dict(xmap=empty),
        **{f"coefficient {i} = {v}": dict(coef=doubles(good[:i] + [v] + good[i + 1:]))
           for i in range(10) for v in (math.nan, math.inf, -math.inf)},
    }
    only_fwd = {"no energies": dict(energy=None), "energies off the 8-byte grid": dict(energy=p + 4)}
    only_bwd = {"no cotangent": dict(genergy=None), "no gradient": dict(gx=None), "an empty gradient row map": dict(gmap=empty),
                "a cotangent off the 8-byte grid": dict(genergy=p + 4)}
    refused(lib.gfx_kweight_energy_f32, fwd, {**bad, **only_fwd})
    refused(lib.gfx_kweight_energy_bwd_f32, bwd, {**bad, **only_bwd})
    short = {"a workspace one byte short": dict(ws_bytes=need - 1)}
    refused(lib.gfx_kweight_energy_f32, fwd, short, code=-2)
    refused(lib.gfx_kweight_energy_bwd_f32, bwd, short, code=-2)


def test_k_weighting_is_the_table_of_the_standard_at_48_khz():
    from grafx_amd.loudness import k_weighting

    Bs, As = k_weighting(48000)
    assert Bs.dtype == As.dtype == torch.float64 and Bs.shape == As.shape == (2, 3)
    assert (Bs - torch.tensor(TABLE_B, dtype=torch.float64)).abs().max() <= 1e-12
    assert (As - torch.tensor(TABLE_A, dtype=torch.float64)).abs().max() <= 1e-12


@pytest.mark.parametrize("fs", [44100, 8000, 4410])
def test_k_weighting_agrees_with_the_yardstick(fs):
    from grafx_amd.loudness import k_weighting

    Bs, As = k_weighting(fs)
    for i, (b, a) in enumerate(f64.k_weighting(fs)):
        assert (Bs[i] - torch.from_numpy(b)).abs().max() <= 1e-14 and (As[i] - torch.from_numpy(a)).abs().max() <= 1e-14
        assert As[i, 0] == 1.0


def test_k_weighting_refuses_a_shelf_at_or_above_nyquist():
    from grafx_amd.loudness import k_weighting

    for fs in (0, -48000, 3000, 2 * 1681.974450955533):
        with pytest.raises(ValueError, match="sample_rate"):
            k_weighting(fs)
    k_weighting(3400)


@pytest.mark.parametrize("fs", f64.GATING_RATES)
def test_gating_agrees_with_the_yardstick(fs):
    """gated_loudness on the yardstick's float64 energies: the loudness within 1e-9 LU, its gradient with respect to the
    energies within 1e-9 relative.  37 blocks, 7 below the absolute gate, 10 below the relative one."""
    from grafx_amd.loudness import gated_loudness

    case = f64.gating_case(fs)
    sums = case["sums"].clone().requires_grad_(True)
    got = gated_loudness(sums / case["hop"], 4, (1.0, 1.0))
    got.backward()
    print(f"{fs} Hz: {float(got.detach()):.6f} LUFS, yardstick {float(case['loudness']):.6f}")
    assert got.dtype == torch.float64 and got.shape == ()
    assert abs(float(got.detach()) - float(case["loudness"])) <= 1e-9
    assert (sums.grad - case["dsums"]).abs().max() <= 1e-9 * case["dsums"].abs().max()
    level = case["blocks"]
    assert level.numel() == 37 and int((level <= -70).sum()) == 7
    kept = sums.grad.sum(0) != 0          # a sub-block inside any kept block
    assert 0 < int(kept.sum()) < kept.numel()


def test_gating_takes_a_batch_channel_gains_and_other_gates():
    from grafx_amd.loudness import gated_loudness

    a, b = f64.gating_case(4410), f64.gating_case(4410, seed=2)
    e = torch.stack([a["sums"], b["sums"], 4.0 * a["sums"]]) / a["hop"]
    got = gated_loudness(e, 4, (1.0, 1.0))
    assert got.shape == (3,)
    assert abs(float(got[0] - a["loudness"])) <= 1e-9 and abs(float(got[1] - b["loudness"])) <= 1e-9
    # a doubled signal: four times the energies, + 20 log10 2 (the relative gate moves with it, the absolute one stays clear)
    assert abs(float(got[2] - got[0]) - 20.0 * math.log10(2.0)) <= 1e-9
    want, _ = f64.gated(a["sums"] / a["hop"], 4, (1.0, 1.41), absolute=-60.0, relative=-8.0)
    assert abs(float(gated_loudness(e[0], 4, (1.0, 1.41), -60.0, -8.0) - want)) <= 1e-9
    with pytest.raises(ValueError, match="channel"):
        gated_loudness(e, 4, (1.0,))
    with pytest.raises(ValueError, match="block_hops"):
        gated_loudness(e[..., :3], 4, (1.0, 1.0))


def test_a_silent_item_is_minus_infinity_with_a_zero_gradient():
    from grafx_amd.loudness import gated_loudness

    case = f64.gating_case(4410)
    e = torch.stack([torch.zeros_like(case["sums"]), case["sums"] / case["hop"], 1e-12 * case["sums"]]).requires_grad_(True)
    got = gated_loudness(e, 4, (1.0, 1.0))
    assert got[0] == -math.inf and got[2] == -math.inf and torch.isfinite(got[1])      # silent; all under the absolute gate
    torch.where(torch.isfinite(got), got, torch.zeros_like(got)).sum().backward()
    assert torch.isfinite(e.grad).all() and torch.count_nonzero(e.grad[0]) == 0 and torch.count_nonzero(e.grad[2]) == 0
    assert torch.count_nonzero(e.grad[1]) > 0
    e.grad = None
    gated_loudness(e, 4, (1.0, 1.0)).sum().backward()                                 # the -inf items in the sum: still no NaN
    assert not torch.isnan(e.grad).any()


def test_constructor_refusals():
    from grafx_amd.loudness import IntegratedLoudness

    meter = IntegratedLoudness(48000)
    assert (meter.hop, meter.block_hops) == (4800, 4) and meter.coef.shape == (2, 5) and not list(meter.parameters())
    assert (IntegratedLoudness(44100).hop, IntegratedLoudness(4410).hop) == (4410, 441)
    assert IntegratedLoudness(48000, block=0.4, overlap=0.0).block_hops == 1
    with pytest.raises(ValueError, match="whole number of samples"):
        IntegratedLoudness(44101)
    with pytest.raises(ValueError, match="hops"):
        IntegratedLoudness(48000, overlap=0.6)            # hop 7680: a block of 19200 samples is 2.5 hops
    with pytest.raises(ValueError, match="hops"):
        IntegratedLoudness(48000, overlap=0.95)           # 20 hops a block
    with pytest.raises(ValueError, match="sample_rate"):
        IntegratedLoudness(3000)


def test_module_refuses_cpu_tensors_and_short_signals():
    from grafx_amd.loudness import IntegratedLoudness, loudness_normalize

    meter = IntegratedLoudness(4410)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        meter(torch.zeros(2, 1, 1764))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        loudness_normalize(torch.zeros(2, 1, 1764), -23.0, meter)
    with pytest.raises(ValueError, match="less than one block"):
        meter(torch.zeros(2, 1, 1763))
