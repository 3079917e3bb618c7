"""The oversampled waveshapers without a GPU: the three C entries are declared, bound and exported with their argument
lists; the workspace query returns the documented size and 0 for bad arguments; every refusal of the entries comes back
before a launch; the yardstick's interpolator and decimator agree with the polyphase yardstick; the alias shares of the
issue's table are reproduced in float64; and the constructors take ``oversample`` as documented."""
import numpy as np
import pytest
import torch

import oversampled_float64 as o64
import upfirdn_float64 as f64
from abi_checks import device_pointer, entries_match, refused

ENTRIES = ("gfx_oversampled_waveshaper_f32", "gfx_oversampled_waveshaper_bwd_ws_bytes", "gfx_oversampled_waveshaper_bwd_f32")
# the issue's table: factor -> alias share of tanh(e^3 x) / e^3 on the tone, float64
SHARES = {1: 1.41e-1, 2: 1.33e-2, 3: 2.68e-3, 4: 7.85e-4, 8: 2.51e-6}
CLASSES = ("TanhDistortion", "PiecewiseTanhDistortion", "PowerDistortion", "ChebyshevDistortion")


def test_the_entries_are_declared_bound_and_exported():
    fwd = ["const float*", "gfx_rowmap_t", "float*", "gfx_rowmap_t", "int64_t", "int64_t", "int64_t", "int64_t", "const float*",
           "int64_t", "int64_t", "const float*", "int64_t", "int64_t", "int", "int", "int", "const float*", "const float*",
           "const float*", "const float*", "int64_t", "const float*", "void*"]
    bwd = ["const float*", "gfx_rowmap_t", "const float*", "gfx_rowmap_t", "int64_t", "int64_t", "int64_t", "int64_t",
           "const float*", "int64_t", "int64_t", "const float*", "int64_t", "int64_t", "int", "int", "int", "const float*",
           "const float*", "const float*", "const float*", "int64_t", "const float*", "float*", "gfx_rowmap_t", "float*", "float*",
           "float*", "float*", "void*", "size_t", "void*"]
    entries_match(ENTRIES, dict(zip(ENTRIES, (("int", fwd), ("size_t", ["int64_t"] * 5), ("int", bwd)))))


def test_tile_and_workspace_query():
    from grafx_amd import _lib, ops

    assert [ops.oversampled_waveshaper_tile(f) for f in (1, 2, 3, 4, 8, 16)] == [4096, 2048, 1344, 1024, 512, 256]
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError):
            ops.oversampled_waveshaper_tile(bad)
    query = _lib.lib().gfx_oversampled_waveshaper_bwd_ws_bytes
    for R, C, L, K, f in ((1, 1, 1, 0, 1), (3, 2, 1025, 0, 4), (3, 2, 1024, 10, 4), (65537, 1, 40, 32, 2), (256, 2, 131072, 10, 4)):
        nt, ns = -(-L // ops.oversampled_waveshaper_tile(f)), (2 + K if K else 6)
        assert query(R, C, L, K, f) == 4 * (R * ns * C * nt + R * C * nt + R * C), (R, C, L, K, f)
    for bad in ((0, 2, 100, 0, 4), (2, 0, 100, 0, 4), (2, 2, 0, 0, 4), (-1, 2, 100, 0, 4), (2, 2, 100, -1, 4), (2, 2, 100, 33, 4),
                (2, 2, 100, 0, 0), (2, 2, 100, 0, 17), (2, 2, 100, 0, -2)):
        assert query(*bad) == 0, bad


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every check comes before the first launch, so the refusals need no GPU (abi_checks.device_pointer)."""
    from grafx_amd import _lib

    lib = _lib.lib()
    R, C, L, N = 3, 2, 2000, 49
    need = lib.gfx_oversampled_waveshaper_bwd_ws_bytes(R, C, L, 0, 4)
    p, _held = device_pointer()
    far = p + 4 * R * C * L      # a second signal that does not overlap the first, a third
    rm, empty, neg = _lib.RowMap(R, 0, C * L, L), _lib.RowMap(0, 0, C * L, L), _lib.RowMap(R, 0, -C * L, L)
    fwd = dict(x=p, xmap=rm, y=far, ymap=rm, R=R, C=C, L=L, factor=4, h_up=p, N_up=N, o_up=24, h_dn=p, N_dn=N, o_dn=24, mode=0,
               use_tanh=0, inverse=0, pre=p, post=None, p0=None, p1=None, K=0, dc=None, stream=None)
    bwd = dict(x=p, xmap=rm, gy=far, gmap=rm, R=R, C=C, L=L, factor=4, h_up=p, N_up=N, o_up=24, h_dn=p, N_dn=N, o_dn=24, mode=0,
               use_tanh=0, inverse=0, pre=p, post=None, p0=None, p1=None, K=0, dc=None, gx=far + 4 * R * C * L, omap=rm, g_pre=p,
               g_post=None, g_p0=None, g_p1=None, ws=p, ws_bytes=need, stream=None)
    bad = {
        "no signal": dict(x=None), "an empty row map": dict(xmap=empty), "no rows": dict(R=0), "negative rows": dict(R=-3),
        "no channels": dict(C=0), "no samples": dict(L=0), "negative length": dict(L=-5),
        "factor 0": dict(factor=0), "factor 17": dict(factor=17), "negative factor": dict(factor=-4),
        "no interpolator": dict(h_up=None), "no decimator": dict(h_dn=None),
        "no interpolator taps": dict(N_up=0, o_up=0), "1025 interpolator taps": dict(N_up=1025),
        "no decimator taps": dict(N_dn=0, o_dn=0), "1025 decimator taps": dict(N_dn=1025),
        "interpolator offset = N": dict(o_up=N), "interpolator offset -1": dict(o_up=-1),
        "decimator offset = N": dict(o_dn=N), "decimator offset -1": dict(o_dn=-1),
        "mode -1": dict(mode=-1), "mode 4": dict(mode=4), "inverse post gain without a pre gain": dict(inverse=1, pre=None),
        "piecewise without its parameters": dict(mode=1), "piecewise without thresholds": dict(mode=1, p0=p),
        "polynomial without weights": dict(mode=2, K=4), "polynomial of order 0": dict(mode=3, p0=p, K=0),
        "polynomial of order 33": dict(mode=3, p0=p, K=33),
        "more than 2^31 - 1 row-channels": dict(R=1 << 16, C=1 << 15),
        "more than 2^31 - 1 workgroups": dict(R=1 << 20, C=1, L=1024 * (1 << 11) + 1),
        "a negative stride": dict(xmap=neg),
    }
    only_fwd = {"no output": dict(y=None), "an empty output row map": dict(ymap=empty), "an output that is the input": dict(y=p),
                "an output that overlaps the input": dict(y=p + 4)}
    only_bwd = {"no output gradient": dict(gy=None), "an empty gradient row map": dict(gmap=empty),
                "nothing asked for": dict(gx=None, g_pre=None), "a gradient of a missing pre gain": dict(pre=None),
                "a post-gain gradient without a post gain": dict(g_post=p), "a bias gradient without a bias": dict(g_p0=p),
                "thresholds outside the piecewise mode": dict(g_p1=p),
                "the post gain unused under inverse_post_gain": dict(inverse=1, post=p, g_post=p),
                "gx is x": dict(gx=p), "gx is gy": dict(gx=far), "gx overlaps x a sample later": dict(gx=p + 4),
                "an empty gx row map": dict(omap=empty), "no workspace": dict(ws=None)}
    refused(lib.gfx_oversampled_waveshaper_f32, fwd, {**bad, **only_fwd})
    refused(lib.gfx_oversampled_waveshaper_bwd_f32, bwd, {**bad, **only_bwd})
    refused(lib.gfx_oversampled_waveshaper_bwd_f32, bwd, {"a workspace one byte short": dict(ws_bytes=need - 1)}, code=-2)


@pytest.mark.parametrize("factor", [1, 2, 3, 4, 8, 16])
def test_the_yardstick_agrees_with_the_polyphase_yardstick(factor):
    """interpolate and decimate are upfirdn(x, h, F, 1) and upfirdn(v, h, 1, F) of upfirdn_float64, to 1e-12; with the
    default design and with short filters whose offsets sit at either end."""
    rng = np.random.default_rng(factor)
    L = 57
    x = torch.as_tensor(rng.standard_normal((2, 3, L)))
    designs = [o64.filters(factor)] if factor > 1 else []
    designs += [(torch.as_tensor(rng.standard_normal(n)).float(), o, torch.as_tensor(rng.standard_normal(m)).float(), q)
                for n, o, m, q in ((1, 0, 1, 0), (5, 0, 7, 6), (7, 6, 5, 0), (2 * factor + 1, factor, 3, 1))]
    for h_up, o_up, h_dn, o_dn in designs:
        u = o64.interpolate(x, h_up, factor, o_up)
        want = f64.upfirdn(x.numpy(), h_up.double().numpy(), factor, 1, o_up, factor * L)
        assert u.shape == want.shape and np.abs(u.numpy() - want).max() <= 1e-12 * np.abs(want).max()
        y = o64.decimate(u, h_dn, factor, o_dn)
        want = f64.upfirdn(u.numpy(), h_dn.double().numpy(), 1, factor, o_dn, L)
        assert y.shape == want.shape and np.abs(y.numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_default_filters():
    from grafx_amd.processors import oversampling_filters

    for factor, taps in ((2, 25), (3, 37), (4, 49), (8, 97)):
        h_up, o_up, h_dn, o_dn = oversampling_filters(factor)
        w_up, w_o_up, w_dn, w_o_dn = o64.filters(factor)
        assert h_up.dtype == h_dn.dtype == torch.float64 and h_up.shape == h_dn.shape == (taps,)
        assert (o_up, o_dn) == ((taps - 1) // 2,) * 2 == (w_o_up, w_o_dn)
        assert torch.equal(h_up.float(), w_up) and torch.equal(h_dn.float(), w_dn)
        for ph in range(factor):                                   # unity gain: every phase of the interpolator (a constant
            assert abs(float(h_up[ph::factor].sum()) - 1.0) < 1e-3  # stays one within 0.1 %), and the decimator
        assert abs(float(h_up.sum()) / factor - 1.00047) < 2e-5 and abs(float(h_dn.sum()) - 1.00047) < 2e-5
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError):
            oversampling_filters(bad)


def test_alias_shares_of_the_table():
    share = {f: o64.tone_share(f) for f in SHARES}
    for f, want in SHARES.items():
        assert abs(share[f] - want) <= 0.01 * want, (f, share[f])
    assert share[2] < 0.1 * share[1] and share[4] < 0.01 * share[1] and share[8] < 1e-4 * share[1]


def test_torch_forward_is_the_definition():
    """torch_forward of an oversampled module against the yardstick's own statement, in float64 on the CPU."""
    import grafx_amd.processors as P

    gen = torch.Generator().manual_seed(3)
    x = torch.rand(3, 2, 300, generator=gen, dtype=torch.float64) * 1.1 - 0.55
    w, pre = torch.randn(3, 6, generator=gen, dtype=torch.float64) * 0.5, -torch.rand(3, 1, generator=gen, dtype=torch.float64)
    m = P.ChebyshevDistortion(max_order=6, use_tanh=True, remove_dc=True, oversample=3)
    want = o64.forward(x, o64.CHEBYSHEV, 3, *o64.filters(3), log_pre_gain=pre, p0=w, use_tanh=True, remove_dc=True)
    assert (m.torch_forward(x, w, pre) - want).abs().max() <= 1e-14
    hard, thr = torch.randn(3, 2, generator=gen, dtype=torch.float64) * 0.5, torch.randn(3, 2, generator=gen, dtype=torch.float64) * 0.5
    m = P.PiecewiseTanhDistortion(inverse_post_gain=False, oversample=4)
    want = o64.forward(x, o64.PIECEWISE, 4, *o64.filters(4), log_pre_gain=pre, log_post_gain=-pre, p0=hard, p1=thr)
    assert (m.torch_forward(x, hard, thr, pre, -pre) - want).abs().max() <= 1e-14


@pytest.mark.parametrize("name", CLASSES)
def test_constructors_take_oversample(name):
    import grafx_amd.processors as P

    cls = getattr(P, name)
    for bad in (0, 17, 2.0, -1, True, "4"):
        with pytest.raises(ValueError, match="oversample"):
            cls(oversample=bad)
    plain = cls(oversample=1)
    assert plain.oversample == 1 == cls().oversample and list(plain.buffers()) == [] and plain.state_dict() == {}
    assert plain.parameter_size() == cls(oversample=4).parameter_size()
    plain.stream_check()
    m = cls(oversample=4)
    assert {k: (v.dtype, tuple(v.shape)) for k, v in m.named_buffers()} == {"os_h_up": (torch.float32, (49,)),
                                                                          "os_h_dn": (torch.float32, (49,))}
    assert m.state_dict() == {} and (m.os_offset_up, m.os_offset_dn) == (24, 24)
    with pytest.raises(ValueError, match="oversample=4.*history"):
        m.stream_check()


def test_wrappers_refuse_cpu_tensors_and_bad_filters():
    from grafx_amd import ops

    x, h = torch.zeros(1, 1, 8), torch.ones(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.oversampled_waveshaper(x, ops.WS_TANH, 2, h, 0, h, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.oversampled_waveshaper_bwd(x, x, ops.WS_TANH, 2, h, 0, h, 0)
