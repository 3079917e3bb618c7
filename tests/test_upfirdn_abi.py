"""The polyphase FIR without a GPU: its C entries are declared, bound and exported; the tile constant of the header is the one
ops exports; the workspace query returns the documented size; the entries refuse bad arguments before any launch; the filter
design agrees with the yardstick's own statement; and the yardstick agrees with itself (scipy route against the direct sum,
the adjoint identity in float64)."""
import os
import re

import numpy as np
import pytest
import torch

import upfirdn_float64 as f64
from abi_checks import device_pointer, entries_match, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gfx_upfirdn_f32", "gfx_upfirdn_absmax_ws_bytes", "gfx_upfirdn_absmax_f32")
# orig -> new, taps (the issue's figures), up, down
DESIGNS = ((44100, 48000, 1939, 160, 147), (44100, 16000, 5345, 160, 441), (1, 4, 49, 4, 1), (2, 1, 25, 1, 2),
           (3, 2, 37, 2, 3), (48000, 16000, 37, 1, 3))
# up, down, N, offset, L: the ratios of the issue's adjoint check, short enough for the direct sum
IDENTITIES = ((160, 147, 1939, 969, 300), (1, 2, 25, 12, 101), (4, 1, 49, 24, 50), (160, 441, 5345, 2672, 600), (2, 3, 37, 18, 77),
              (4, 1, 49, 0, 33), (4, 1, 49, 48, 33))


def test_the_entries_are_declared_bound_and_exported():
    from grafx_amd import ops

    header = open(os.path.join(ROOT, "include", "grafx_amd.h")).read()
    assert "gfx_upfirdn_absmax_ws_bytes = R * C * ceil(M / GFX_UPFIRDN_TILE) * 16 bytes" in header
    assert int(re.search(r"#define GFX_UPFIRDN_TILE (\d+)", header).group(1)) == ops.UPFIRDN_TILE
    entries_match(ENTRIES)


def test_workspace_query_returns_the_documented_size():
    from grafx_amd import ops

    T = ops.UPFIRDN_TILE
    for R, C, M in ((1, 1, 1), (1, 1, T), (1, 1, T + 1), (3, 2, 144001), (66000, 1, 256), (256, 2, 524288)):
        assert ops.upfirdn_absmax_ws_bytes(R, C, M) == R * C * -(-M // T) * 16, (R, C, M)
    for bad in ((0, 2, 100), (2, 0, 100), (2, 2, 0), (-1, 2, 100), (2, -2, 100), (2, 2, -100)):
        assert ops.upfirdn_absmax_ws_bytes(*bad) == 0, bad


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every check of the two entries comes before their first launch, so the refusals need no GPU
    (abi_checks.device_pointer)."""
    from grafx_amd import _lib

    lib = _lib.lib()
    R, C, L, M, N = 3, 2, 2000, 2177, 1939
    need = lib.gfx_upfirdn_absmax_ws_bytes(R, C, M)
    assert need == R * C * 3 * 16
    p, _held = device_pointer()
    rm, ym, empty = _lib.RowMap(R, 0, C * L, L), _lib.RowMap(R, 0, C * M, M), _lib.RowMap(0, 0, C * L, L)
    fwd = dict(x=p, xmap=rm, h=p, N=N, up=160, down=147, offset=969, y=p, ymap=ym, R=R, C=C, L=L, M=M, accumulate=0, stream=None)
    peak = dict(x=p, xmap=rm, h=p, N=N, up=160, down=147, offset=969, peak=p, index=p, R=R, C=C, L=L, M=M, ws=p, ws_bytes=need,
                stream=None)
    bad = {
        "no signal": dict(x=None), "no taps": dict(h=None), "an empty row map": dict(xmap=empty),
        "no rows": dict(R=0), "negative rows": dict(R=-3), "no channels": dict(C=0), "negative channels": dict(C=-2),
        "no samples": dict(L=0), "negative length": dict(L=-5), "no outputs": dict(M=0), "negative outputs": dict(M=-1),
        "up = 0": dict(up=0), "up = 1025": dict(up=1025), "down = 0": dict(down=0), "down = 1025": dict(down=1025),
        "negative up": dict(up=-2), "no taps at all": dict(N=0, offset=0), "16385 taps": dict(N=16385),
        "offset = N": dict(offset=N), "offset = -1": dict(offset=-1),
        "more than 2^31 - 1 row-channels": dict(R=1 << 16, C=1 << 15),
    }
    only_fwd = {"no output": dict(y=None), "an empty output row map": dict(ymap=empty)}
    only_peak = {"no peaks": dict(peak=None), "no indices": dict(index=None), "no workspace": dict(ws=None),
                 "a workspace off the 16-byte grid": dict(ws=p + 8), "indices off the 8-byte grid": dict(index=p + 4)}
    refused(lib.gfx_upfirdn_f32, fwd, {**bad, **only_fwd})
    refused(lib.gfx_upfirdn_absmax_f32, peak, {**bad, **only_peak})
    refused(lib.gfx_upfirdn_absmax_f32, peak, {"a workspace one byte short": dict(ws_bytes=need - 1)}, code=-2)


@pytest.mark.parametrize("orig,new,taps,up,down", DESIGNS)
def test_sinc_kernel_agrees_with_the_yardstick(orig, new, taps, up, down):
    from grafx_amd.resample import sinc_kernel

    h, u, d, offset = sinc_kernel(orig, new)
    want, wu, wd, woff = f64.sinc_kernel(orig, new)
    assert (u, d, offset) == (up, down, (taps - 1) // 2) == (wu, wd, woff)
    assert h.dtype == torch.float64 and h.shape == (taps,) == want.shape
    assert np.abs(h.numpy() - want).max() <= 1e-14 * np.abs(want).max()


def test_resample_refuses_a_design_beyond_the_kernel_without_a_gpu():
    from grafx_amd.resample import Resample

    with pytest.raises(ValueError, match=r"44100/44101.*534557 taps"):
        Resample(44100, 44101)
    with pytest.raises(ValueError, match="taps"):
        Resample(1, 1024, lowpass_filter_width=9)        # the ratio fits, 2 * 9309 + 1 taps do not
    assert Resample(44100, 48000).taps.dtype == torch.float32 and Resample(44100, 48000).taps.shape == (1939,)


@pytest.mark.parametrize("up,down,N,offset,L", IDENTITIES)
def test_the_yardstick_agrees_with_itself(up, down, N, offset, L):
    """The scipy route against the direct sum, outputs beyond the default length included, and <upfirdn(x), g> = <x, adjoint(g)>."""
    rng = np.random.default_rng(N + L)
    h, x = rng.standard_normal(N), rng.standard_normal((2, L))
    M = f64.default_n_out(L, N, up, down, offset) + 5
    y = f64.upfirdn(x, h, up, down, offset, M)
    direct = f64.upfirdn_direct(x, h, up, down, offset, range(M))
    assert np.abs(y - direct).max() <= 1e-12 * np.abs(direct).max()
    assert np.count_nonzero(y[:, -5:]) == 0 and np.count_nonzero(direct[:, -5:]) == 0
    g = rng.standard_normal(y.shape)
    lhs, rhs = (y * g).sum(), (x * f64.adjoint(g, h, up, down, offset, L)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.abs(y * g).sum())
