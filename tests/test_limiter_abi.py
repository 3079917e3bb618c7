"""The look-ahead limiter without a GPU: the three C entries are declared, bound and exported with their argument lists;
the workspace query returns the documented size and 0 for bad arguments; every refusal of the entries comes back before
a launch; the float64 yardstick agrees with a brute-force loop and its autograd with the written adjoint; blocks equal one
call exactly; the ceiling holds; a row under the ceiling is the delayed input; ``compensate`` aligns the output; and the
constructor takes what is documented."""
import numpy as np
import pytest
import torch

import limiter_float64 as l64
from abi_checks import device_pointer, entries_match, refused

ENTRIES = ("gfx_limiter_f32", "gfx_limiter_bwd_ws_bytes", "gfx_limiter_bwd_f32")
# D, H, N of the small float64 checks
SMALL = ((4, 3, 4), (0, 0, 1), (7, 0, 3), (5, 9, 6))


def test_the_entries_are_declared_bound_and_exported():
    fwd = ["const float*", "gfx_rowmap_t", "float*", "gfx_rowmap_t", "int64_t", "int64_t", "int64_t", "const float*",
           "const float*", "int64_t", "int64_t", "int64_t", "int64_t", "const float*", "float*", "float*", "void*"]
    bwd = ["const float*", "gfx_rowmap_t", "const float*", "gfx_rowmap_t", "int64_t", "int64_t", "int64_t", "const float*",
           "const float*", "int64_t", "int64_t", "int64_t", "int64_t", "float*", "gfx_rowmap_t", "float*", "void*", "size_t",
           "void*"]
    entries_match(ENTRIES, dict(zip(ENTRIES, (("int", fwd), ("size_t", ["int64_t"] * 4), ("int", bwd)))))


def test_tile_and_workspace_query():
    from grafx_amd import _lib, ops

    assert (ops.LIMITER_MAX_TAPS, ops.LIMITER_MAX_WINDOW) == (1024, 4096)
    assert [ops.limiter_tile(m) for m in (1, 240, 2640, 2795, 2796, 3000, 4096)] == [4096, 4096, 4096, 4096, 3584, 3584, 1024]
    for m in range(1, 4097, 5):      # the backward tile of the largest filter fits the CU's 160 KiB of LDS
        t = ops.limiter_tile(m)
        assert t % 512 == 0 and 12 * (t + 2 * m) + 4 * (t + m) + 4 * min(m, 1024) <= 160 * 1024 - 4096
    for bad in (0, 4097, 2.0, True):
        with pytest.raises(ValueError):
            ops.limiter_tile(bad)
    query = _lib.lib().gfx_limiter_bwd_ws_bytes
    for R, L, D, H in ((1, 1, 0, 0), (3, 4097, 7, 0), (3, 4096, 239, 2400), (70000, 40, 63, 0), (256, 131072, 1023, 3072)):
        assert query(R, L, D, H) == 8 * R * -(-L // ops.limiter_tile(D + 1 + H)), (R, L, D, H)
    for bad in ((0, 100, 7, 0), (-1, 100, 7, 0), (2, 0, 7, 0), (2, 100, -1, 0), (2, 100, 7, -1), (2, 100, 4096, 0),
                (2, 100, 1023, 3073)):
        assert query(*bad) == 0, bad


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every check comes before the first launch, so the refusals need no GPU (abi_checks.device_pointer)."""
    from grafx_amd import _lib

    lib = _lib.lib()
    R, C, L, D, H, N = 3, 2, 2000, 63, 100, 64
    S = D + H + N - 1
    need = lib.gfx_limiter_bwd_ws_bytes(R, L, D, H)
    p, _held = device_pointer()
    far = p + 4 * R * C * L      # a second signal that does not overlap the first, then a third, then two states
    third = far + 4 * R * C * L
    z0, z1 = third + 4 * R * C * L, third + 4 * R * C * L + 4 * R * C * S
    rm, empty, neg = _lib.RowMap(R, 0, C * L, L), _lib.RowMap(0, 0, C * L, L), _lib.RowMap(R, 0, -C * L, L)
    fwd = dict(x=p, xmap=rm, y=far, ymap=rm, R=R, C=C, L=L, log_ceiling=p, w=p, N=N, D=D, H=H, sigma=0, zi=None, zf=None,
               gain=None, stream=None)
    bwd = dict(x=p, xmap=rm, gy=far, gmap=rm, R=R, C=C, L=L, log_ceiling=p, w=p, N=N, D=D, H=H, sigma=0, gx=third, omap=rm,
               g_log_ceiling=p, ws=p, ws_bytes=need, stream=None)
    bad = {
        "no signal": dict(x=None), "an empty row map": dict(xmap=empty), "no rows": dict(R=0), "negative rows": dict(R=-3),
        "no channels": dict(C=0), "no samples": dict(L=0), "negative length": dict(L=-5), "no ceiling": dict(log_ceiling=None),
        "no taps": dict(w=None), "zero taps": dict(N=0), "1025 taps": dict(N=1025, D=2000), "more taps than D + 1": dict(N=D + 2),
        "negative look-ahead": dict(D=-1, N=1), "negative hold": dict(H=-1), "a window of 4097": dict(H=4096 - D),
        "a look-ahead of 4096": dict(D=4096, H=0), "sigma neither 0 nor D": dict(sigma=1), "negative sigma": dict(sigma=-D),
        "more than 2^31 - 1 row-channels": dict(R=1 << 16, C=1 << 15),
        "more than 2^31 - 1 workgroups": dict(R=1 << 20, L=4096 * (1 << 11) + 1),
        "a negative stride": dict(xmap=neg),
    }
    only_fwd = {"no output": dict(y=None), "an empty output row map": dict(ymap=empty), "an output that is the input": dict(y=p),
                "an output that overlaps the input": dict(y=p + 4), "a negative output stride": dict(ymap=neg),
                "a state with sigma = D": dict(sigma=D, zi=z0), "a new state with sigma = D": dict(sigma=D, zf=z1),
                "zf is zi": dict(zi=z0, zf=z0), "zf overlaps zi": dict(zi=z0, zf=z0 + 4 * (R * C * S - 1))}
    only_bwd = {"no output gradient": dict(gy=None), "an empty gradient row map": dict(gmap=empty),
                "nothing asked for": dict(gx=None, g_log_ceiling=None), "gx is x": dict(gx=p), "gx is gy": dict(gx=far),
                "gx overlaps x a sample later": dict(gx=p + 4), "an empty gx row map": dict(omap=empty),
                "a ceiling gradient without a workspace": dict(ws=None), "a workspace that is not 8-byte aligned": dict(ws=p + 4)}
    refused(lib.gfx_limiter_f32, fwd, {**bad, **only_fwd})
    refused(lib.gfx_limiter_bwd_f32, bwd, {**bad, **only_bwd})
    refused(lib.gfx_limiter_bwd_f32, bwd, {"a workspace one byte short": dict(ws_bytes=need - 1)}, code=-2)


def _case(D, H, N, seed, R=2, C=2, L=60):
    x = l64.burst_rows(R, C, L, seed)
    lc = torch.log(torch.tensor([0.25, 0.12][:R] + [0.2] * max(0, R - 2), dtype=torch.float32))
    return x, lc, l64.window(D, N)


@pytest.mark.parametrize("D,H,N", SMALL)
@pytest.mark.parametrize("sigma_is_D", [False, True])
def test_the_yardstick_agrees_with_a_brute_force_loop(D, H, N, sigma_is_D):
    x, lc, w = _case(D, H, N, seed=D + H)
    sigma = D if sigma_is_D else 0
    y, gain, _ = l64.forward(x, lc, w, D, H, sigma)
    by, bgain, _ = l64.brute(x, lc, w, D, H, sigma)
    assert np.abs(y.numpy() - by).max() <= 1e-14 and np.abs(gain.numpy() - bgain).max() <= 1e-14
    assert float(gain.min()) < 0.9      # the burst is limited
    if not sigma_is_D and D + H + N > 1:
        state = torch.randn(2, 2, D + H + N - 1, generator=torch.Generator().manual_seed(1)) * 0.3
        y, gain, zf = l64.forward(x, lc, w, D, H, 0, state)
        by, bgain, _ = l64.brute(x, lc, w, D, H, 0, state)
        assert np.abs(y.numpy() - by).max() <= 1e-14 and np.abs(gain.numpy() - bgain).max() <= 1e-14
        assert torch.equal(zf, torch.cat([state.double(), x.double()], -1)[..., -zf.shape[-1]:])


@pytest.mark.parametrize("D,H,N", SMALL)
@pytest.mark.parametrize("sigma_is_D", [False, True])
def test_autograd_of_the_yardstick_agrees_with_the_written_adjoint(D, H, N, sigma_is_D):
    x, lc, w = _case(D, H, N, seed=10 + D + H)
    sigma = D if sigma_is_D else 0
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    gx, gc = l64.gradients(x, g, lc, w, D, H, sigma)
    wx, wc = l64.adjoint(x, g, lc, w, D, H, sigma)
    assert np.abs(gx.numpy() - wx).max() <= 1e-12 * max(1.0, np.abs(wx).max())
    assert np.abs(gc.numpy() - wc).max() <= 1e-12 * max(1.0, np.abs(wc).max())
    assert np.abs(wc).max() > 0


def test_ties_are_found():
    w = l64.window(4)
    lc = torch.log(torch.tensor([0.5]))
    square = torch.ones(1, 1, 40) * torch.tensor([1.0, -1.0]).repeat(20)
    with pytest.raises(ValueError, match="twice"):
        l64.check_ties(square, lc, w, 4, 3)
    two = l64.burst_rows(1, 2, 40, 3, scale=1.0)
    two[0, 1] = -two[0, 0]
    with pytest.raises(ValueError, match="channels"):
        l64.check_ties(two, lc, w, 4, 3)
    l64.check_ties(square * 0.4, lc, w, 4, 3)          # ties under the ceiling reach no gradient
    l64.check_ties(l64.burst_rows(3, 2, 500, 4, scale=1.0), lc.expand(3), w, 4, 3)


@pytest.mark.parametrize("D,H,N", SMALL)
def test_blocks_equal_one_call_exactly(D, H, N):
    x, lc, w = _case(D, H, N, seed=20, L=60)
    whole, wgain, wz = l64.forward(x, lc, w, D, H)
    ys, gains, state, at = [], [], None, 0
    for n in (7, 1, 20, 32):
        y, gain, state = l64.forward(x[..., at:at + n], lc, w, D, H, 0, state)
        ys.append(y), gains.append(gain)
        at += n
    assert at == 60 and torch.equal(torch.cat(ys, -1), whole) and torch.equal(torch.cat(gains, -1), wgain)
    assert torch.equal(state, wz)


@pytest.mark.parametrize("D,H,N", [(63, 0, 64), (63, 200, 64), (255, 1000, 100), (0, 0, 1), (7, 0, 3)])
@pytest.mark.parametrize("sigma_is_D", [False, True])
def test_the_ceiling_holds_in_float64(D, H, N, sigma_is_D):
    x = l64.burst_rows(3, 2, 3000, D + 1, scale=0.2)
    lc = torch.log(torch.tensor([0.3, 0.1, 5.0]))
    y, gain, _ = l64.forward(x, lc, l64.window(D, N), D, H, D if sigma_is_D else 0)
    # (the taps are float32 values: their sum, which scales the bound, is one within N 2^-25, not exactly)
    total = float(l64.window(D, N).double().sum())
    assert abs(total - 1) <= N * 2.0 ** -25
    ratio = y.abs().amax((1, 2)) / torch.exp(lc.double()) / total
    assert float(ratio[:2].max()) <= 1 + 1e-14 and float(ratio[:2].min()) > 0.5
    # the third row never reaches its ceiling: the delayed input times the taps' sum
    d = 0 if sigma_is_D else D
    want = torch.nn.functional.pad(x[2].double(), (d, 0))[..., :3000] * total
    assert (y[2] - want).abs().max() <= 1e-14


@pytest.mark.parametrize("D,H,N", SMALL)
def test_compensate_aligns_the_output(D, H, N):
    x, lc, w = _case(D, H, N, seed=30)
    x = torch.cat([x, torch.zeros(2, 2, D)], -1)       # (what sigma = D assumes beyond the end, made explicit)
    late, _, _ = l64.forward(x, lc, w, D, H, 0)
    aligned, _, _ = l64.forward(x[..., :60], lc, w, D, H, D)
    assert torch.equal(aligned, late[..., D:D + 60])


def test_constructor_and_window():
    import grafx_amd.processors as P
    from grafx_amd import ops

    m = P.Limiter()
    assert (m.lookahead, m.hold, m.compensate_delay, m.latency, m.state_samples) == (240, 0, True, 0, 480)
    assert m.parameter_size() == {"log_ceiling": 1} and m.state_dict() == {}
    assert {k: (v.dtype, tuple(v.shape)) for k, v in m.named_buffers()} == {"window": (torch.float32, (241,))}
    w = P.limiter_window(240)
    assert w.dtype == torch.float64 and abs(float(w.sum()) - 1) < 1e-15 and torch.equal(w.float(), l64.window(240))
    assert torch.equal(m.window, w.float()) and float((w - w.flip(0)).abs().max()) < 1e-15 and float(w.min()) > 0
    assert torch.equal(P.limiter_window(0), torch.ones(1, dtype=torch.float64))
    for bad in (-1, 1024, 2.0, True):
        with pytest.raises(ValueError):
            P.limiter_window(bad)
    with pytest.raises(ValueError, match="compensate_delay=True.*next block"):
        m.stream_check()
    ok = P.Limiter(lookahead=7, hold=4088, window=[0.25, 0.5, 0.25], compensate_delay=False)
    ok.stream_check()
    assert (ok.latency, ok.state_samples) == (7, 7 + 4088 + 2)
    assert P.Limiter(0, 0, compensate_delay=False).state_samples == 0
    assert P.Limiter(1023, 3072).window.numel() == 1024 == ops.LIMITER_MAX_TAPS
    for kwargs in (dict(lookahead=2, window=[0.25] * 4), dict(lookahead=7, hold=4089), dict(lookahead=4096),
                   dict(lookahead=7, window=[1.5, -0.5]), dict(lookahead=7, window=[0.5, 0.4]), dict(lookahead=7, window=[]),
                   dict(lookahead=7, window=[[1.0]]), dict(lookahead=-1), dict(lookahead=7, hold=-1), dict(lookahead=7.0),
                   dict(lookahead=True), dict(lookahead=2000)):      # (2000: the default window would hold 2001 taps)
        with pytest.raises(ValueError):
            P.Limiter(**kwargs)


@pytest.mark.parametrize("D,H,N", SMALL)
@pytest.mark.parametrize("compensate", [False, True])
def test_torch_forward_is_the_definition(D, H, N, compensate):
    """torch_forward against the yardstick's own statement, in float64 on the CPU; the guarded division leaves no NaN in
    the ceiling gradient of a row that starts with silence (pk = 0)."""
    import grafx_amd.processors as P

    x, lc, w = _case(D, H, N, seed=40)
    x[..., :10] = 0
    m = P.Limiter(D, H, window=w.double() / w.double().sum(), compensate_delay=compensate)
    want, _, wz = l64.forward(x, lc, m.window, D, H, D if compensate else 0)
    lcp = lc.double().reshape(2, 1).requires_grad_(True)
    got = m.torch_forward(x.double(), lcp)
    assert (got - want).abs().max() <= 1e-15
    got.square().sum().backward()
    assert bool(torch.isfinite(lcp.grad).all()) and float(lcp.grad.abs().min()) > 0
    if not compensate and m.state_samples:
        a, za = m.torch_forward(x.double()[..., :25], lcp.detach(), return_state=True)
        b, zb = m.torch_forward(x.double()[..., 25:], lcp.detach(), state=za, return_state=True)
        assert torch.equal(torch.cat([a, b], -1), got.detach()) and torch.equal(zb, wz)


def test_wrappers_refuse_cpu_tensors():
    from grafx_amd import ops

    x, lc, h = torch.zeros(1, 1, 8), torch.zeros(1), torch.ones(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.limiter(x, lc, h, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.limiter_bwd(x, x, lc, h, 0)
