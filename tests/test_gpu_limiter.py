"""The look-ahead limiter on the GPU (csrc/limiter.hip, ops.limiter / limiter_bwd, autograd.LimiterFn, processors.Limiter)
against the float64 yardstick of tests/limiter_float64.py on the same float32 inputs.

Forward (``y`` and ``gain``) and both gradients are held to the project's 1e-5 of the reference's peak.  The ceiling is
held on every case to max|y| <= exp(log_ceiling) (1 + (N + 16) 2^-23), exp taken in float64: the N additions, the taps'
rounding, the division and the product give at most (1 + 2^-24)^(N + 4); the bound is that doubled, plus room for expf.
Streaming is held to equal bits.  Tile edges come from ops.limiter_tile."""
import functools

import pytest
import torch

import limiter_float64 as l64

pytestmark = pytest.mark.gpu

CONFIGS = [(0, 0, 1), (7, 0, 3), (63, 0, 64), (239, 2400, 240), (1023, 3072, 1024)]     # D, H, N
ROWS = [(1, 1), (3, 2), (2, 5)]                                                          # R, C
CEILINGS = (0.25, 0.12, 0.2)     # linear; the inputs' quiet part has standard deviation 0.1, the burst 0.5


def _tile(D, H):
    from grafx_amd import ops

    return ops.limiter_tile(D + 1 + H)


def _lengths(D, H):
    t = _tile(D, H)
    return sorted({n for n in (1, D, D + 1, t - 1, t, t + 1, 2 * t + 3) if n >= 1})


def _ceilings(R):
    return torch.log(torch.tensor(CEILINGS[:R], dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _reference(D, H, N, sigma, R, C, L):
    """(x, log_ceiling, w, g) float32 on the host, and the yardstick's (y, gain, gx, g_log_ceiling): computed once."""
    x = l64.burst_rows(R, C, L, seed=1000 * D + 10 * R + C + L)
    lc, w = _ceilings(R), l64.window(D, N)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(L), dtype=torch.float32)
    y, gain, _ = l64.forward(x, lc, w, D, H, sigma)
    gx, gc = l64.gradients(x, g, lc, w, D, H, sigma)
    return (x, lc, w, g), (y, gain, gx, gc)


def _close(got, want, tol, what):
    err, peak = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
    print(f"{what}: max error {err:.3e}, peak {peak:.3e}, relative {err / max(peak, 1e-300):.3e}")
    assert err <= tol * peak, what


def _float32_autograd_errors(D, H, N, sigma, R, C, L):
    """Max errors (gx, g_log_ceiling) of float32 torch autograd of Limiter.torch_forward against the float64 yardstick on
    the same inputs: what a float32 evaluation of the definition keeps of a gradient that cancels.  The residue of a
    cancellation is a few roundings whose count depends on the library that evaluates the formula (figures in
    test_gradients_against_the_yardstick), so it is taken on the host and on the GPU, and the larger one counts."""
    import grafx_amd.processors as P

    (x, lc, w, g), (_, _, wgx, wgc) = _reference(D, H, N, sigma, R, C, L)
    worst = [0.0, 0.0]
    for device in ("cpu", "cuda"):
        m = P.Limiter(D, H, window=w.double(), compensate_delay=sigma > 0).to(device)
        xr = x.detach().clone().to(device).requires_grad_(True)       # (new leaves: the reference's inputs are shared)
        lr = lc.detach().clone().reshape(R, 1).to(device).requires_grad_(True)
        (m.torch_forward(xr, lr) * g.to(device)).sum().backward()
        errs = (float((xr.grad.double().cpu() - wgx).abs().max()), float((lr.grad.double().cpu().reshape(R) - wgc).abs().max()))
        print(f"float32 torch autograd on {device}: gx {errs[0]:.3e}, g_log_ceiling {errs[1]:.3e}")
        worst = [max(a, b) for a, b in zip(worst, errs)]
    return tuple(worst)


def _close_or_float32(got, want, what, float32_error):
    """1e-5 of the reference's peak; a case that needs more is allowed what float32 torch autograd of the definition is
    itself off float64 there (``float32_error()``, measured on the spot), and no more."""
    err, peak = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
    print(f"{what}: max error {err:.3e}, peak {peak:.3e}, relative {err / max(peak, 1e-300):.3e}")
    if err <= 1e-5 * peak:
        return
    allowed = float32_error()
    print(f"{what}: NEEDS MORE THAN 1e-5: kernel {err:.3e}, float32 torch autograd {allowed:.3e}, reference peak {peak:.3e}")
    assert err <= allowed, what


def _bound(lc, N):
    return torch.exp(lc.double()) * (1 + (N + 16) * 2.0 ** -23)


@pytest.mark.parametrize("sigma_is_D", [False, True])
@pytest.mark.parametrize("D,H,N", CONFIGS)
def test_forward_against_the_yardstick(D, H, N, sigma_is_D):
    from grafx_amd import ops

    for R, C in ROWS:
        for L in _lengths(D, H):
            (x, lc, w, _), (wy, wgain, _, _) = _reference(D, H, N, D if sigma_is_D else 0, R, C, L)
            y, gain = ops.limiter(x.cuda(), lc.cuda(), w.cuda(), D, H, compensate=sigma_is_D, return_gain=True)
            what = f"D={D} H={H} N={N} compensate={sigma_is_D} R={R} C={C} L={L}"
            assert y.shape == (R, C, L) and gain.shape == (R, L)
            _close(y, wy, 1e-5, what + ": y")
            _close(gain, wgain, 1e-5, what + ": gain")
            peak = y.double().abs().amax((1, 2)).cpu()
            print(f"{what}: max|y| / T = {(peak / torch.exp(lc.double())).tolist()}")
            assert bool((peak <= _bound(lc, N)).all()), what + ": the ceiling"
            if L > 3 * (D + H + N):
                assert float(wgain.min()) < 0.9, what + ": the burst is not limited"


@pytest.mark.parametrize("D,H,N", CONFIGS)
def test_ceiling_on_a_square_wave(D, H, N):
    """A row of +-1 at T = 0.5 is all ties: every window's maximum is reached M times.  The output is +-T (times the taps'
    sum) wherever the look-ahead window is inside the signal."""
    from grafx_amd import ops

    L = _tile(D, H) + 37
    x = (torch.ones(L) * torch.tensor([1.0, -1.0]).repeat(L // 2 + 1)[:L]).reshape(1, 1, L).cuda()
    lc = torch.log(torch.tensor([0.5])).cuda()
    for compensate in (False, True):
        y = ops.limiter(x, lc, l64.window(D, N).cuda(), D, H, compensate=compensate)
        peak = float(y.double().abs().max())
        print(f"D={D} H={H} N={N} compensate={compensate}: max|y| / T = {peak / 0.5}")
        assert peak <= float(_bound(lc.cpu(), N)[0]) and peak >= 0.5 * (1 - N * 2.0 ** -23)


@pytest.mark.parametrize("D,H,N", CONFIGS)
def test_rows_under_the_ceiling_are_the_delayed_input(D, H, N):
    from grafx_amd import ops

    L = _tile(D, H) + 5
    x = l64.burst_rows(2, 2, L, 7).cuda()
    lc = torch.log(torch.tensor([100.0, 100.0])).cuda()
    for compensate in (False, True):
        y, gain = ops.limiter(x, lc, l64.window(D, N).cuda(), D, H, compensate=compensate, return_gain=True)
        d = 0 if compensate else D
        want = torch.nn.functional.pad(x, (d, 0))[..., :L]
        assert bool(((y - want).abs() <= N * 2.0 ** -24 * want.abs()).all())
        assert bool(((gain - 1).abs() <= N * 2.0 ** -24).all())


def test_determinism_rows_and_layout():
    """Two runs give equal bits; a row's result does not depend on the other rows; strided (B, n, C, L) views in and out
    match contiguous ones; an ``out`` that overlaps ``x`` is refused."""
    from grafx_amd import ops

    D, H, N = 63, 40, 64
    L = _tile(D, H) + 9
    w = l64.window(D, N).cuda()
    B, n, C = 2, 3, 2
    buf = torch.zeros(B, n + 2, C, L + 8, device="cuda")
    x = l64.burst_rows(B * n, C, L, 11).cuda()
    lc = torch.log(torch.tensor([0.25, 0.12, 0.2, 0.3, 0.15, 0.22])).cuda()
    g = torch.randn(B * n, C, L, generator=torch.Generator().manual_seed(5)).cuda()
    for compensate in (False, True):
        y, gain = ops.limiter(x, lc, w, D, H, compensate=compensate, return_gain=True)
        gx, gc = ops.limiter_bwd(x, g, lc, w, D, H, compensate=compensate)
        y2, gain2 = ops.limiter(x, lc, w, D, H, compensate=compensate, return_gain=True)
        gx2, gc2 = ops.limiter_bwd(x, g, lc, w, D, H, compensate=compensate)
        assert torch.equal(y, y2) and torch.equal(gain, gain2) and torch.equal(gx, gx2) and torch.equal(gc, gc2)
        one = ops.limiter(x[4:5], lc[4:5], w, D, H, compensate=compensate)
        gx1, gc1 = ops.limiter_bwd(x[4:5], g[4:5], lc[4:5], w, D, H, compensate=compensate)
        assert torch.equal(one, y[4:5]) and torch.equal(gx1, gx[4:5]) and torch.equal(gc1, gc[4:5])
        # strided views of a wider buffer, in and out
        buf.zero_()
        xin, out = buf[:, 1:1 + n, :, 3:3 + L], torch.zeros(B, n + 1, C, L + 4, device="cuda")[:, :n, :, 2:2 + L]
        xin.copy_(x.view(B, n, C, L))
        got = ops.limiter(xin, lc, w, D, H, compensate=compensate, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(out.reshape(B * n, C, L), y)
        gin = torch.zeros(B, n + 1, C, L + 4, device="cuda")[:, 1:, :, :L]
        gin.copy_(g.view(B, n, C, L))
        gout = torch.zeros(B, n, C, L + 2, device="cuda")[..., 1:1 + L]
        sx, sc = ops.limiter_bwd(xin, gin, lc, w, D, H, compensate=compensate, out=gout)
        assert torch.equal(sx.reshape(B * n, C, L), gx) and torch.equal(sc, gc)
    with pytest.raises(ValueError, match="share memory"):
        ops.limiter(buf[:, :n, :, :L], lc, w, D, H, out=buf[:, 1:1 + n, :, 1:1 + L])
    with pytest.raises(ValueError, match="share memory"):
        ops.limiter(x, lc, w, D, H, out=x)
    with pytest.raises(ValueError, match="share memory"):
        ops.limiter_bwd(x, g, lc, w, D, H, out=g)
    with pytest.raises(ValueError, match="compensate"):
        ops.limiter(x, lc, w, D, H, compensate=True, return_state=True)
    with pytest.raises(ValueError):
        ops.limiter(x, lc, torch.full((D + 2,), 1.0 / (D + 2), device="cuda"), D, H)     # N > D + 1


def test_seventy_thousand_rows():
    """Rows ride on grid.x: more of them than grid.y holds."""
    from grafx_amd import ops

    R, L, D, H, N = 70000, 40, 7, 2, 8
    x = l64.burst_rows(R, 1, L, 13)
    lc = torch.full((R,), -1.8)
    w = l64.window(D, N)
    g = torch.ones(R, 1, L)
    y, gain = ops.limiter(x.cuda(), lc.cuda(), w.cuda(), D, H, return_gain=True)
    gx, gc = ops.limiter_bwd(x.cuda(), g.cuda(), lc.cuda(), w.cuda(), D, H)
    rows = [0, 1, 65535, 65536, R - 1]
    wy, wgain, _ = l64.forward(x[rows], lc[rows], w, D, H)
    wgx, wgc = l64.gradients(x[rows], g[rows], lc[rows], w, D, H)
    _close(y[rows], wy, 1e-5, "70000 rows: y")
    _close(gain[rows], wgain, 1e-5, "70000 rows: gain")
    _close(gx[rows], wgx, 1e-5, "70000 rows: gx")
    _close(gc[rows], wgc, 1e-5, "70000 rows: g_log_ceiling")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gc).all())


@pytest.mark.parametrize("sigma_is_D", [False, True])
@pytest.mark.parametrize("D,H,N", CONFIGS)
def test_gradients_against_the_yardstick(D, H, N, sigma_is_D):
    """gx and g_log_ceiling against float64 autograd of the definition, 1e-5 of the peak.

    One kind of case needs more: a single sample of a single channel above the ceiling under ``compensate`` (R, C, L =
    1, 1, 1).  Its output is +-T whatever x is, so gx is zero analytically -- the direct term g s and the routed term cancel
    -- and the float64 reference is 5.6e-17 or 0.0: every float32 evaluation keeps a rounding of the two terms.  Measured,
    kernel / float32 torch autograd of torch_forward on the same inputs on two hosts and on the GPU: 3.0e-8 / 8.9e-8,
    3.0e-8 and 5.6e-17 (D = 63), 8.9e-8 / 1.2e-7, 2.4e-7 and 2.4e-7 (D = 239, H = 2400), 1.5e-8 / 7.5e-8, 1.0e-7 and
    6.0e-8 (D = 1023, H = 3072) -- none to eight roundings of a term of size one.  Those cases are held to what float32 autograd is off, measured in the test on the
    host and on the GPU; every other case of this file is within 1e-5 (the ceiling gradient at N = 1024, L = 2051 was
    2.0e-5 off while its partial sums were float32: it is summed in double now, see lim_fir_runs in csrc/limiter.hip)."""
    from grafx_amd import ops

    sigma = D if sigma_is_D else 0
    for R, C in ROWS:
        for L in _lengths(D, H):
            (x, lc, w, g), (_, _, wgx, wgc) = _reference(D, H, N, sigma, R, C, L)
            gx, gc = ops.limiter_bwd(x.cuda(), g.cuda(), lc.cuda(), w.cuda(), D, H, compensate=sigma_is_D)
            what = f"D={D} H={H} N={N} compensate={sigma_is_D} R={R} C={C} L={L}"
            assert gx.shape == (R, C, L) and gc.shape == (R,)
            _close_or_float32(gx, wgx, what + ": gx", lambda: _float32_autograd_errors(D, H, N, sigma, R, C, L)[0])
            _close_or_float32(gc, wgc, what + ": g_log_ceiling", lambda: _float32_autograd_errors(D, H, N, sigma, R, C, L)[1])
            only_x, none = ops.limiter_bwd(x.cuda(), g.cuda(), lc.cuda(), w.cuda(), D, H, compensate=sigma_is_D, want=("x",))
            none_x, only_c = ops.limiter_bwd(x.cuda(), g.cuda(), lc.cuda(), w.cuda(), D, H, compensate=sigma_is_D,
                                             want=("log_ceiling",))
            assert none is None and none_x is None and torch.equal(only_x, gx) and torch.equal(only_c, gc)


def test_ceiling_gradient_of_a_row_that_never_limits_is_zero():
    from grafx_amd import ops

    D, H, N = 63, 0, 64
    L = 2 * _tile(D, H) + 3
    x = l64.burst_rows(2, 2, L, 17).cuda()
    lc = torch.log(torch.tensor([0.2, 100.0])).cuda()
    g = torch.randn(2, 2, L, generator=torch.Generator().manual_seed(6)).cuda()
    for compensate in (False, True):
        gx, gc = ops.limiter_bwd(x, g, lc, l64.window(D, N).cuda(), D, H, compensate=compensate)
        assert float(gc[1]) == 0.0 and float(gc[0]) != 0.0
        d = 0 if compensate else D                       # gx of that row is the advanced gradient times the taps' sum
        want = torch.nn.functional.pad(g[1], (0, d))[..., d:]
        assert bool(((gx[1] - want).abs() <= N * 2.0 ** -24 * want.abs()).all())


@pytest.mark.parametrize("compensate", [False, True])
def test_module_and_node_agree_with_the_op(compensate):
    import grafx_amd.processors as P
    from grafx_amd import ops
    from grafx_amd.autograd import LimiterFn

    D, H = 31, 50
    L = _tile(D, H) + 3
    m = P.Limiter(D, H, compensate_delay=compensate).cuda()
    x = l64.burst_rows(3, 2, L, 19).cuda()
    lc = _ceilings(3).reshape(3, 1).cuda()
    g = torch.randn(3, 2, L, generator=torch.Generator().manual_seed(7)).cuda()
    wy = ops.limiter(x, lc, m.window, D, H, compensate=compensate)
    wgx, wgc = ops.limiter_bwd(x, g, lc, m.window, D, H, compensate=compensate)
    assert torch.equal(m(x, lc), wy)
    for run in (lambda a, b: m(a, b), lambda a, b: LimiterFn.apply(a, b, m.window, D, H, compensate)):
        xr, lr = x.clone().requires_grad_(True), lc.clone().requires_grad_(True)
        y = run(xr, lr)
        assert torch.equal(y.detach(), wy)
        y.backward(g)
        assert torch.equal(xr.grad, wgx) and lr.grad.shape == (3, 1) and torch.equal(lr.grad.reshape(3), wgc)
    lr = lc.clone().requires_grad_(True)                  # the ceiling alone
    m(x, lr).backward(g)
    assert torch.equal(lr.grad.reshape(3), wgc)
    # the module's own torch formula, float32 on the GPU, agrees with the kernel
    _close(m.torch_forward(x, lc), wy.double().cpu(), 1e-5, "torch_forward")
    with pytest.raises(ValueError, match="taps get no gradient"):
        LimiterFn.apply(x, lc, m.window.clone().requires_grad_(True), D, H, compensate)


def _cuts(total, S, tile):
    cuts = [1, 7, S, tile + 1]
    return cuts + [total - sum(cuts)]


@pytest.mark.parametrize("D,H,N", [(7, 0, 3), (63, 0, 64), (239, 2400, 240)])
def test_blocks_equal_one_call_in_bits(D, H, N):
    """Blocks of 1, 7, M + N - 2, tile + 1 and the rest, through ops.limiter, Limiter.forward(state=) and stream_block:
    outputs, gains and states equal the one-call results bit for bit."""
    import grafx_amd.processors as P
    from grafx_amd import ops

    S, tile = D + H + N - 1, _tile(D, H)
    L = 1 + 7 + S + tile + 1 + 300
    R, C = 2, 2
    x = l64.burst_rows(R, C, L, 23).cuda()
    lc, w = _ceilings(R).cuda(), l64.window(D, N).cuda()
    whole, zw, gw = ops.limiter(x, lc, w, D, H, return_state=True, return_gain=True)
    assert torch.equal(whole, ops.limiter(x, lc, w, D, H)) and zw.shape == (R, C, S)
    assert torch.equal(zw, x[..., L - S:])
    m = P.Limiter(D, H, window=w.double().cpu(), compensate_delay=False).cuda()
    assert torch.equal(m.window, w)
    x4, out4 = x.view(1, R, C, L), torch.zeros(1, R, C, L, device="cuda")
    ys, gains, fs, state, fstate, carry, at = [], [], [], None, None, None, 0
    for n in _cuts(L, S, tile):
        y, state, gain = ops.limiter(x[..., at:at + n], lc, w, D, H, state=state, return_state=True, return_gain=True)
        f, fstate = m(x[..., at:at + n], lc.reshape(R, 1), state=fstate, return_state=True)
        carry = m.stream_block(x4[..., at:at + n], out4[..., at:at + n], carry, log_ceiling=lc.reshape(R, 1))
        ys.append(y), gains.append(gain), fs.append(f)
        assert torch.equal(state, fstate) and torch.equal(state, carry)
        at += n
    assert at == L
    assert torch.equal(torch.cat(ys, -1), whole) and torch.equal(torch.cat(gains, -1), gw) and torch.equal(torch.cat(fs, -1), whole)
    assert torch.equal(out4[0], whole) and torch.equal(state, zw)
    zeros = m.stream_silence(carry)
    assert torch.equal(zeros, torch.zeros_like(carry))
    first = ops.limiter(x[..., :50], lc, w, D, H, state=zeros, return_state=True)[0]
    assert torch.equal(first, whole[..., :50])          # zeros mean "nothing came before"


def test_blocks_with_a_two_chunk_state_from_strided_views():
    """The state copy runs on one workgroup per 1024 state samples (launch_history_tail, csrc/common.hip): D, H, N = 1023,
    500, 64 keep S = 1586 of them, two chunks, the second partial and no multiple of 256.  Blocks of 300 (shorter than S,
    entering without a state), 300 (shorter, entering with one: the old state shifts) and 3000 (longer), read as strided
    (B, n, C, L) views of a wider buffer: outputs and every state equal the one-call results bit for bit."""
    from grafx_amd import ops

    D, H, N = 1023, 500, 64
    S, B, n, C = D + H + N - 1, 1, 3, 2
    cuts = [300, 300, 3000]
    L = sum(cuts)
    x = l64.burst_rows(B * n, C, L, 29).cuda()
    lc, w = _ceilings(B * n).cuda(), l64.window(D, N).cuda()
    xin = torch.zeros(B, n + 2, C, L + 8, device="cuda")[:, 1:1 + n, :, 3:3 + L]
    xin.copy_(x.view(B, n, C, L))
    whole, zw = ops.limiter(x, lc, w, D, H, return_state=True)
    assert zw.shape == (B * n, C, S) and torch.equal(zw, x[..., L - S:])
    ys, state, at = [], None, 0
    for m in cuts:
        y, state = ops.limiter(xin[..., at:at + m], lc, w, D, H, state=state, return_state=True)
        at += m
        assert torch.equal(state, ops.limiter(x[..., :at], lc, w, D, H, return_state=True)[1]), at
        ys.append(y.reshape(B * n, C, m))
    assert torch.equal(torch.cat(ys, -1), whole) and torch.equal(state, zw)


def test_streaming_refusals_and_the_memoryless_module():
    import grafx_amd.processors as P

    x = l64.burst_rows(2, 2, 100, 29).cuda()
    lc = _ceilings(2).reshape(2, 1).cuda()
    m = P.Limiter(15, 0, compensate_delay=True).cuda()
    with pytest.raises(ValueError, match="compensate_delay=True.*next block"):
        m.stream_check()
    with pytest.raises(ValueError, match="compensate_delay=True"):
        m(x, lc, return_state=True)
    with pytest.raises(ValueError, match="compensate_delay=True"):
        m.stream_block(x.view(1, 2, 2, 100), torch.zeros(1, 2, 2, 100, device="cuda"), None, log_ceiling=lc)
    plain = P.Limiter(0, 0, compensate_delay=False).cuda()
    out4 = torch.zeros(1, 2, 2, 100, device="cuda")
    assert plain.stream_block(x.view(1, 2, 2, 100), out4, None, log_ceiling=lc) is None
    y, state = plain(x, lc, return_state=True)
    assert state is None and torch.equal(out4[0], y) and torch.equal(y, plain(x, lc))
    want = torch.where(x.abs().amax(1, keepdim=True) > torch.exp(lc)[:, :, None],
                       x * torch.exp(lc)[:, :, None] / x.abs().amax(1, keepdim=True), x)
    assert (y - want).abs().max() <= 1e-6
    with pytest.raises(ValueError, match="no memory"):
        plain(x, lc, state=torch.zeros(2, 2, 0, device="cuda"))
    bad = P.Limiter(15, 0, compensate_delay=False).cuda()
    with pytest.raises(ValueError, match="state must be a contiguous float32 GPU tensor"):
        bad(x, lc, state=torch.zeros(2, 2, 5, device="cuda"))


def _render_setup(D, H, L, seed):
    import grafx_amd.processors as P
    from test_gpu_render_state import _chain_graph, _parameters, _render_data

    procs = {"limiter": P.Limiter(D, H, compensate_delay=False).cuda()}
    G = _chain_graph(["in", "limiter", "out"])
    params = _parameters(procs, G, seed)
    params["limiter"]["log_ceiling"] = torch.full_like(params["limiter"]["log_ceiling"], -1.6)
    x = l64.burst_rows(2, 2, L, seed).view(2, 1, 2, L).cuda()
    return procs, x, params, _render_data(G)


def test_render_node_stream_and_captured_stream():
    """input -> Limiter -> output through render_grafx equals forward(); streamed with state= in blocks of 512 it equals
    the one-block-at-a-time eager output and the one call; through CapturedStream the blocks are bit-identical."""
    from grafx_amd.render import CapturedStream, render_grafx, silent_state

    D, H, n, blocks = 239, 100, 512, 5
    procs, x, params, rd = _render_setup(D, H, n * blocks, 31)
    m = procs["limiter"]
    lc = torch.full((2, 1), -1.6, device="cuda")
    with torch.no_grad():
        want = m(x[:, 0], lc).unsqueeze(1)               # the render's output keeps the node dimension: (B, 1, C, L)
        y, _, _ = render_grafx(procs, x, params, rd)
        y = y.reshape(want.shape)
        assert float(want.abs().max()) <= 0.2021 and torch.equal(y, want)
        ys, state = [], None
        for k in range(blocks):
            yk, _, _, state = render_grafx(procs, x[..., k * n:(k + 1) * n], params, rd, state=state, return_state=True)
            ys.append(yk.clone())
        assert torch.equal(torch.cat(ys, -1).reshape(want.shape), want)
        eager, state = [], silent_state(procs, x[..., :n], params, rd)
        for k in range(blocks):
            yk, _, _, state = render_grafx(procs, x[..., k * n:(k + 1) * n], params, rd, state=state, return_state=True)
            eager.append(yk.clone())
        assert torch.equal(torch.cat(eager, -1).reshape(want.shape), want)
    stream = CapturedStream(procs, x[..., :n], params, rd)
    for k in range(blocks):
        yk, _, _ = stream(x[..., k * n:(k + 1) * n])
        assert torch.equal(yk, eager[k]), f"block {k}"
    aligned = {"limiter": type(m)(D, H).cuda()}          # compensate_delay=True: not a stream
    with pytest.raises(ValueError, match="compensate_delay=True"):
        render_grafx(aligned, x[..., :n], params, rd, state=None, return_state=True)


def test_render_trains_the_ceiling():
    """The node under autograd inside render_grafx: the gradients of the input and the ceiling are those of the op."""
    from grafx_amd import ops
    from grafx_amd.render import render_grafx

    D, H, L = 63, 0, 1500
    procs, x, params, rd = _render_setup(D, H, L, 37)
    m = procs["limiter"]
    p = params["limiter"]["log_ceiling"].clone().requires_grad_(True)
    g = torch.randn(2, 2, L, generator=torch.Generator().manual_seed(8)).cuda()
    y, _, _ = render_grafx(procs, x, {"limiter": {"log_ceiling": p}}, rd)
    y.backward(g.view(y.shape))
    lc = torch.full((2,), -1.6, device="cuda")
    _, wgc = ops.limiter_bwd(x[:, 0], g, lc, m.window, D, H)
    assert p.grad is not None and abs(float(p.grad.sum()) - float(wgc.sum())) <= 1e-5 * float(wgc.abs().sum())
