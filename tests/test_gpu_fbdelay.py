"""The feedback delay on the GPU (csrc/fbdelay.hip, ops.fbdelay / fbdelay_bwd, autograd.FeedbackDelayFn,
processors.FeedbackDelay) against the float64 yardstick of tests/fbdelay_float64.py on the same float32 inputs.

The forward is held to 1e-5 of every row's own peak (conftest.assert_close_rows), every gradient to 1e-5 of its tensor's
peak; a case that needs more is allowed what float32 torch (processors.fbdelay.fbdelay_torch and its autograd) is itself
off float64 on the same inputs, measured on the spot on the host and on the GPU, and no more (the policy of
test_gpu_moddelay._close_or_float32).  For scale: a float32 per-sample loop of the definition on the
host is 1.4e-7 of the peak off float64 at fb = 0.95, delay = 64, L = 700.  Determinism, row independence, layouts and a
delay longer than the signal are held to equal bits; streamed blocks to the forward's tolerance (the walk restarts at
each block) and, for one sequence of calls run twice, to equal bits."""
import functools

import pytest
import torch

import fbdelay_float64 as f64
from conftest import assert_close_rows, rel_err_rows

pytestmark = pytest.mark.gpu

ROWS = [(1, 1), (3, 2), (5, 2)]                                                          # R, C
DELAYS = [128, 4096, 65536]
NAMES = f64.NAMES


def _lengths(Dmax, R):
    from grafx_amd import ops

    K = ops.FBDELAY_CHUNK
    ls = [1, 63, 64, 65, K, K + 1, 2 * K + K // 2 + 5]
    return ls + [Dmax + 200] if Dmax == 65536 and R == 3 else ls                         # (one echo of the long line arrives)


def _cuda(ts):
    return tuple(t.cuda() for t in ts)


@functools.lru_cache(maxsize=None)
def _reference(Dmax, R, C, L):
    """(x, params, g) float32 on the host, and the yardstick's y and six gradients from one float64 graph: computed once."""
    x = f64.bright_rows(R, C, L, seed=10 * R + C + L)
    params = f64.draw_parameters(R, C, Dmax, seed=Dmax + R + C)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(L), dtype=torch.float32)
    leaves = [t.double().clone().requires_grad_(True) for t in (x, *params)]
    y, _ = f64.forward(*leaves, Dmax)
    (y * g.double()).sum().backward()
    return (x, params, g), (y.detach(), f64.leaf_gradients(leaves))


def _float32_errors(x, params, g, wy, want, Dmax, state=None):
    """What float32 torch is off float64 on the same inputs: the forward's worst row (relative to the row's peak) and the
    max errors of the six gradients, on the host and on the GPU; the larger one counts."""
    from grafx_amd.processors.fbdelay import fbdelay_torch

    worst_y, worst = 0.0, [0.0] * 6
    for device in ("cpu", "cuda"):
        leaves = [t.detach().clone().to(device).requires_grad_(g is not None) for t in (x, *params)]
        y = fbdelay_torch(*leaves, Dmax, None if state is None else tuple(s.to(device) for s in state))[0]
        ey = rel_err_rows(y, wy)[0]
        print(f"float32 torch on {device}: y {ey:.3e} of the row's peak")
        worst_y = max(worst_y, ey)
        if g is not None:
            (y * g.to(device)).sum().backward()
            errs = [float((gl.double().cpu() - w).abs().max()) for gl, w in zip(f64.leaf_gradients(leaves), want)]
            print(f"float32 torch autograd on {device}: " + ", ".join(f"g_{n} {e:.3e}" for n, e in zip(NAMES, errs)))
            worst = [max(a, b) for a, b in zip(worst, errs)]
    return worst_y, worst


def _rows_close_or_float32(y, wy, what, float32_error):
    """assert_close_rows at 1e-5; a case that needs more is allowed the worst row of float32 torch, and no more."""
    peak, _ = rel_err_rows(y, wy)
    print(f"{what}: worst row {peak:.3e} of its peak")
    if peak <= 1e-5:
        return assert_close_rows(y, wy, 1e-5, what)
    allowed = float32_error()
    print(f"{what}: NEEDS MORE THAN 1e-5: kernel {peak:.3e}, float32 torch {allowed:.3e}")
    assert peak <= allowed, what


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


def _strided(t, B, n):
    """The rows of a contiguous (B n, C, L) tensor as a strided (B, n, C, L) view of a wider buffer."""
    C, L = t.shape[-2:]
    view = torch.zeros(B, n + 2, C, L + 8, device=t.device)[:, 1:1 + n, :, 3:3 + L]
    view.copy_(t.view(B, n, C, L))
    return view


@pytest.mark.parametrize("Dmax", DELAYS)
def test_forward_against_the_yardstick(Dmax):
    from grafx_amd import ops

    for R, C in ROWS:
        for L in _lengths(Dmax, R):
            (x, params, _), (wy, _) = _reference(Dmax, R, C, L)
            xg, pg = x.cuda(), _cuda(params)
            y = ops.fbdelay(xg, *pg, Dmax)
            what = f"Dmax={Dmax} R={R} C={C} L={L}"
            assert y.shape == (R, C, L)
            _rows_close_or_float32(y, wy, what, lambda: _float32_errors(x, params, None, wy, None, Dmax)[0])
            out = _strided(torch.zeros_like(xg), 1, R)
            got = ops.fbdelay(_strided(xg, 1, R), *pg, Dmax, out=out)
            assert got.data_ptr() == out.data_ptr() and torch.equal(out.reshape(R, C, L), y), what + ": strided views"


def test_chunk_lengths_around_one_wave():
    """The walk's chunk is min(floor(delay)) samples: up to 256 one wave holds it and the cross-wave exchange is skipped,
    above that two to four waves share it, the last one partly filled.  Rows at 256, 257, 700 and 1023 / 1024 samples,
    forward and every gradient."""
    from grafx_amd import ops

    R, C, Dmax = 4, 2, 4096
    L = 2 * ops.FBDELAY_CHUNK + 517
    x = f64.bright_rows(R, C, L, 51)
    _, a, F, dry, wet = f64.draw_parameters(R, C, Dmax, 52)
    delay = torch.tensor([[256.0, 300.5], [257.0, 257.5], [700.25, 1024.0], [1023.5, 1025.0]])
    params = (delay, a, F, dry, wet)
    g = torch.randn(R, C, L, generator=torch.Generator().manual_seed(53))
    leaves = [t.double().clone().requires_grad_(True) for t in (x, *params)]
    wy, _ = f64.forward(*leaves, Dmax)
    (wy * g.double()).sum().backward()
    wy, want = wy.detach(), f64.leaf_gradients(leaves)
    y, (q, w) = ops.fbdelay(x.cuda(), *_cuda(params), Dmax, tape=True)
    allowed = functools.lru_cache(maxsize=None)(lambda: _float32_errors(x, params, g, wy, want, Dmax))
    _rows_close_or_float32(y, wy, "chunks of 256, 257, 700, 1023", lambda: allowed()[0])
    got = ops.fbdelay_bwd(x.cuda(), g.cuda(), q, w, *_cuda(params), Dmax)
    for k, name in enumerate(NAMES):
        _close_or_float32(got[k], want[k], f"chunks of 256, 257, 700, 1023: g_{name}", lambda k=k: allowed()[1][k])


def test_more_rows_than_compute_units():
    """Rows ride on grid.x, one workgroup each: 1030 of them.  Three are checked against the yardstick, all are finite."""
    from grafx_amd import ops

    R, L, Dmax = 1030, 200, 128
    x = torch.randn(R, 1, L, generator=torch.Generator().manual_seed(13))
    one = f64.draw_parameters(6, 1, Dmax, 14)
    params = tuple(p[torch.arange(R) % 6].contiguous() for p in one)
    g = torch.ones(R, 1, L)
    y, (q, w) = ops.fbdelay(x.cuda(), *_cuda(params), Dmax, tape=True)
    got = ops.fbdelay_bwd(x.cuda(), g.cuda(), q, w, *_cuda(params), Dmax)
    rows = [0, 517, R - 1]
    sub = tuple(p[rows] for p in params)
    wy, _ = f64.forward(x[rows], *sub, Dmax)
    assert_close_rows(y[rows], wy, 1e-5, "1030 rows: y")
    for name, a, wg in zip(NAMES, got, f64.gradients(x[rows], g[rows], *sub, Dmax)):
        _close_or_float32(a[rows], wg, f"1030 rows: g_{name}", lambda: 0.0)
        assert bool(torch.isfinite(a).all())
    assert bool(torch.isfinite(y).all())


def test_a_delay_longer_than_the_signal_leaves_the_dry_signal_to_the_bit():
    from grafx_amd import ops

    R, C, L, Dmax = 3, 2, 1500, 4096
    x = f64.bright_rows(R, C, L, 5).cuda()
    _, a, F, dry, wet = _cuda(f64.draw_parameters(R, C, Dmax, 6))
    delay = torch.tensor([[1500.0, 4096.0], [1500.5, 2000.25], [4095.75, 1501.0]]).cuda()
    y, (zf, ql), (q, w) = ops.fbdelay(x, delay, a, F, dry, wet, Dmax, return_state=True, tape=True)
    assert torch.equal(y, dry.reshape(R, 1, 1) * x) and not bool(q.any()) and torch.equal(w, x) and not bool(ql.any())
    assert torch.equal(zf[..., -L:], x) and not bool(zf[..., :-L].any())


def test_determinism_rows_and_layout():
    """Two runs give equal bits, forward and backward; a row's result does not depend on the other rows; strided
    (B, n, C, L) views in and out match contiguous ones; ``want`` subsets give the same bits; an ``out`` that overlaps an
    input is refused."""
    from grafx_amd import ops

    Dmax, B, n, C = 441, 2, 3, 2
    L = 2 * ops.FBDELAY_CHUNK + 77
    x = f64.bright_rows(B * n, C, L, 11).cuda()
    params = _cuda(f64.draw_parameters(B * n, C, Dmax, 12))
    g = torch.randn(B * n, C, L, generator=torch.Generator().manual_seed(5)).cuda()

    def both(xx, gg, pp, **kw):
        y, (q, w) = ops.fbdelay(xx, *pp, Dmax, tape=True)
        return y, ops.fbdelay_bwd(xx, gg, q, w, *pp, Dmax, **kw), (q, w)

    y, grads, (q, w) = both(x, g, params)
    y2, grads2, _ = both(x, g, params)
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert torch.equal(y, ops.fbdelay(x, *params, Dmax))              # (the tape changes nothing)
    for r in (0, 4):
        one = tuple(p[r:r + 1] for p in params)
        y1, g1, _ = both(x[r:r + 1], g[r:r + 1], one)
        assert torch.equal(y1, y[r:r + 1])
        for a, b in zip(g1, grads):
            assert torch.equal(a, b[r:r + 1])
    xin, gin = _strided(x, B, n), _strided(g, B, n)
    gout = torch.zeros(B, n, C, L + 2, device="cuda")[..., 1:1 + L]
    sgrads = ops.fbdelay_bwd(xin, gin, q, w, *params, Dmax, out=gout)
    assert sgrads[0].data_ptr() == gout.data_ptr() and torch.equal(gout.reshape(B * n, C, L), grads[0])
    assert all(torch.equal(a, b) for a, b in zip(sgrads[1:], grads[1:]))
    ws = torch.empty(ops.lib().gfx_fbdelay_bwd_ws_bytes(B * n, C, L) + 8, dtype=torch.uint8, device="cuda")
    assert all(torch.equal(a, b) for a, b in zip(ops.fbdelay_bwd(x, g, q, w, *params, Dmax, ws=ws[:-8]), grads))
    for subset in (("x",), ("delay", "wet"), ("damping", "feedback", "dry"), ("dry", "wet")):
        part = ops.fbdelay_bwd(x, g, q, w, *params, Dmax, want=subset)
        for name, a, b in zip(NAMES, part, grads):
            assert (a is None) if name not in subset else torch.equal(a, b), f"want={subset}: {name}"
    with pytest.raises(ValueError, match="share memory"):
        ops.fbdelay(x, *params, Dmax, out=x)
    with pytest.raises(ValueError, match="share memory"):
        ops.fbdelay_bwd(x, g, q, w, *params, Dmax, out=g)
    with pytest.raises(ValueError, match="history must be a contiguous float32 GPU tensor"):
        ops.fbdelay(x, *params, Dmax, state=(torch.zeros(B * n, C, Dmax, device="cuda"), torch.zeros(B * n, C, device="cuda")))
    with pytest.raises(ValueError, match="q_last must be a contiguous float32 GPU tensor"):
        ops.fbdelay(x, *params, Dmax, state=(torch.zeros(B * n, C, Dmax + 1, device="cuda"), torch.zeros(B * n, device="cuda")))


@pytest.mark.parametrize("Dmax", DELAYS)
def test_gradients_against_the_yardstick(Dmax):
    """All six gradients against float64 autograd of the definition."""
    from grafx_amd import ops

    for R, C in ROWS:
        for L in _lengths(Dmax, R):
            (x, params, g), (wy, want) = _reference(Dmax, R, C, L)
            xg, pg, gg = x.cuda(), _cuda(params), g.cuda()
            _, (q, w) = ops.fbdelay(xg, *pg, Dmax, tape=True)
            got = ops.fbdelay_bwd(xg, gg, q, w, *pg, Dmax)
            what = f"Dmax={Dmax} R={R} C={C} L={L}"
            assert [tuple(t.shape) for t in got] == [tuple(t.shape) for t in want]
            allowed = functools.lru_cache(maxsize=None)(lambda: _float32_errors(x, params, g, wy, want, Dmax)[1])
            for k, name in enumerate(NAMES):
                _close_or_float32(got[k], want[k], f"{what}: g_{name}", lambda k=k: allowed()[k])


@pytest.mark.parametrize("channel", ["stereo", "mono"])
def test_module_and_node_agree_with_the_op(channel):
    """FeedbackDelay(...)(x, **z) is ops.fbdelay on physical(**z); under requires_grad it runs FeedbackDelayFn, whose
    gradients in x and the z parameters match float64 autograd of torch_forward under the policy of this file."""
    import grafx_amd.processors as P
    from grafx_amd import ops
    from grafx_amd.autograd import FeedbackDelayFn

    Dmax, R = 128, 3                                     # (short delays: float32 rounding of the mapping moves them least)
    m = P.FeedbackDelay(64, Dmax, processor_channel=channel).cuda()
    C, L = m.num_channels, ops.FBDELAY_CHUNK + 300
    gen = torch.Generator().manual_seed(19)
    z = {k: torch.randn(R, n, generator=gen) * (0.3 if k.startswith("log") else 1.0) for k, n in m.parameter_size().items()}
    x = f64.bright_rows(R, C, L, 20)
    g = torch.randn(R, C, L, generator=torch.Generator().manual_seed(7))
    xg, zg, gg = x.cuda(), {k: v.cuda() for k, v in z.items()}, g.cuda()
    params = m.physical(**zg)
    wy, (q, w) = ops.fbdelay(xg, *params, Dmax, tape=True)
    wgrads = ops.fbdelay_bwd(xg, gg, q, w, *params, Dmax)
    assert torch.equal(m(xg, **zg), wy)
    leaves = [xg.clone().requires_grad_(True), *(p.clone().requires_grad_(True) for p in params)]
    y = FeedbackDelayFn.apply(*leaves, Dmax)
    assert torch.equal(y.detach(), wy)
    y.backward(gg)
    assert all(torch.equal(t.grad, wg.reshape(t.shape)) for t, wg in zip(leaves, wgrads))
    only = params[1].clone().requires_grad_(True)        # the damping alone: the node asks for nothing else
    FeedbackDelayFn.apply(xg, params[0], only, *params[2:], Dmax).backward(gg)
    assert torch.equal(only.grad, wgrads[2])
    # the module under autograd against float64 autograd of its own torch formula
    xl, zl = xg.clone().requires_grad_(True), {k: v.clone().requires_grad_(True) for k, v in zg.items()}
    y = m(xl, **zl)
    assert torch.equal(y.detach(), wy) and type(y.grad_fn).__name__.startswith("FeedbackDelayFn")
    y.backward(gg)

    def torch_grads(dtype, device):
        xs = x.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
        zs = {k: v.detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k, v in z.items()}
        (m.torch_forward(xs, **zs) * g.to(device=device, dtype=dtype)).sum().backward()
        return [t.grad.double().cpu() for t in (xs, *zs.values())]

    want = torch_grads(torch.float64, "cpu")
    allowed = functools.lru_cache(maxsize=None)(lambda: [max(float((a - wg).abs().max()), float((b - wg).abs().max())) for a, b, wg in
                                                         zip(torch_grads(torch.float32, "cpu"), torch_grads(torch.float32, "cuda"), want)])
    for k, (name, leaf) in enumerate([("x", xl), *zl.items()]):
        _close_or_float32(leaf.grad, want[k], f"module ({channel}): g_{name}", lambda k=k: allowed()[k])
    with pytest.raises(ValueError, match="no native backward"):
        m(xl, **zg, state=m(xg, **zg, return_state=True)[1])
    y, (hist, ql) = m(xl, **zg, return_state=True)       # return_state alone under autograd: (y, state_after)
    _, (whist, wql) = m(xg, **zg, return_state=True)
    assert torch.equal(hist, whist) and torch.equal(ql, wql) and torch.equal(y.detach(), wy)


@pytest.mark.parametrize("Dmax,C", [(128, 2), (4096, 2), (4096, 1)])
def test_blocks_against_the_one_call(Dmax, C):
    """Blocks cut at 1, K - 1, K, inside a chunk and beyond max_delay through ops.fbdelay(state=), FeedbackDelay.forward
    (state=) and stream_block, the first entering with a random state: the output against the one call and against float64
    to the forward's tolerance, the states relative to the history's peak; state tensors that the caller updates in place
    serve as well; and the same sequence of calls gives the same bits."""
    import grafx_amd.processors as P
    from grafx_amd import ops

    R, S, K = 3, Dmax + 1, ops.FBDELAY_CHUNK
    cuts = [1, K - 1, K, 300, S + 5]
    L = sum(cuts)
    x = f64.bright_rows(R, C, L, 24)
    params = f64.draw_parameters(R, C, Dmax, 25)
    gen = torch.Generator().manual_seed(26)
    enter = (torch.randn(R, C, S, generator=gen), torch.randn(R, C, generator=gen))
    wy, (wz, wq) = f64.forward(x, *params, Dmax, enter)
    xg, pg, eg = x.cuda(), _cuda(params), _cuda(enter)
    allowed = functools.lru_cache(maxsize=None)(lambda: _float32_errors(x, params, None, wy, None, Dmax, enter)[0])
    whole, (zw, qw) = ops.fbdelay(xg, *pg, Dmax, state=eg)
    _rows_close_or_float32(whole, wy, f"Dmax={Dmax} C={C}: one call with a state", allowed)
    hpeak = float(wz.abs().max())

    def state_close(state, what):
        ez = float((state[0].double().cpu() - wz).abs().max()) / hpeak
        eq = float((state[1].double().cpu() - wq).abs().max()) / float(wq.abs().max())
        print(f"{what}: history {ez:.3e} of its peak, q_last {eq:.3e}")
        assert max(ez, eq) <= (1e-5 if max(ez, eq) <= 1e-5 else allowed()), what

    state_close((zw, qw), "one call")

    def run():
        ys, state, at = [], eg, 0
        for n in cuts:
            y, state = ops.fbdelay(xg[..., at:at + n], *pg, Dmax, state=state)
            ys.append(y)
            at += n
        return torch.cat(ys, -1), state

    blocks, state = run()
    again, state2 = run()
    assert torch.equal(blocks, again) and torch.equal(state[0], state2[0]) and torch.equal(state[1], state2[1])
    _rows_close_or_float32(blocks, wy, f"Dmax={Dmax} C={C}: blocks against float64", allowed)
    _rows_close_or_float32(blocks, whole.double().cpu(), f"Dmax={Dmax} C={C}: blocks against the one call", allowed)
    state_close(state, "blocks")
    # the caller's own state tensors, overwritten after every block
    held, ys, at = (eg[0].clone(), eg[1].clone()), [], 0
    for n in cuts:
        y, new = ops.fbdelay(xg[..., at:at + n], *pg, Dmax, state=held)
        held[0].copy_(new[0]), held[1].copy_(new[1])
        ys.append(y)
        at += n
    assert torch.equal(torch.cat(ys, -1), blocks) and torch.equal(held[0], state[0]) and torch.equal(held[1], state[1])
    # the module: forward(state=) and stream_block are the op
    m = P.FeedbackDelay(64, Dmax, processor_channel="stereo" if C == 2 else "mono").cuda()
    gz = torch.Generator().manual_seed(27)
    z = {k: torch.randn(R, n, generator=gz).cuda() for k, n in m.parameter_size().items()}
    phys = m.physical(**z)
    x4, out4 = xg.view(1, R, C, L), torch.zeros(1, R, C, L, device="cuda")
    fs, ostate, fstate, carry, at = [], None, None, None, 0
    for n in cuts:
        y, ostate = ops.fbdelay(xg[..., at:at + n], *phys, Dmax, state=ostate, return_state=True)
        f, fstate = m(xg[..., at:at + n], **z, state=fstate, return_state=True)
        carry = m.stream_block(x4[..., at:at + n], out4[..., at:at + n], carry, **z)
        assert torch.equal(f, y) and torch.equal(out4[0, ..., at:at + n], y)
        for other in (fstate, carry):
            assert torch.equal(ostate[0], other[0]) and torch.equal(ostate[1], other[1])
        at += n
    zeros = m.stream_silence(carry)
    assert not bool(zeros[0].any()) and not bool(zeros[1].any())
    first = ops.fbdelay(xg[..., :50], *phys, Dmax, state=zeros)[0]
    assert torch.equal(first, ops.fbdelay(xg[..., :50], *phys, Dmax))          # zeros mean "nothing came before"


def _render_setup(L, seed):
    import grafx_amd.processors as P
    from test_gpu_render_state import _chain_graph, _eq, _parameters, _render_data

    procs = {"eq": _eq(), "fbdelay": P.FeedbackDelay(64, 441).cuda()}
    G = _chain_graph(["in", "eq", "fbdelay", "out"])
    params = _parameters(procs, G, seed)
    x = f64.bright_rows(2, 2, L, seed).view(2, 1, 2, L).cuda()
    return procs, x, params, _render_data(G)


def test_render_node_stream_and_captured_stream():
    """input -> equaliser -> FeedbackDelay -> output through render_grafx: streamed with state= in three blocks it equals
    the one render to the forward's tolerance (the walk restarts at each block); through CapturedStream the blocks are
    bit-identical to the eager ones started from silent_state -- the echoes go on inside a replayed graph."""
    from grafx_amd.render import CapturedStream, render_grafx, silent_state
    from test_gpu_render_state import _exact

    n, blocks = 1536, 3
    procs, x, params, rd = _render_setup(n * blocks, 31)
    with torch.no_grad():
        with _exact():       # (the equaliser's one call is a linear convolution only in this scope, as in test_gpu_render_state)
            want, _, _ = render_grafx(procs, x, params, rd)
            ys, state = [], None
            for k in range(blocks):
                yk, _, _, state = render_grafx(procs, x[..., k * n:(k + 1) * n], params, rd, state=state, return_state=True)
                ys.append(yk.clone())
        assert_close_rows(torch.cat(ys, -1), want.double().cpu(), 1e-5, "three blocks against the one render")
        eager, state = [], silent_state(procs, x[..., :n], params, rd)
        for k in range(blocks):
            yk, _, _, state = render_grafx(procs, x[..., k * n:(k + 1) * n], params, rd, state=state, return_state=True)
            eager.append(yk.clone())
        assert_close_rows(torch.cat(eager, -1), want.double().cpu(), 1e-5, "blocks from silent_state against the one render")
    stream = CapturedStream(procs, x[..., :n], params, rd)
    for k in range(blocks):
        yk, _, _ = stream(x[..., k * n:(k + 1) * n])
        assert torch.equal(yk, eager[k]), f"block {k}"
    assert not torch.equal(eager[1], eager[0])
