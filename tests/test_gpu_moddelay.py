"""The modulated delay line on the GPU (csrc/moddelay.hip, ops.moddelay / moddelay_bwd, autograd.ModulatedDelayFn,
processors.ModulatedDelay) against the float64 yardstick of tests/moddelay_float64.py on the same float32 inputs.

The forward is held to 1e-5 of every row's own peak (assert_close_rows).  An integer delay without depth is held to the
bits of dry x[n] + gain x[n - D] formed as the kernel forms it.  Every gradient is held to 1e-5 of its tensor's peak, or
else to what float32 torch autograd of the same formula is off float64 on the same inputs, measured on the spot on the
host and on the GPU (the policy of test_gpu_limiter._close_or_float32).  Streaming and determinism are
held to equal bits.  Tile edges come from ops.moddelay_tile.  Every parameter set is inside the contract
2 pi rate depth <= 1/2."""
import functools
import math

import pytest
import torch

import moddelay_float64 as m64
from conftest import assert_close_rows

pytestmark = pytest.mark.gpu

CONFIGS = [(1, 2, "linear"), (1, 8, "cubic"), (3, 441, "cubic"), (4, 1764, "cubic"), (2, 8192, "linear"), (8, 8192, "cubic")]
ROWS = [(1, 1), (3, 2), (2, 5)]                                                          # R, C
NAMES = ("x", "delay", "depth", "rate", "phase", "gain", "dry")


def _tile(Dmax, C):
    from grafx_amd import ops

    return ops.moddelay_tile(Dmax, C)


def _lengths(Dmax, C):
    t = _tile(Dmax, C)
    return sorted({1, Dmax - 1, t, t + 3, 2 * t + Dmax + 5})


def _cuda(ts):
    return tuple(t.cuda() for t in ts)


@functools.lru_cache(maxsize=None)
def _reference(V, Dmax, interp, R, C, L):
    """(x, params, g) float32 on the host, and the yardstick's y and seven gradients from one float64 graph: computed once."""
    x = m64.bright_rows(R, C, L, seed=1000 * V + 10 * R + C + L)
    params = m64.draw_parameters(R, V, C, Dmax, seed=Dmax + R + C)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(L), dtype=torch.float32)
    leaves = [t.double().clone().requires_grad_(True) for t in (x, *params)]
    y, _ = m64.forward(*leaves, Dmax, interp)
    (y * g.double()).sum().backward()
    return (x, params, g), (y.detach(), tuple(t.grad for t in leaves))


def _float32_autograd_errors(x, params, g, want, Dmax, interp):
    """Max errors of the seven gradients by float32 torch autograd of processors.moddelay.moddelay_torch against the
    float64 ones ``want`` on the same inputs: on the host and on the GPU, the larger one counts."""
    from grafx_amd.processors.moddelay import moddelay_torch

    worst = [0.0] * 7
    for device in ("cpu", "cuda"):
        leaves = [t.detach().clone().to(device).requires_grad_(True) for t in (x, *params)]
        (moddelay_torch(*leaves, Dmax, interp)[0] * g.to(device)).sum().backward()
        errs = [float((t.grad.double().cpu() - w).abs().max()) for t, w in zip(leaves, want)]
        print(f"float32 torch autograd on {device}: " + ", ".join(f"g_{n} {e:.3e}" for n, e in zip(NAMES, errs)))
        worst = [max(a, b) for a, b in zip(worst, errs)]
    return worst


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


@pytest.mark.parametrize("V,Dmax,interp", CONFIGS)
def test_forward_against_the_yardstick(V, Dmax, interp):
    from grafx_amd import ops

    for R, C in ROWS:
        for L in _lengths(Dmax, C):
            (x, params, _), (wy, _) = _reference(V, Dmax, interp, R, C, L)
            xg, pg = x.cuda(), _cuda(params)
            y = ops.moddelay(xg, *pg, Dmax, interp)
            what = f"V={V} Dmax={Dmax} {interp} R={R} C={C} L={L}"
            assert y.shape == (R, C, L)
            assert_close_rows(y, wy, 1e-5, what)
            out = _strided(torch.zeros_like(xg), 1, R)
            got = ops.moddelay(_strided(xg, 1, R), *pg, Dmax, interp, out=out)
            assert got.data_ptr() == out.data_ptr() and torch.equal(out.reshape(R, C, L), y), what + ": strided views"


@pytest.mark.parametrize("V,Dmax,interp", CONFIGS)
def test_an_integer_delay_without_depth_is_exact(V, Dmax, interp):
    """depth = 0 and an integer delay D give f = 0 and the weights (0, 1, 0, 0) exactly: the output has the bits of
    dry x[n] + sum_v gain_v x[n - D_v], a product and then one fused multiply-add per voice (formed here in float64, where
    the product of two float32 is exact, and rounded once per step).  Also at D = Dmax and D = 1."""
    from grafx_amd import ops

    R, C = 3, 2
    L = _tile(Dmax, C) + Dmax + 7
    gen = torch.Generator().manual_seed(Dmax + V)
    x = m64.bright_rows(R, C, L, 41)
    delays = torch.randint(1, Dmax + 1, (R, V), generator=gen)
    delays[0], delays[1] = Dmax, 1
    gain = torch.randn(R, V, C, generator=gen)
    dry = torch.tensor([0.7, 0.0, 1.3])
    rate, phase = torch.full((R, V), 1e-3), torch.rand(R, V, C, generator=gen)
    y = ops.moddelay(x.cuda(), delays.float().cuda(), torch.zeros(R, V).cuda(), rate.cuda(), phase.cuda(), gain.cuda(), dry.cuda(),
                     Dmax, interp)
    acc = (dry.reshape(R, 1, 1) * x)
    for v in range(V):
        for r in range(R):
            D = int(delays[r, v])
            shifted = torch.nn.functional.pad(x[r], (D, 0))[..., :L]
            acc[r] = (acc[r].double() + gain[r, v].double().reshape(C, 1) * shifted.double()).float()
    assert torch.equal(y.cpu(), acc)


def test_positions_near_two_to_the_31():
    """A stateful call that starts at position 2^31 - 5 with a swing of about 4000 samples: a phase accumulated in float32,
    or a position cut to 32 bits, is far outside 1e-5."""
    from grafx_amd import ops

    Dmax, V, R, C = 8192, 2, 2, 2
    L = _tile(Dmax, C) + 3
    x = m64.bright_rows(R, C, L, 43)
    gen = torch.Generator().manual_seed(44)
    delay = torch.tensor([[4096.0, 4100.5], [4090.25, 4096.0]])
    depth = torch.tensor([[4000.0, 3990.0], [4000.0, 3950.0]])
    rate = 0.49 / (2 * math.pi * depth.double()) * torch.tensor([[1.0, 0.7], [0.9, 1.0]], dtype=torch.float64)
    params = (delay, depth, rate.float(), torch.rand(R, V, C, generator=gen), torch.randn(R, V, C, generator=gen) / V,
              torch.tensor([0.5, 1.0]))
    state = (torch.randn(R, C, Dmax + 2, generator=gen), torch.tensor([2 ** 31 - 5, 2 ** 31 + 12345]))
    state[0][-1] *= 1e-3
    wy, (wz, wpos) = m64.forward(x, *params, Dmax, "cubic", state)
    y, (zf, pos) = ops.moddelay(x.cuda(), *_cuda(params), Dmax, "cubic", state=_cuda(state))
    assert_close_rows(y, wy, 1e-5, "positions near 2^31")
    assert torch.equal(pos.cpu(), wpos) and pos.dtype == torch.int64 and torch.equal(zf.cpu().double(), wz)


@pytest.mark.parametrize("V,Dmax,interp", CONFIGS)
def test_gradients_against_the_yardstick(V, Dmax, interp):
    """All seven gradients against float64 autograd of the definition; ``want`` subsets give None for the rest and the
    same bits for what is asked."""
    from grafx_amd import ops

    for R, C in ROWS:
        for L in _lengths(Dmax, C):
            (x, params, g), (_, want) = _reference(V, Dmax, interp, R, C, L)
            xg, pg, gg = x.cuda(), _cuda(params), g.cuda()
            got = ops.moddelay_bwd(xg, gg, *pg, Dmax, interp)
            what = f"V={V} Dmax={Dmax} {interp} R={R} C={C} L={L}"
            assert [tuple(t.shape) for t in got] == [tuple(w.shape) for w in want]
            allowed = functools.lru_cache(maxsize=None)(lambda: _float32_autograd_errors(x, params, g, want, Dmax, interp))
            for k, name in enumerate(NAMES):
                _close_or_float32(got[k], want[k], f"{what}: g_{name}", lambda k=k: allowed()[k])
            for subset in (("x",), ("delay", "gain"), ("rate", "phase", "depth", "dry")):
                part = ops.moddelay_bwd(xg, gg, *pg, Dmax, interp, want=subset)
                for name, a, b in zip(NAMES, part, got):
                    assert (a is None) if name not in subset else torch.equal(a, b), f"{what}: want={subset}: {name}"


def test_a_single_gradient_over_three_tiles_has_the_bits_of_all_seven():
    """Every gradient asked for alone, on rows of two tiles and 17 samples: None for the other six and the bits of the call
    that asks for all.  Alone, every other slot of the rows' tile sums has no destination when they are added up."""
    from grafx_amd import ops

    V, Dmax, R, C = 2, 441, 3, 2
    L = 2 * _tile(Dmax, C) + 17
    x = m64.bright_rows(R, C, L, 21).cuda()
    params = _cuda(m64.draw_parameters(R, V, C, Dmax, 22))
    g = torch.randn(R, C, L, generator=torch.Generator().manual_seed(23)).cuda()
    for interp in ("linear", "cubic"):
        every = ops.moddelay_bwd(x, g, *params, Dmax, interp)
        for only in NAMES:
            part = ops.moddelay_bwd(x, g, *params, Dmax, interp, want=(only,))
            for name, a, b in zip(NAMES, part, every):
                assert (a is None) if name != only else torch.equal(a, b), f"{interp}: want=({only},): {name}"


def test_determinism_rows_and_layout():
    """Two runs give equal bits, forward and backward; a row's result does not depend on the other rows; strided
    (B, n, C, L) views in and out match contiguous ones; an ``out`` that overlaps an input is refused."""
    from grafx_amd import ops

    V, Dmax, interp = 3, 441, "cubic"
    B, n, C = 2, 3, 2
    L = _tile(Dmax, C) + 9
    x = m64.bright_rows(B * n, C, L, 11).cuda()
    params = _cuda(m64.draw_parameters(B * n, V, C, Dmax, 12))
    g = torch.randn(B * n, C, L, generator=torch.Generator().manual_seed(5)).cuda()
    y, grads = ops.moddelay(x, *params, Dmax, interp), ops.moddelay_bwd(x, g, *params, Dmax, interp)
    y2, grads2 = ops.moddelay(x, *params, Dmax, interp), ops.moddelay_bwd(x, g, *params, Dmax, interp)
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    one = tuple(p[4:5] for p in params)
    assert torch.equal(ops.moddelay(x[4:5], *one, Dmax, interp), y[4:5])
    for a, b in zip(ops.moddelay_bwd(x[4:5], g[4:5], *one, Dmax, interp), grads):
        assert torch.equal(a, b[4:5])
    xin, gin = _strided(x, B, n), _strided(g, B, n)
    gout = torch.zeros(B, n, C, L + 2, device="cuda")[..., 1:1 + L]
    sgrads = ops.moddelay_bwd(xin, gin, *params, Dmax, interp, out=gout)
    assert sgrads[0].data_ptr() == gout.data_ptr() and torch.equal(gout.reshape(B * n, C, L), grads[0])
    assert all(torch.equal(a, b) for a, b in zip(sgrads[1:], grads[1:]))
    ws = torch.empty(ops.lib().gfx_moddelay_bwd_ws_bytes(B * n, C, L, V) + 8, dtype=torch.uint8, device="cuda")
    assert all(torch.equal(a, b) for a, b in zip(ops.moddelay_bwd(x, g, *params, Dmax, interp, ws=ws[:-8]), grads))
    with pytest.raises(ValueError, match="share memory"):
        ops.moddelay(x, *params, Dmax, interp, out=x)
    with pytest.raises(ValueError, match="share memory"):
        ops.moddelay_bwd(x, g, *params, Dmax, interp, out=g)
    with pytest.raises(ValueError, match="interp"):
        ops.moddelay(x, *params, Dmax, "sinc")
    with pytest.raises(ValueError, match="position must be a contiguous int64"):
        ops.moddelay(x, *params, Dmax, interp, state=(torch.zeros(B * n, C, Dmax + 2, device="cuda"), torch.zeros(B * n, device="cuda")))
    with pytest.raises(ValueError, match="history must be a contiguous float32 GPU tensor"):
        ops.moddelay(x, *params, Dmax, interp, state=(torch.zeros(B * n, C, Dmax, device="cuda"),
                                                     torch.zeros(B * n, dtype=torch.int64, device="cuda")))


def test_seventy_thousand_rows():
    """Rows ride on grid.x: more of them than grid.y holds.  Three of them are checked against the yardstick."""
    from grafx_amd import ops

    R, L, V, Dmax = 70000, 40, 2, 8
    x = torch.randn(R, 1, L, generator=torch.Generator().manual_seed(13))
    one = m64.draw_parameters(4, V, 1, Dmax, 14)
    params = tuple(p[torch.arange(R) % 4].contiguous() for p in one)
    g = torch.ones(R, 1, L)
    y = ops.moddelay(x.cuda(), *_cuda(params), Dmax, "cubic")
    got = ops.moddelay_bwd(x.cuda(), g.cuda(), *_cuda(params), Dmax, "cubic")
    rows = [0, 65537, R - 1]
    sub = tuple(p[rows] for p in params)
    wy, _ = m64.forward(x[rows], *sub, Dmax, "cubic")
    assert_close_rows(y[rows], wy, 1e-5, "70000 rows: y")
    for name, a, w in zip(NAMES, got, m64.gradients(x[rows], g[rows], *sub, Dmax, "cubic")):
        _close_or_float32(a[rows], w, f"70000 rows: g_{name}", lambda: 0.0)
        assert bool(torch.isfinite(a).all())
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("V,Dmax,interp", [(1, 8, "cubic"), (3, 441, "cubic"), (2, 8192, "linear")])
def test_blocks_equal_one_call_in_bits(V, Dmax, interp):
    """Blocks cut at 1, inside a tile, at a tile edge and beyond S, through ops.moddelay(state=),
    ModulatedDelay.forward(state=) and stream_block: outputs and states equal the one-call results bit for bit, and the
    position is the number of samples rendered."""
    import grafx_amd.processors as P
    from grafx_amd import ops

    R, C, S = 2, 2, Dmax + 2
    tile = _tile(Dmax, C)
    cuts = [1, 700, tile - 701, S + 5, 300]
    L = sum(cuts)
    m = P.ModulatedDelay(V, 0, Dmax, max_rate=60.0, interpolation=interp).cuda()
    gen = torch.Generator().manual_seed(23)
    z = dict(z_delay=torch.randn(R, V, generator=gen), z_depth=torch.randn(R, V, generator=gen) + 1, z_rate=torch.randn(R, V, generator=gen),
             phase=torch.rand(R, V, C, generator=gen), log_gain=0.3 * torch.randn(R, V, C, generator=gen),
             log_dry=0.3 * torch.randn(R, 1, generator=gen))
    z = {k: v.cuda() for k, v in z.items()}
    params = m.physical(**z)
    x = m64.bright_rows(R, C, L, 24).cuda()
    whole, (zw, pw) = ops.moddelay(x, *params, Dmax, interp, return_state=True)
    assert torch.equal(whole, ops.moddelay(x, *params, Dmax, interp)) and zw.shape == (R, C, S)
    assert torch.equal(zw, x[..., L - S:]) and pw.tolist() == [L] * R and pw.dtype == torch.int64
    x4, out4 = x.view(1, R, C, L), torch.zeros(1, R, C, L, device="cuda")
    ys, fs, state, fstate, carry, at = [], [], None, None, None, 0
    for n in cuts:
        y, state = ops.moddelay(x[..., at:at + n], *params, Dmax, interp, state=state, return_state=True)
        f, fstate = m(x[..., at:at + n], **z, state=fstate, return_state=True)
        carry = m.stream_block(x4[..., at:at + n], out4[..., at:at + n], carry, **z)
        ys.append(y), fs.append(f)
        at += n
        for other in (fstate, carry):
            assert torch.equal(state[0], other[0]) and torch.equal(state[1], other[1])
        assert state[1].tolist() == [at] * R
    assert torch.equal(torch.cat(ys, -1), whole) and torch.equal(torch.cat(fs, -1), whole) and torch.equal(out4[0], whole)
    assert torch.equal(state[0], zw) and torch.equal(state[1], pw)
    zeros = m.stream_silence(carry)
    assert zeros[1].dtype == torch.int64 and not bool(zeros[0].any()) and not bool(zeros[1].any())
    first = ops.moddelay(x[..., :50], *params, Dmax, interp, state=zeros, return_state=True)[0]
    assert torch.equal(first, whole[..., :50])          # zeros mean "nothing came before"


def test_blocks_with_a_two_chunk_history_from_strided_views():
    """The history copy runs on one workgroup per 1024 state samples (launch_history_tail, csrc/common.hip): max_delay =
    1500 keeps S = 1502 of them, two chunks, the second partial and no multiple of 256.  Blocks of 400 (shorter than S,
    entering without a state), 400 (shorter, entering with one: the old history shifts) and 2500 (longer), read as strided
    (B, n, C, L) views of a wider buffer: outputs and every history equal the one-call results bit for bit, and the
    position is the number of samples rendered."""
    from grafx_amd import ops

    V, Dmax, interp = 3, 1500, "cubic"
    B, n, C, S = 1, 3, 2, Dmax + 2
    cuts = [400, 400, 2500]
    L = sum(cuts)
    x = m64.bright_rows(B * n, C, L, 31).cuda()
    params = _cuda(m64.draw_parameters(B * n, V, C, Dmax, 32))
    whole, (zw, pw) = ops.moddelay(x, *params, Dmax, interp, return_state=True)
    assert zw.shape == (B * n, C, S) and torch.equal(zw, x[..., L - S:]) and pw.tolist() == [L] * (B * n)
    xin = _strided(x, B, n)
    ys, state, at = [], None, 0
    for m in cuts:
        y, state = ops.moddelay(xin[..., at:at + m], *params, Dmax, interp, state=state, return_state=True)
        at += m
        zs, ps = ops.moddelay(x[..., :at], *params, Dmax, interp, return_state=True)[1]
        assert torch.equal(state[0], zs) and state[1].tolist() == ps.tolist() == [at] * (B * n)
        ys.append(y.reshape(B * n, C, m))
    assert torch.equal(torch.cat(ys, -1), whole) and torch.equal(state[0], zw) and torch.equal(state[1], pw)


def test_module_and_node_agree_with_the_op():
    """ModulatedDelay(...)(x, **z) is ops.moddelay on physical(**z); under requires_grad it runs ModulatedDelayFn, whose
    gradients in x and the z parameters match float64 autograd of torch_forward under the policy of this file."""
    import grafx_amd.processors as P
    from grafx_amd import ops
    from grafx_amd.autograd import ModulatedDelayFn

    V, Dmax, interp, R, C = 3, 48, "cubic", 3, 2      # (short delays: float32 rounding of the mapping moves them least)
    L = _tile(Dmax, C) + 3
    m = P.ModulatedDelay(V, 4, Dmax, max_rate=40.0, interpolation=interp).cuda()
    gen = torch.Generator().manual_seed(19)
    z = [torch.randn(R, V, generator=gen), torch.randn(R, V, generator=gen), torch.randn(R, V, generator=gen),
         torch.rand(R, V, C, generator=gen), 0.3 * torch.randn(R, V, C, generator=gen), 0.3 * torch.randn(R, 1, generator=gen)]
    x = m64.bright_rows(R, C, L, 20)
    g = torch.randn(R, C, L, generator=torch.Generator().manual_seed(7))
    xg, zg, gg = x.cuda(), [t.cuda() for t in z], g.cuda()
    params = m.physical(*zg)
    wy = ops.moddelay(xg, *params, Dmax, interp)
    wgrads = ops.moddelay_bwd(xg, gg, *params, Dmax, interp)
    assert torch.equal(m(xg, *zg), wy)
    leaves = [xg.clone().requires_grad_(True), *(p.clone().requires_grad_(True) for p in params)]
    y = ModulatedDelayFn.apply(*leaves, Dmax, interp)
    assert torch.equal(y.detach(), wy)
    y.backward(gg)
    assert all(torch.equal(t.grad, w.reshape(t.shape)) for t, w in zip(leaves, wgrads))
    only = params[1].clone().requires_grad_(True)        # the depth alone: the node asks for nothing else
    ModulatedDelayFn.apply(xg, params[0], only, *params[2:], Dmax, interp).backward(gg)
    assert torch.equal(only.grad, wgrads[2])
    # the module under autograd against float64 autograd of its own torch formula
    leaves = [xg.clone().requires_grad_(True), *(t.clone().requires_grad_(True) for t in zg)]
    y = m(*leaves)
    assert torch.equal(y.detach(), wy) and type(y.grad_fn).__name__.startswith("ModulatedDelayFn")
    y.backward(gg)

    def torch_grads(dtype, device):
        ls = [t.detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for t in (x, *z)]
        (m.torch_forward(*ls) * g.to(device=device, dtype=dtype)).sum().backward()
        return [t.grad.double().cpu() for t in ls]

    want = torch_grads(torch.float64, "cpu")
    allowed = functools.lru_cache(maxsize=None)(lambda: [max(float((a - w).abs().max()), float((b - w).abs().max())) for a, b, w in
                                                         zip(torch_grads(torch.float32, "cpu"), torch_grads(torch.float32, "cuda"), want)])
    for k, name in enumerate(("x", "z_delay", "z_depth", "z_rate", "phase", "log_gain", "log_dry")):
        _close_or_float32(leaves[k].grad, want[k], f"module: g_{name}", lambda k=k: allowed()[k])
    with pytest.raises(ValueError, match="no native backward"):
        m(leaves[0], *zg, state=m(xg, *zg, return_state=True)[1])
    y, (hist, pos) = m(leaves[0], *zg, return_state=True)     # return_state alone under autograd: (y, state_after)
    _, (whist, wpos) = m(xg, *zg, return_state=True)
    assert torch.equal(hist, whist) and torch.equal(pos, wpos)


def _render_setup(L, seed, smooth=False):
    """``smooth``: two slow sines per row instead of white noise (a loss that a small step in the delay lowers)."""
    import grafx_amd.processors as P
    from test_gpu_render_state import _chain_graph, _parameters, _render_data

    procs = {"moddelay": P.ModulatedDelay(2, 16, 441, max_rate=40.0).cuda()}
    G = _chain_graph(["in", "moddelay", "out"])
    params = _parameters(procs, G, seed)
    x = m64.bright_rows(2, 2, L, seed).view(2, 1, 2, L).cuda()
    if smooth:
        k = torch.arange(4, dtype=torch.float64).view(2, 1, 2, 1)
        x = torch.sin(2 * math.pi * (0.01 + 0.003 * k) * torch.arange(L, dtype=torch.float64) + k).float().cuda()
    return procs, x, params, _render_data(G)


def test_render_node_stream_and_captured_stream():
    """input -> ModulatedDelay -> output through render_grafx equals forward(); streamed with state= in blocks of 512 it
    equals the one call in bits; through CapturedStream the blocks are bit-identical to the eager ones -- the oscillator
    advances inside a replayed graph because the position lives on the device."""
    from grafx_amd.render import CapturedStream, render_grafx, silent_state

    n, blocks = 512, 6
    procs, x, params, rd = _render_setup(n * blocks, 31)
    m = procs["moddelay"]
    with torch.no_grad():
        rows = {k: v.expand(2, *v.shape[1:]) for k, v in params["moddelay"].items()}      # one node, a batch of two
        want = m(x[:, 0], **rows).unsqueeze(1)               # the render's output keeps the node dimension: (B, 1, C, L)
        y, _, _ = render_grafx(procs, x, params, rd)
        assert torch.equal(y.reshape(want.shape), want)
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
    assert not torch.equal(eager[1], eager[0])


def test_render_trains_the_depth():
    """One optimiser step through render_grafx changes z_depth and lowers an L2 loss to a target rendered with other
    parameters."""
    from grafx_amd.render import render_grafx

    procs, x, params, rd = _render_setup(3000, 37, smooth=True)
    other = {k: v.clone() for k, v in params["moddelay"].items()}
    other["z_depth"] = other["z_depth"] + 1.5
    other["log_gain"] = other["log_gain"] + 0.2
    with torch.no_grad():
        target, _, _ = render_grafx(procs, x, {"moddelay": other}, rd)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params["moddelay"].items()}
    opt = torch.optim.SGD(leaves.values(), lr=1e-2)

    def loss():
        y, _, _ = render_grafx(procs, x, {"moddelay": leaves}, rd)
        return (y - target).square().mean()

    before = loss()
    before.backward()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in leaves.values())
    assert float(leaves["z_depth"].grad.abs().max()) > 0
    start = leaves["z_depth"].detach().clone()
    opt.step()
    with torch.no_grad():
        after = loss()
    before = before.detach()
    print(f"loss {float(before):.6e} -> {float(after):.6e}")
    assert not torch.equal(leaves["z_depth"].detach(), start) and float(after) < float(before)
