"""The oversampled waveshapers on the GPU (gfx_oversampled_waveshaper_f32 / _bwd_f32, ops.oversampled_waveshaper(_bwd),
autograd.OversampledWaveshaperFn, the ``oversample=`` keyword of the four distortions) against the float64 definition of
tests/oversampled_float64.py, at the standing 1e-5 (peak-relative and relative L2).

Inputs follow test_gpu_waveshaper_bwd.py (parameters randn * 0.5, log_pre_gain <= 0 for the polynomial shapers) except that
x is uniform in [-0.55, 0.55]: sinc interpolation of white noise overshoots by 1.65, so +-0.9 would reach |u| = 1.48, where
the Chebyshev basis is ill-conditioned and float32 autograd of the formula itself is 1e-5 off float64.  With +-0.55 the
interpolated peak is 0.91 and the float32 formula stays within 5.2e-6 of float64, so a miss at 1e-5 is a kernel defect.
One more narrowing, of the piecewise shaper's pre gain, with its reason and figures at _past_the_thresholds."""
import functools

import pytest
import torch

import oversampled_float64 as o64
from conftest import assert_close
from test_gpu_next_rows2 import NL
from test_gpu_waveshaper_bwd import _off_by_one_float

pytestmark = pytest.mark.gpu

FACTORS = (2, 3, 4, 8)
# name -> (mode, K, use_tanh, inverse_post_gain, remove_dc, parameters given): the four modes, bias, both post gains, centring
CONFIGS = {
    "tanh_inv": (o64.TANH, 0, False, True, False, ("log_pre_gain",)),
    "tanh_bias_dc": (o64.TANH, 0, False, False, True, ("log_pre_gain", "log_post_gain", "p0")),
    "tanh_bare": (o64.TANH, 0, False, False, False, ()),
    "pw_inv": (o64.PIECEWISE, 0, False, True, False, ("log_pre_gain", "p0", "p1")),
    "pw_post_dc": (o64.PIECEWISE, 0, False, False, True, ("log_pre_gain", "log_post_gain", "p0", "p1")),
    "pow": (o64.POWER, 10, False, False, False, ("log_pre_gain", "p0")),
    "pow_tanh_dc": (o64.POWER, 6, True, False, True, ("p0",)),
    "cheb": (o64.CHEBYSHEV, 10, False, False, False, ("log_pre_gain", "p0")),
    "cheb_tanh_dc": (o64.CHEBYSHEV, 6, True, True, True, ("log_pre_gain", "p0")),
    "pow_1": (o64.POWER, 1, False, False, False, ("log_pre_gain", "p0")),
    "cheb_1_tanh": (o64.CHEBYSHEV, 1, True, False, True, ("log_pre_gain", "p0")),
    "pow_32": (o64.POWER, 32, False, False, False, ("log_pre_gain", "p0")),
    "cheb_32": (o64.CHEBYSHEV, 32, False, False, True, ("log_pre_gain", "p0")),
    "cheb_32_tanh": (o64.CHEBYSHEV, 32, True, False, False, ("log_pre_gain", "p0")),
}
FORWARD = ("tanh_inv", "tanh_bias_dc", "tanh_bare", "pw_inv", "pw_post_dc", "pow", "pow_tanh_dc", "cheb", "cheb_tanh_dc")


def _tile(factor):
    from grafx_amd import ops

    return ops.oversampled_waveshaper_tile(factor)


@functools.lru_cache(maxsize=None)
def _filters(factor):
    """The default design on the GPU as the ops take it; factor 1: the identity, one tap of 1.0 each way."""
    if factor == 1:
        return torch.ones(1, device="cuda"), 0, torch.ones(1, device="cuda"), 0
    h_up, o_up, h_dn, o_dn = o64.filters(factor)
    return h_up.cuda(), o_up, h_dn.cuda(), o_dn


def _past_the_thresholds(log_pre_gain):
    """The piecewise shaper's pre gain, narrowed to |randn * 0.5| + 0.5.  Its thresholds are sigmoid(randn * 0.5), 0.38 to
    0.62 mostly; with |x| <= 0.55 and a pre gain around 1 only a handful of samples pass them, by a = hardness (u - k) of a
    few hundredths, and the hardness gradient a sech^2(a) - tanh(a) ~ -2 a^3 / 3 of such a sample keeps eps / a^2 of its
    value in ANY float32 evaluation: float32 torch autograd of the definition is 4.6e-5 off float64 there (F = 3, L = 2689,
    seed 1, two and three samples past the threshold), the kernel 2.0e-5.  With the pre gain at 1.65 and more the outer
    branches hold a good share of the samples and float32 autograd is within 2.9e-6 on every case of this file."""
    return log_pre_gain.abs() + 0.5


def _cfg(name):
    mode, K, use_tanh, inverse, remove_dc, given = CONFIGS[name]
    return dict(mode=mode, use_tanh=use_tanh, inverse_post_gain=inverse, remove_dc=remove_dc)


@functools.lru_cache(maxsize=None)
def _case(name, factor, R, C, L, seed=0):
    """(x, parameters by their ops names, gy) on the CPU in float32 and the float64 reference {"y", "x", names} -- computed
    once per case and shared; nothing modifies them."""
    mode, K, use_tanh, inverse, remove_dc, given = CONFIGS[name]
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(R, C, L, generator=gen) * 1.1 - 0.55
    width = {"log_pre_gain": 1, "log_post_gain": 1, "p0": K if K else (2 if mode == o64.PIECEWISE else 1), "p1": 2}
    ps = {k: torch.randn(R, width[k], generator=gen) * 0.5 for k in given}
    if mode >= o64.POWER and "log_pre_gain" in ps:
        ps["log_pre_gain"] = -ps["log_pre_gain"].abs()
    if mode == o64.PIECEWISE:
        ps["log_pre_gain"] = _past_the_thresholds(ps["log_pre_gain"])
    gy = torch.randn(R, C, L, generator=gen)
    h_up, o_up, h_dn, o_dn = o64.filters(factor) if factor > 1 else (torch.ones(1), 0, torch.ones(1), 0)
    ref = o64.reference(x, gy, ps, factor=factor, h_up=h_up, o_up=o_up, h_dn=h_dn, o_dn=o_dn, **_cfg(name))
    return x, ps, gy, ref


def _forward(name, factor, x, ps, **kw):
    from grafx_amd import ops

    cfg = _cfg(name)
    return ops.oversampled_waveshaper(x, cfg.pop("mode"), factor, *_filters(factor), **{k: v.cuda() for k, v in ps.items()},
                                      **cfg, **kw)


def _backward(name, factor, x, gy, ps, **kw):
    from grafx_amd import ops

    cfg = _cfg(name)
    return ops.oversampled_waveshaper_bwd(x, gy, cfg.pop("mode"), factor, *_filters(factor),
                                          **{k: v.cuda() for k, v in ps.items()}, **cfg, **kw)


def _check(gx, grads, ps, ref, what, names=None):
    names = tuple(ps) if names is None else names
    if gx is not None:
        assert_close(gx.reshape(ref["x"].shape).cpu(), ref["x"], 1e-5, f"{what}: gx")
    assert set(grads) == set(names)
    for k in names:
        assert_close(grads[k].reshape(ref[k].shape).cpu(), ref[k], 1e-5, f"{what}: d/d{k}")


# ------------------------------------------------------------------------------------------------- 1: forward against float64
@pytest.mark.parametrize("name", FORWARD)
@pytest.mark.parametrize("factor", FACTORS)
def test_forward_matches_float64(factor, name):
    x, ps, _, ref = _case(name, factor, 3, 2, 700)
    y = _forward(name, factor, x.cuda(), ps)
    assert y.shape == (3, 2, 700)
    assert_close(y.cpu(), ref["y"], 1e-5, f"{name} F={factor}")


# ------------------------------------------------------------------------------------------------------------------ 2: lengths
def _lengths(factor):
    T = _tile(factor)
    return (T - 1, T, T + 1, 2 * T + 1)


@pytest.mark.parametrize("name", ["tanh_bias_dc", "cheb"])
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("L", [1, 5])
def test_rows_shorter_than_every_halo(L, factor, name):
    x, ps, _, ref = _case(name, factor, 3, 2, L, seed=L)
    assert_close(_forward(name, factor, x.cuda(), ps).cpu(), ref["y"], 1e-5, f"{name} F={factor} L={L}")


@pytest.mark.parametrize("name", ["tanh_inv", "pw_post_dc"])
@pytest.mark.parametrize("factor,which", [(f, i) for f in (3, 4) for i in range(4)])
def test_lengths_around_the_tile(factor, which, name):
    L = _lengths(factor)[which]
    x, ps, _, ref = _case(name, factor, 2, 2, L, seed=which)
    assert_close(_forward(name, factor, x.cuda(), ps).cpu(), ref["y"], 1e-5, f"{name} F={factor} L={L}")


@pytest.mark.parametrize("name", ["pow", "cheb_tanh_dc"])
@pytest.mark.parametrize("factor", [3, 4])
def test_the_shaped_signal_is_zero_outside_the_row(factor, name):
    """A polynomial shaper has the constant term w_0 f(1): were v = s(0) past the ends of the row instead of 0, the first
    and last outputs would carry it through the decimator's taps.  The constant is not small here."""
    for L in (5, _tile(factor) + 1):
        x, ps, _, ref = _case(name, factor, 2, 2, L, seed=8)
        assert float(torch.tanh(ps["p0"][:, 0]).abs().min()) > 0.1
        y = _forward(name, factor, x.cuda(), ps).cpu()
        assert_close(y, ref["y"], 1e-5, f"{name} F={factor} L={L}")
        assert_close(y[..., :3], ref["y"][..., :3], 1e-5, f"{name} F={factor} L={L}: head")
        assert_close(y[..., -3:], ref["y"][..., -3:], 1e-5, f"{name} F={factor} L={L}: tail")


@pytest.mark.parametrize("factor,n_up,o_up,n_dn,o_dn", [(1, 1024, 0, 1024, 1023), (1, 1024, 1023, 1024, 0), (16, 1024, 511, 1024, 512),
                                                       (16, 1, 0, 1, 0), (16, 3, 2, 40, 0), (5, 1024, 7, 2, 1)])
def test_the_ends_of_the_served_range(factor, n_up, o_up, n_dn, o_dn):
    """The largest and smallest filters and factors the entries take, offsets at either end, forward and backward: factor 1
    with two filters of 1024 taps is the one geometry whose backward tile needs more than 64 KiB of LDS; filters shorter
    than the factor have phases without a tap.  Taps randn / sqrt(N): the interpolated signal keeps the input's scale.
    The tanh shaper with bias, both gains and remove_dc -- a post gain of its own, not the inverse of the pre gain: under
    inverse_post_gain the pre-gain gradient is the difference s'(u) u - s(u), small at a pre gain of 0.36 on such a
    signal, and float32 autograd of the definition is itself 3.3e-5 off float64 there (F = 5); with the post gain it is
    within 4.0e-6 on all six geometries.  The cancellation has its cases among the configurations above."""
    from grafx_amd import ops

    L = _tile(factor) + 1
    gen = torch.Generator().manual_seed(n_up + n_dn)
    h_up, h_dn = torch.randn(n_up, generator=gen) / n_up ** 0.5, torch.randn(n_dn, generator=gen) / n_dn ** 0.5
    x = torch.rand(2, 2, L, generator=gen) * 1.1 - 0.55
    ps = {k: torch.randn(2, 1, generator=gen) * 0.5 for k in ("log_pre_gain", "log_post_gain", "p0")}
    cfg = dict(mode=o64.TANH, factor=factor, h_up=h_up, o_up=o_up, h_dn=h_dn, o_dn=o_dn, remove_dc=True)
    # gy is the output itself, the cotangent of the loss |y|^2 / 2, so that a parameter sum adds terms of like sign.  With a
    # white gy and two white filters of 1024 taps every term carries about eps sqrt(N / 2) = 1.3e-6 of itself from its two
    # float32 dot products, and the post-gain sum of the first geometry cancels to a tenth of its terms' root sum square
    # (2.58 against 25.3, in float64): 1e-5 of the sum is then less than the format gives, whatever evaluates it.
    gy = o64.forward(x.double(), **cfg, **{k: v.double() for k, v in ps.items()}).float()
    ref = o64.reference(x, gy, ps, **cfg)
    args = (factor, h_up.cuda(), o_up, h_dn.cuda(), o_dn)
    kw = dict(remove_dc=True, **{k: v.cuda() for k, v in ps.items()})
    what = f"F={factor}, {n_up} + {n_dn} taps"
    assert_close(ops.oversampled_waveshaper(x.cuda(), ops.WS_TANH, *args, **kw).cpu(), ref["y"], 1e-5, what)
    gx, grads = ops.oversampled_waveshaper_bwd(x.cuda(), gy.cuda(), ops.WS_TANH, *args, **kw)
    _check(gx, grads, ps, ref, what)


# --------------------------------------------------------------------------------------------------------------------- 3: bits
@pytest.mark.parametrize("name", ["tanh_inv", "tanh_bias_dc", "pw_inv", "pw_post_dc", "pow", "pow_tanh_dc", "cheb", "cheb_tanh_dc"])
def test_factor_one_is_the_plain_waveshaper_bit_for_bit(name):
    """factor = 1 with the taps [1.0]: interpolation and decimation are exact, so y has the bits of ops.waveshaper (with and
    without remove_dc: both subtract the means of ops.row_mean) and gx those of ops.waveshaper_bwd.  Under remove_dc gx
    is compared at 1e-5 instead: its mean is added up from per-tile partial sums here and per-workgroup ones there, and
    the last bit of a float sum depends on the grouping."""
    from grafx_amd import ops

    x, ps, gy, ref = _case(name, 1, 3, 2, 4099)
    cfg = _cfg(name)
    mode = cfg.pop("mode")
    pg = {k: v.cuda() for k, v in ps.items()}
    y = _forward(name, 1, x.cuda(), ps)
    assert torch.equal(y, ops.waveshaper(x.cuda(), mode, **pg, **cfg))
    assert_close(y.cpu(), ref["y"], 1e-5, name)
    gx, grads = _backward(name, 1, x.cuda(), gy.cuda(), ps)
    want_gx, want = ops.waveshaper_bwd(x.cuda(), gy.cuda(), mode, **pg, **cfg)
    if cfg["remove_dc"]:
        assert_close(gx.cpu(), want_gx.double().cpu(), 1e-5, f"{name}: gx against the plain backward")
    else:
        assert torch.equal(gx, want_gx)
    _check(gx, grads, ps, ref, name)


@pytest.mark.parametrize("name", ["tanh_bias_dc", "pw_post_dc", "cheb_tanh_dc"])
def test_equal_bits_from_call_to_call_and_rows_on_their_own(name):
    factor = 4
    L = 2 * _tile(factor) + 1
    x, ps, gy, _ = _case(name, factor, 3, 2, L)
    xg, gg = x.cuda(), gy.cuda()
    y, y2 = _forward(name, factor, xg, ps), _forward(name, factor, xg, ps)
    gx, grads = _backward(name, factor, xg, gg, ps)
    gx2, grads2 = _backward(name, factor, xg, gg, ps)
    assert torch.equal(y, y2) and torch.equal(gx, gx2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    one = {k: v[1:2] for k, v in ps.items()}                                 # row 1 alone
    assert torch.equal(_forward(name, factor, xg[1:2], one), y[1:2])
    gx1, grads1 = _backward(name, factor, xg[1:2], gg[1:2], one)
    assert torch.equal(gx1, gx[1:2])
    for k in grads:
        assert torch.equal(grads1[k], grads[k][1:2]), k


# ------------------------------------------------------------------------------------------- 4: backward against float64 autograd
@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("factor", FACTORS)
def test_backward_matches_float64_autograd(factor, name):
    T = _tile(factor)
    for L in (5, T + 1, 2 * T + 1):
        x, ps, gy, ref = _case(name, factor, 3, 2, L, seed=L % 7)
        what = f"{name} F={factor} L={L}"
        out = torch.full((3, 2, L), float("nan"), device="cuda")
        gx, grads = _backward(name, factor, x.cuda(), gy.cuda(), ps, out=out)
        assert gx is out and not torch.isnan(out).any()
        _check(gx, grads, ps, ref, what)
        if CONFIGS[name][4]:                                             # remove_dc: gx is blind to a constant offset
            total, scale = gx.double().sum(-1).abs(), gx.double().abs().sum(-1)
            assert (total <= 1e-6 * scale).all(), (what, float((total / scale).max()))


@pytest.mark.parametrize("name", ["tanh_bias_dc", "pw_post_dc", "cheb_tanh_dc"])
@pytest.mark.parametrize("factor", [3, 8])
def test_only_some_gradients(factor, name):
    L = _tile(factor) + 1
    x, ps, gy, ref = _case(name, factor, 3, 2, L, seed=L % 7)
    xg, gg = x.cuda(), gy.cuda()
    gx, grads = _backward(name, factor, xg, gg, ps, want=tuple(ps))                   # parameters only
    assert gx is None
    _check(None, grads, ps, ref, f"{name} F={factor}: parameters only")
    gx, grads = _backward(name, factor, xg, gg, ps, want=("x",))                      # input only
    assert grads == {}
    _check(gx, grads, ps, ref, f"{name} F={factor}: gx only", names=())
    one = sorted(ps)[0]
    gx, grads = _backward(name, factor, xg, gg, ps, want=(one,))                      # one parameter
    assert gx is None
    _check(None, grads, ps, ref, f"{name} F={factor}: {one} only", names=(one,))
    with pytest.raises(ValueError, match="unknown gradients"):
        _backward(name, factor, xg, gg, ps, want=("h_up",))


# ------------------------------------------------------------------------------------------------------------------ 5: layouts
@pytest.mark.parametrize("name", ["tanh_bias_dc", "cheb"])
def test_strided_views_in_and_out(name):
    """x and gy as (B, n, C, L) views of one larger buffer each, y and gx into views of two more; rows L + 1 apart.  Nothing
    outside the views is touched."""
    factor, B, n, C = 4, 2, 3, 2
    L = _tile(factor) + 3
    x, ps, gy, ref = _case(name, factor, B * n, C, L)
    xbuf = torch.full((B, 7, C, L + 1), 3.0, device="cuda")
    gbuf = torch.full((B, 6, C, L + 1), 5.0, device="cuda")
    ybuf = torch.full((B, 8, C, L + 1), 7.0, device="cuda")
    obuf = torch.full((B, 8, C, L + 1), 7.0, device="cuda")
    xv, gv, yv, ov = xbuf[:, 2:5, :, :L], gbuf[:, 1:4, :, :L], ybuf[:, 0:3, :, :L], obuf[:, 4:7, :, :L]
    xv.copy_(x.view(B, n, C, L))
    gv.copy_(gy.view(B, n, C, L))
    xkeep, gkeep = xbuf.clone(), gbuf.clone()
    y = _forward(name, factor, xv, ps, out=yv)
    gx, grads = _backward(name, factor, xv, gv, ps, out=ov)
    assert y is yv and gx is ov
    assert_close(y.reshape(B * n, C, L).cpu(), ref["y"], 1e-5, f"{name}: strided views, y")
    _check(gx, grads, ps, ref, f"{name}: strided views")
    assert torch.equal(xbuf, xkeep) and torch.equal(gbuf, gkeep)
    for buf, lo in ((ybuf, 0), (obuf, 4)):
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:, lo:lo + 3, :, :L] = False
        assert torch.equal(buf[outside], torch.full_like(buf[outside], 7.0))
    # two node ranges of ONE buffer interleave in memory without sharing an element: x and y may be such a pair
    both = torch.full((B, 8, C, L + 1), 7.0, device="cuda")
    both[:, 0:3, :, :L].copy_(x.view(B, n, C, L))
    y = _forward(name, factor, both[:, 0:3, :, :L], ps, out=both[:, 3:6, :, :L])
    assert_close(y.reshape(B * n, C, L).cpu(), ref["y"], 1e-5, f"{name}: x and y in one buffer")


@pytest.mark.parametrize("misaligned", ["x", "gy", "out"])
def test_bases_off_the_16_byte_grid(misaligned):
    name, factor = "pw_post_dc", 3
    L = _tile(factor) + 1
    x, ps, gy, ref = _case(name, factor, 3, 2, L, seed=L % 7)
    xg = _off_by_one_float(x) if misaligned == "x" else x.cuda()
    gg = _off_by_one_float(gy) if misaligned == "gy" else gy.cuda()
    blank = torch.full((3, 2, L), float("nan"))
    y = _forward(name, factor, xg, ps, out=_off_by_one_float(blank) if misaligned == "out" else None)
    assert_close(y.cpu(), ref["y"], 1e-5, f"misaligned {misaligned}: y")
    gx, grads = _backward(name, factor, xg, gg, ps, out=_off_by_one_float(blank) if misaligned == "out" else None)
    _check(gx, grads, ps, ref, f"misaligned {misaligned}")


def test_refusals_of_the_wrappers():
    from grafx_amd import ops

    factor, L = 4, 64
    x, ps, gy, _ = _case("tanh_inv", factor, 2, 2, L)
    xg, gg = x.cuda(), gy.cuda()
    h_up, o_up, h_dn, o_dn = _filters(factor)
    pre = ps["log_pre_gain"].cuda()
    with pytest.raises(ValueError, match="must not share memory"):                             # out is x: never in place
        ops.oversampled_waveshaper(xg, ops.WS_TANH, factor, h_up, o_up, h_dn, o_dn, pre, inverse_post_gain=True, out=xg)
    buf = torch.zeros(2, 2, L + 8, device="cuda")                                              # ... nor a sample later
    with pytest.raises(ValueError, match="must not share memory"):
        ops.oversampled_waveshaper(buf[..., :L], ops.WS_TANH, factor, h_up, o_up, h_dn, o_dn, pre, inverse_post_gain=True,
                                   out=buf[..., 1:L + 1])
    for out in (xg, gg):
        with pytest.raises(ValueError, match="must not share memory"):
            ops.oversampled_waveshaper_bwd(xg, gg, ops.WS_TANH, factor, h_up, o_up, h_dn, o_dn, pre, inverse_post_gain=True, out=out)
    with pytest.raises(TypeError, match="h_up must be a float32 tensor on the GPU"):
        ops.oversampled_waveshaper(xg, ops.WS_TANH, factor, h_up.cpu(), o_up, h_dn, o_dn)
    with pytest.raises(TypeError, match="h_dn must be a float32 tensor on the GPU"):
        ops.oversampled_waveshaper_bwd(xg, gg, ops.WS_TANH, factor, h_up, o_up, h_dn.double(), o_dn)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.oversampled_waveshaper(x, ops.WS_TANH, factor, h_up, o_up, h_dn, o_dn)
    for bad in (dict(factor=0), dict(factor=17), dict(factor=2.0), dict(o_up=49), dict(o_dn=-1), dict(h_up=torch.zeros(1025, device="cuda")),
                dict(h_dn=torch.zeros(2, 3, device="cuda"))):
        a = dict(factor=factor, h_up=h_up, o_up=o_up, h_dn=h_dn, o_dn=o_dn)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.oversampled_waveshaper(xg, ops.WS_TANH, a["factor"], a["h_up"], a["o_up"], a["h_dn"], a["o_dn"])
    with pytest.raises(ValueError, match="does not match the input"):
        ops.oversampled_waveshaper_bwd(xg, gg[..., :-1], ops.WS_TANH, factor, h_up, o_up, h_dn, o_dn)


def test_the_node_writes_gx_into_a_grad_sink_and_refuses_trainable_taps():
    from grafx_amd import autograd as diff

    name, factor = "tanh_bias_dc", 4
    L = _tile(factor) + 1
    x, ps, gy, ref = _case(name, factor, 3, 2, L, seed=L % 7)
    cfg = _cfg(name)
    xg = x.cuda().requires_grad_()
    pg = {k: v.cuda().requires_grad_() for k, v in ps.items()}
    h_up, o_up, h_dn, o_dn = _filters(factor)

    def run():
        return diff.OversampledWaveshaperFn.apply(xg, pg["log_pre_gain"], pg["log_post_gain"], pg["p0"], None, cfg["mode"],
                                                  cfg["use_tanh"], cfg["inverse_post_gain"], cfg["remove_dc"], factor,
                                                  (h_up, o_up, h_dn, o_dn))

    y = run()
    assert_close(y.detach().cpu(), ref["y"], 1e-5, "node: y")
    buf = torch.zeros(3, 2, 2, L, device="cuda")
    with diff.grad_sink(xg, buf[:, 1]) as sink:
        grads = torch.autograd.grad(y, [xg, *pg.values()], gy.cuda())
        assert sink.writes == 1
    assert grads[0].data_ptr() == buf[:, 1].data_ptr() and torch.count_nonzero(buf[:, 0]) == 0
    assert_close(buf[:, 1].cpu(), ref["x"], 1e-5, "node: gx in the sink")
    for k, g in zip(pg, grads[1:]):
        assert g.shape == pg[k].shape
        assert_close(g.cpu(), ref[k], 1e-5, f"node: d/d{k}")
    with pytest.raises(ValueError, match="taps get no gradient"):
        diff.OversampledWaveshaperFn.apply(xg, None, None, None, None, cfg["mode"], False, False, False, factor,
                                           (h_up.clone().requires_grad_(), o_up, h_dn, o_dn))


# ---------------------------------------------------------------------------------------------------------------- 6: many rows
def test_more_rows_than_one_launch_grid():
    """65 537 rows x 1 channel x 40 samples at F = 2: rows 0, 1 and 65 536 have the bits of the three-row call, forward,
    gx and parameter gradients."""
    name, factor, R, L = "pw_post_dc", 2, 65537, 40
    x, ps, gy, _ = _case(name, factor, 3, 1, L)
    rows = torch.tensor([0, 1, R - 1])
    gen = torch.Generator().manual_seed(1)
    xb = (torch.rand(R, 1, L, generator=gen) * 1.1 - 0.55)
    gb = torch.randn(R, 1, L, generator=gen)
    pb = {k: torch.randn(R, v.shape[1], generator=gen) * 0.5 for k, v in ps.items()}
    xb[rows], gb[rows] = x, gy
    for k in pb:
        pb[k][rows] = ps[k]
    y3 = _forward(name, factor, x.cuda(), ps)
    gx3, grads3 = _backward(name, factor, x.cuda(), gy.cuda(), ps)
    y = _forward(name, factor, xb.cuda(), pb)
    gx, grads = _backward(name, factor, xb.cuda(), gb.cuda(), pb)
    rows = rows.cuda()
    assert torch.equal(y[rows], y3) and torch.equal(gx[rows], gx3)
    for k in grads3:
        assert torch.equal(grads[k][rows], grads3[k]), k


# ---------------------------------------------------------------------------------------------------------------- 7: a long row
def test_a_row_whose_high_rate_length_passes_2_to_the_31():
    """One row-channel at F = 16 with L just above 2^27 + T, so F L > 2^31: the first and the last 3000 outputs against the
    float64 formula on the head / the tail of x alone (plus a halo of 64 base samples, far more than the
    (N_up + N_dn) / F = 25 a sample's output reaches; the halo's own outputs are cut off at its inner end)."""
    from grafx_amd import ops

    factor, n, halo = 16, 3000, 64
    L = (1 << 27) + _tile(factor) + 37
    assert factor * L > 1 << 31
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(1, 1, L, generator=gen, device="cuda") * 1.1 - 0.55
    pre = torch.full((1, 1), 0.7, device="cuda")
    h_up, o_up, h_dn, o_dn = o64.filters(factor)
    y = ops.oversampled_waveshaper(x, ops.WS_TANH, factor, h_up.cuda(), o_up, h_dn.cuda(), o_dn, pre, inverse_post_gain=True)
    cfg = dict(mode=o64.TANH, factor=factor, h_up=h_up, o_up=o_up, h_dn=h_dn, o_dn=o_dn, log_pre_gain=pre.double().cpu(),
               inverse_post_gain=True)
    head = o64.forward(x[..., :n + halo].double().cpu(), **cfg)[..., :n]
    tail = o64.forward(x[..., -(n + halo):].double().cpu(), **cfg)[..., -n:]
    assert_close(y[..., :n].cpu(), head, 1e-5, "first 3000 outputs")
    assert_close(y[..., -n:].cpu(), tail, 1e-5, "last 3000 outputs")


# ------------------------------------------------------------------------------------------------------------------ 8: modules
MODULES = ("tanh_b", "pw_a", "pow_a", "cheb_b")


@functools.lru_cache(maxsize=None)
def _module_case(tag, oversample, R=3, C=2, L=1500):
    import grafx_amd.processors as P

    cls, kw = NL[tag]
    m = getattr(P, cls)(oversample=oversample, **kw)
    gen = torch.Generator().manual_seed(11)
    x = torch.rand(R, C, L, generator=gen) * 1.1 - 0.55
    ps = {k: torch.randn(R, n, generator=gen) * 0.5 for k, n in m.parameter_size().items()}
    if "Tanh" not in cls and "log_pre_gain" in ps:
        ps["log_pre_gain"] = -ps["log_pre_gain"].abs()
    if cls == "PiecewiseTanhDistortion":
        ps["log_pre_gain"] = _past_the_thresholds(ps["log_pre_gain"])
    gy = torch.randn(R, C, L, generator=gen)
    x64 = x.double().requires_grad_()
    ps64 = {k: v.double().requires_grad_() for k, v in ps.items()}
    y64 = m.torch_forward(x64, **ps64)
    grads = torch.autograd.grad(y64, [x64, *ps64.values()], gy.double())
    return m, x, ps, gy, {"y": y64.detach(), "x": grads[0], **dict(zip(ps64, grads[1:]))}


@pytest.mark.parametrize("tag", MODULES)
def test_modules_match_their_torch_forward(tag):
    from grafx_amd.autograd import tape_only

    m, x, ps, gy, ref = _module_case(tag, 4)
    m = m.cuda()
    xg = x.cuda().requires_grad_()
    pg = {k: v.cuda().requires_grad_() for k, v in ps.items()}
    y = m(xg, **pg)
    assert_close(y.detach().cpu(), ref["y"], 1e-5, f"{tag}: output")
    grads = torch.autograd.grad(y, [xg, *pg.values()], gy.cuda())
    assert_close(grads[0].cpu(), ref["x"], 1e-5, f"{tag}: gx")
    for k, g in zip(pg, grads[1:]):
        assert g.shape == pg[k].shape
        assert_close(g.cpu(), ref[k], 1e-5, f"{tag}: d/d{k}")
    with torch.no_grad():                                                   # inference: the op itself, the same bits
        plain = m(x.cuda(), **{k: v.cuda() for k, v in ps.items()})
        assert torch.equal(plain, y.detach())
        # render_into: a strided (B, n, C, L) view in, another out
        R, C, L = x.shape
        xbuf, obuf = torch.zeros(1, R + 2, C, L + 1, device="cuda"), torch.full((1, R + 2, C, L + 1), 7.0, device="cuda")
        xbuf[:, 1:R + 1, :, :L].copy_(x.view(1, R, C, L))
        m.render_into(xbuf[:, 1:R + 1, :, :L], obuf[:, 2:R + 2, :, :L], **{k: v.cuda() for k, v in ps.items()})
        assert torch.equal(obuf[0, 2:R + 2, :, :L], plain)
    with tape_only():                                                       # the output's values are not computed; the tape is
        y2 = m(xg, **pg)
    grads2 = torch.autograd.grad(y2, [xg, *pg.values()], gy.cuda())
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("tag", MODULES)
def test_oversample_one_is_the_module_as_it_was(tag):
    from grafx_amd import ops
    from test_gpu_waveshaper_bwd import MODES, _ops_arguments

    m, x, ps, gy, ref = _module_case(tag, 1)
    m = m.cuda()
    args, names = _ops_arguments(m, NL[tag][0], ps)
    with torch.no_grad():
        y = m(x.cuda(), **{k: v.cuda() for k, v in ps.items()})
    assert torch.equal(y, ops.waveshaper(x.cuda(), **args))
    assert list(m.buffers()) == [] and MODES[NL[tag][0]] == args["mode"]
    xg = x.cuda().requires_grad_()
    pg = {k: v.cuda().requires_grad_() for k, v in ps.items()}
    grads = torch.autograd.grad(m(xg, **pg), [xg, *pg.values()], gy.cuda())
    gx, want = ops.waveshaper_bwd(x.cuda(), gy.cuda(), **args)
    assert torch.equal(grads[0], gx)
    for k, pname in names.items():
        assert torch.equal(grads[1 + list(pg).index(pname)].reshape(want[k].shape), want[k]), pname


def test_a_streamed_render_refuses_an_oversampled_node_before_any_launch():
    from grafx_amd.processors import TanhDistortion
    from grafx_amd.render import render_grafx
    from test_gpu_render_state import _chain_graph, _parameters, _render_data

    procs = {"distortion": TanhDistortion(oversample=4).cuda()}
    with pytest.raises(ValueError, match="oversample=4"):
        procs["distortion"].stream_check()
    G = _chain_graph(["in", "distortion", "out"])
    rd, params = _render_data(G), _parameters(procs, G, 5)
    x = 0.3 * torch.randn(2, 1, 2, 512, device="cuda")
    before = x.clone()
    with torch.no_grad(), pytest.raises(ValueError, match=r"'distortion'.*oversample=4"):
        render_grafx(procs, x, params, rd, return_state=True)
    assert torch.equal(x, before)
    with torch.no_grad():                                                   # one call renders it
        y = render_grafx(procs, x, params, rd)[0]
        want = procs["distortion"](x.view(2, 2, 512), **{k: v.expand(2, -1).contiguous() for k, v in params["distortion"].items()})
    assert_close(y.reshape(2, 2, 512).cpu(), want.double().cpu(), 1e-5, "one-call render of an oversampled node")


# -------------------------------------------------------------------------------------------------------------- 9: the purpose
def test_oversampling_removes_the_aliasing_it_is_for():
    """The tone of the issue through TanhDistortion(oversample=F) with log_pre_gain = 3: the alias share of the GPU's output
    is at most 1.1 x the float64 share at the same F (a 1e-5 peak-relative output error against an alias amplitude of
    1.6e-3 at F = 8 is about 1.2 % in energy), and eight-fold oversampling takes it below 1e-4 of the plain shaper's."""
    from grafx_amd.processors import TanhDistortion

    x, pre = o64.tone().cuda(), torch.full((1, 1), 3.0, device="cuda")
    share = {}
    for factor in (1, 2, 4, 8):
        with torch.no_grad():
            share[factor] = o64.alias_share(TanhDistortion(oversample=factor).cuda()(x, pre))
        want = o64.tone_share(factor)
        print(f"F={factor}: alias share {share[factor]:.4e} on the GPU, {want:.4e} in float64")
        assert share[factor] <= 1.1 * want, (factor, share[factor], want)
    assert share[8] < 1e-4 * share[1]


# ------------------------------------------------------------------------------------------------------------------ 10: memory
def test_training_keeps_no_signal_at_the_high_rate():
    """F = 8 on 64 x 2 x 65 536 samples (32 MiB): forward + backward through the module under autograd peaks below 4 x the
    bytes of x above the state that holds x and the parameters -- y, gy, gx and a workspace of kilobytes.  The composed
    route would hold u alone at 8 x."""
    from grafx_amd.processors import TanhDistortion

    R, C, L = 64, 2, 65536
    signal = R * C * L * 4
    m = TanhDistortion(oversample=8).cuda()
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(R, C, L, generator=gen) * 1.1 - 0.55).cuda().requires_grad_()
    pre = (torch.randn(R, 1, generator=gen) * 0.5).cuda().requires_grad_()
    torch.cuda.synchronize()
    start = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = m(x, pre)
    gy = torch.randn_like(y)
    grads = torch.autograd.grad(y, [x, pre], gy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - start
    print(f"peak above x and the parameters: {peak / signal:.2f} signals")
    assert grads[0].shape == x.shape and peak < 4 * signal, peak / signal
