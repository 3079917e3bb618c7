"""The native backward of the memoryless distortions (gfx_waveshaper_bwd_f32, ops.waveshaper_bwd, autograd.WaveshaperFn)
against float64 autograd of each class's torch_forward on the CPU, at the standing 1e-5 (peak-relative and relative L2).

Inputs: x uniform in [-0.9, 0.9]; parameters randn * 0.5; the polynomial shapers get log_pre_gain <= 0 (their bases are
conditioned on |u| <= 1).  On such inputs float32 autograd of the same formulas stays within 4.1e-6 of float64 (the pre-gain
gradient under inverse_post_gain, a cancellation), so 1e-5 leaves room and a miss is a kernel defect."""
import ctypes
import functools

import pytest
import torch

from conftest import assert_close
from test_gpu_next_rows2 import NL

pytestmark = pytest.mark.gpu

MODES = {"TanhDistortion": 0, "PiecewiseTanhDistortion": 1, "PowerDistortion": 2, "ChebyshevDistortion": 3}


def _module(name, kw):
    import grafx_amd.processors as P

    return getattr(P, name)(**dict(kw))


@functools.lru_cache(maxsize=None)
def _case(name, kw, R, C, L, seed=0):
    """(module, x, parameters, gy) on the CPU in float32 and the float64 reference {"y", "x", parameter names} -- computed
    once per case and shared; nothing modifies them."""
    m = _module(name, kw)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(R, C, L, generator=gen) * 1.8 - 0.9
    ps = {k: torch.randn(R, n, generator=gen) * 0.5 for k, n in m.parameter_size().items()}
    if MODES[name] >= 2 and "log_pre_gain" in ps:
        ps["log_pre_gain"] = -ps["log_pre_gain"].abs()
    gy = torch.randn(R, C, L, generator=gen)
    x64 = x.double().requires_grad_()
    ps64 = {k: v.double().requires_grad_() for k, v in ps.items()}
    y64 = m.torch_forward(x64, **ps64)
    leaves = [x64, *ps64.values()]
    grads = torch.autograd.grad(y64, leaves, gy.double(), allow_unused=True)     # (unused: x and the gain of a K = 1 basis)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, grads)]
    ref = {"y": y64.detach(), "x": grads[0], **dict(zip(ps64, grads[1:]))}
    return m, x, ps, gy, ref


def _ops_arguments(m, name, ps):
    """The processor's parameters as ops.waveshaper_bwd takes them -> (keywords, {ops name: parameter name})."""
    mode = MODES[name]
    pre_post = getattr(m, "pre_post_gain", getattr(m, "pre_gain", False))
    inverse = bool(mode < 2 and pre_post and m.inverse_post_gain)
    p0_name = {0: "bias", 1: "log_hardness", 2: "basis_weights", 3: "basis_weights"}[mode]
    names = {"log_pre_gain": "log_pre_gain", "log_post_gain": "log_post_gain", "p0": p0_name, "p1": "z_threshold"}
    names = {k: v for k, v in names.items() if v in ps}
    kw = {k: ps[v].cuda() for k, v in names.items()}
    kw.update(mode=mode, use_tanh=getattr(m, "use_tanh", False), inverse_post_gain=inverse, remove_dc=m.remove_dc)
    return kw, names


def _check(gx, grads, names, ref, what):
    if gx is not None:
        assert_close(gx.reshape(ref["x"].shape).cpu(), ref["x"], 1e-5, f"{what}: gx")
    assert set(grads) == set(names)
    for k, pname in names.items():
        assert_close(grads[k].reshape(ref[pname].shape).cpu(), ref[pname], 1e-5, f"{what}: d/d{pname}")


# ------------------------------------------------------------------------------------- the nine configurations, via forward
@pytest.mark.parametrize("tag", sorted(NL))
def test_processor_gradients_match_float64(tag):
    name, kw = NL[tag]
    m, x, ps, gy, ref = _case(name, tuple(sorted(kw.items())), 3, 2, 4099)
    xg = x.cuda().requires_grad_()
    pg = {k: v.cuda().requires_grad_() for k, v in ps.items()}
    y = m.cuda()(xg, **pg)
    assert_close(y.detach().cpu(), ref["y"], 1e-5, f"{tag}: output")
    grads = torch.autograd.grad(y, [xg, *pg.values()], gy.cuda())
    assert_close(grads[0].cpu(), ref["x"], 1e-5, f"{tag}: gx")
    for k, g in zip(pg, grads[1:]):
        assert g.shape == pg[k].shape
        assert_close(g.cpu(), ref[k], 1e-5, f"{tag}: d/d{k}")


# ------------------------------------------------------------------------------------------------------- polynomial orders
@pytest.mark.parametrize("use_tanh", [False, True])
@pytest.mark.parametrize("K", [1, 2, 10, 32])
@pytest.mark.parametrize("name", ["PowerDistortion", "ChebyshevDistortion"])
def test_polynomial_orders(name, K, use_tanh):
    from grafx_amd import ops

    kw = (("max_order", K), ("pre_gain", True), ("remove_dc", False), ("use_tanh", use_tanh))
    m, x, ps, gy, ref = _case(name, kw, 3, 2, 4099)
    args, names = _ops_arguments(m, name, ps)
    out = torch.full((3, 2, 4099), float("nan"), device="cuda")
    gx, grads = ops.waveshaper_bwd(x.cuda(), gy.cuda(), out=out, **args)
    assert gx is out and not torch.isnan(out).any()          # (K = 1: s' = 0, written as zeros)
    if K == 1:
        assert torch.equal(out, torch.zeros_like(out)) and torch.equal(grads["log_pre_gain"], torch.zeros(3, 1, device="cuda"))
    _check(gx, grads, names, ref, f"{name} K={K} tanh={use_tanh}")


def test_polynomial_with_a_post_gain():
    """The C entry takes a post gain in every mode, as the forward does (no processor class uses it with a polynomial)."""
    from grafx_amd import ops

    kw = (("max_order", 7), ("pre_gain", True), ("remove_dc", True), ("use_tanh", True))
    m, x, ps, gy, _ = _case("ChebyshevDistortion", kw, 3, 2, 4099)
    gen = torch.Generator().manual_seed(5)
    post = torch.randn(3, 1, generator=gen) * 0.5
    for inverse in (False, True):
        x64, post64 = x.double().requires_grad_(), post.double().requires_grad_()
        ps64 = {k: v.double().requires_grad_() for k, v in ps.items()}
        y64 = m.torch_forward(x64, **ps64)
        y64 = y64 / torch.exp(ps64["log_pre_gain"]).unsqueeze(-1) if inverse else y64 * torch.exp(post64).unsqueeze(-1)
        wrt = [x64, ps64["basis_weights"], ps64["log_pre_gain"]] + ([] if inverse else [post64])
        want = torch.autograd.grad(y64, wrt, gy.double())
        gx, grads = ops.waveshaper_bwd(x.cuda(), gy.cuda(), ops.WS_CHEBYSHEV, ps["log_pre_gain"].cuda(),
                                       None if inverse else post.cuda(), p0=ps["basis_weights"].cuda(), use_tanh=True,
                                       inverse_post_gain=inverse, remove_dc=True)
        assert_close(gx.cpu(), want[0], 1e-5, f"inverse={inverse}: gx")
        assert_close(grads["p0"].cpu(), want[1], 1e-5, f"inverse={inverse}: d/dbasis_weights")
        assert_close(grads["log_pre_gain"].cpu(), want[2], 1e-5, f"inverse={inverse}: d/dlog_pre_gain")
        if not inverse:
            assert_close(grads["log_post_gain"].cpu(), want[3], 1e-5, "d/dlog_post_gain")


# ---------------------------------------------------------------------------------------------- small and misaligned shapes
def _off_by_one_float(t):
    """A copy of t on the GPU whose first element lies one float past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 5, device="cuda")
    shift = 1 + (-(flat.data_ptr() // 4) % 4)
    v = flat[shift : shift + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("misaligned", ["none", "x", "gy", "gx"])
@pytest.mark.parametrize("L", [1, 3, 5, 64])
@pytest.mark.parametrize("tag", ["pw_b", "cheb_a"])
def test_small_and_misaligned_shapes(tag, L, misaligned):
    """C = 1, rows of 1, 3, 5 samples (scalar path, fewer samples than lanes) and of 64 (the 16-byte path unless one of the
    three signals starts off a 16-byte boundary)."""
    from grafx_amd import ops

    name, kw = NL[tag]
    m, x, ps, gy, ref = _case(name, tuple(sorted(kw.items())), 3, 1, L, seed=L)
    args, names = _ops_arguments(m, name, ps)
    xg = _off_by_one_float(x) if misaligned == "x" else x.cuda()
    gg = _off_by_one_float(gy) if misaligned == "gy" else gy.cuda()
    out = torch.full((3, 1, L), float("nan"))
    out = _off_by_one_float(out) if misaligned == "gx" else out.cuda()
    gx, grads = ops.waveshaper_bwd(xg, gg, out=out, **args)
    _check(gx, grads, names, ref, f"{tag} L={L} misaligned={misaligned}")


# --------------------------------------------------------------------------------------------------- many workgroups per row
@pytest.mark.parametrize("tag", ["pw_b", "cheb_a"])
def test_many_workgroups_per_row_and_bitwise_repeatability(tag):
    """L = 70 001: all 64 workgroups of a row hold partial sums; two runs give the same bits (stored partials summed in a
    fixed order, no float atomics)."""
    from grafx_amd import ops

    name, kw = NL[tag]
    m, x, ps, gy, ref = _case(name, tuple(sorted(kw.items())), 2, 2, 70001)
    args, names = _ops_arguments(m, name, ps)
    xg, gg = x.cuda(), gy.cuda()
    gx, grads = ops.waveshaper_bwd(xg, gg, **args)
    gx2, grads2 = ops.waveshaper_bwd(xg, gg, **args)
    _check(gx, grads, names, ref, tag)
    assert torch.equal(gx, gx2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


# ----------------------------------------------------------------------------------------------------------------- many rows
@pytest.mark.parametrize("tag", ["tanh_b", "cheb_a"])
def test_more_rows_than_one_launch_grid(tag):
    from grafx_amd import ops

    name, kw = NL[tag]
    m, x, ps, gy, ref = _case(name, tuple(sorted(kw.items())), 65539, 1, 8)
    args, names = _ops_arguments(m, name, ps)
    gx, grads = ops.waveshaper_bwd(x.cuda(), gy.cuda(), **args)
    _check(gx, grads, names, ref, f"{tag}: 65 539 rows")


# ------------------------------------------------------------------------------------------------------ strided buffer views
@pytest.mark.parametrize("tag", ["tanh_b", "pw_a", "pow_b", "cheb_a"])
def test_strided_views_of_render_buffers(tag):
    """x and gy as (B, n, C, L) views of one larger buffer each, gx into a view of a third.  The buffers' rows are L + 1 long:
    every row starts on a 16-byte boundary and ends in a tail of three samples.  Nothing outside the views is touched."""
    from grafx_amd import ops

    B, n, C, L = 2, 3, 2, 4099
    name, kw = NL[tag]
    m, x, ps, gy, ref = _case(name, tuple(sorted(kw.items())), B * n, C, L)
    args, names = _ops_arguments(m, name, ps)
    xbuf = torch.full((B, 7, C, L + 1), 3.0, device="cuda")
    gbuf = torch.full((B, 6, C, L + 1), 5.0, device="cuda")
    obuf = torch.full((B, 8, C, L + 1), 7.0, device="cuda")
    xv, gv, ov = xbuf[:, 2:5, :, :L], gbuf[:, 1:4, :, :L], obuf[:, 4:7, :, :L]
    xv.copy_(x.view(B, n, C, L))
    gv.copy_(gy.view(B, n, C, L))
    xkeep, gkeep = xbuf.clone(), gbuf.clone()
    gx, grads = ops.waveshaper_bwd(xv, gv, out=ov, **args)
    assert gx is ov
    _check(gx, grads, names, ref, f"{tag}: strided views")
    assert torch.equal(xbuf, xkeep) and torch.equal(gbuf, gkeep)
    outside = torch.ones_like(obuf, dtype=torch.bool)
    outside[:, 4:7, :, :L] = False
    assert torch.equal(obuf[outside], torch.full_like(obuf[outside], 7.0))
    # two node ranges of ONE buffer interleave in memory without sharing an element: x and gx may be such a pair
    both = torch.full((B, 8, C, L + 1), 7.0, device="cuda")
    both[:, 0:3, :, :L].copy_(x.view(B, n, C, L))
    gx, _ = ops.waveshaper_bwd(both[:, 0:3, :, :L], gv, out=both[:, 3:6, :, :L], want=("x",), **args)
    assert_close(gx.reshape(B * n, C, L).cpu(), ref["x"], 1e-5, f"{tag}: x and gx in one buffer")


# -------------------------------------------------------------------------------------------------------------------- options
def test_remove_dc_makes_the_input_gradient_blind_to_a_constant_offset():
    """With remove_dc a constant added to x changes nothing, so gx sums to zero over every row-channel.  Bound: the L
    subtractions of the mean round by at most eps / 2 of each |gx|, and the mean itself comes from float partial sums of a
    few terms each, added in double -- together under 1e-6 of sum |gx|."""
    from grafx_amd import ops

    name, kw = NL["tanh_b"]
    m, x, ps, gy, ref = _case(name, tuple(sorted(kw.items())), 3, 2, 4099)
    args, names = _ops_arguments(m, name, ps)
    gx, _ = ops.waveshaper_bwd(x.cuda(), gy.cuda(), **args)
    total, scale = gx.double().sum(-1).abs(), gx.double().abs().sum(-1)
    assert (total <= 1e-6 * scale).all(), (total / scale).max()
    # the means handed over by the forward are the ones the backward would recompute
    y, dc = ops.waveshaper(x.cuda(), **{k: v for k, v in args.items()}, return_dc=True)
    assert dc.shape == (6,) and torch.equal(dc, ops.row_mean(x.cuda()))
    gx2, _ = ops.waveshaper_bwd(x.cuda(), gy.cuda(), dc=dc, **args)
    assert torch.equal(gx, gx2)
    assert_close(y.cpu(), ref["y"], 1e-5, "forward with return_dc")


@pytest.mark.parametrize("tag", ["tanh_b", "pw_b", "cheb_b"])
def test_only_some_gradients(tag):
    from grafx_amd import ops

    name, kw = NL[tag]
    m, x, ps, gy, ref = _case(name, tuple(sorted(kw.items())), 3, 2, 4099)
    args, names = _ops_arguments(m, name, ps)
    gx, grads = ops.waveshaper_bwd(x.cuda(), gy.cuda(), want=tuple(names), **args)       # parameters only
    assert gx is None
    _check(None, grads, names, ref, f"{tag}: parameters only")
    gx, grads = ops.waveshaper_bwd(x.cuda(), gy.cuda(), want=("x",), **args)               # input only
    assert grads == {}
    _check(gx, grads, {}, ref, f"{tag}: gx only")
    one = sorted(names)[0]
    gx, grads = ops.waveshaper_bwd(x.cuda(), gy.cuda(), want=(one,), **args)               # one parameter
    assert gx is None
    _check(None, grads, {one: names[one]}, ref, f"{tag}: {one} only")


# -------------------------------------------------------------------------------------------------------------- the C entry
def test_c_entry_refuses_aliasing_and_missing_arguments():
    from grafx_amd import _lib, ops

    lib = _lib.lib()
    R, C, L = 2, 2, 64
    x, gy, gx = (torch.zeros(R, C, L, device="cuda") for _ in range(3))
    pre, gpre = torch.zeros(R, device="cuda"), torch.zeros(R, device="cuda")
    ws = torch.empty(lib.gfx_waveshaper_bwd_ws_bytes(R, C, L, 0), dtype=torch.uint8, device="cuda")
    assert ws.numel() == 4 * (R * 6 * 1 + R * C * 1 + R * C)
    assert lib.gfx_waveshaper_bwd_ws_bytes(8192, 2, 131072, 10) == 4 * (8192 * 12 * 64 + 8192 * 2 * 64 + 8192 * 2)
    rm = ops.rowmap(x)[0]

    def call(x=x, gy=gy, gx=gx, gpre=gpre, pre=pre, ws=ws, mode=0, gp1=None, inverse=0, gpost=None, p0=None, K=0):
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        return lib.gfx_waveshaper_bwd_f32(ptr(x), rm, ptr(gy), rm, R, C, L, mode, 0, inverse, ptr(pre), None, ptr(p0), None, K,
                                          None, ptr(gx), rm, ptr(gpre), ptr(gpost), None, ptr(gp1), ptr(ws),
                                          0 if ws is None else ws.numel(), None)

    assert call() == 0
    assert call(gx=x) == ops.GFX_EINVAL and call(gx=gy) == ops.GFX_EINVAL          # gx aliases an input
    assert call(gx=x[:, :, 1:]) == ops.GFX_EINVAL                                    # ... or overlaps one, a sample later
    assert call(x=None) == ops.GFX_EINVAL and call(gy=None) == ops.GFX_EINVAL
    assert call(gx=None, gpre=None) == ops.GFX_EINVAL                                # nothing asked for
    assert call(pre=None) == ops.GFX_EINVAL                                          # a gradient of a missing parameter
    assert call(gp1=gpre) == ops.GFX_EINVAL                                          # z_threshold outside the piecewise mode
    assert call(inverse=1, gpost=gpre) == ops.GFX_EINVAL                             # post gain unused under inverse_post_gain
    assert call(mode=1) == ops.GFX_EINVAL and call(mode=7) == ops.GFX_EINVAL         # piecewise without its parameters
    assert call(mode=3, p0=pre, K=33) == ops.GFX_EINVAL and call(mode=3, K=4) == ops.GFX_EINVAL
    assert call(ws=None) == ops.GFX_EINVAL and call(ws=ws[:8]) == -2                 # GFX_ENOSPC
    assert call(gpre=None, ws=None) == 0                                             # only gx, no dc: no workspace needed
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------------- memory
def test_backward_keeps_no_full_size_terms():
    """ChebyshevDistortion(16, tanh) on 32 stereo rows of 65 536 samples (16 MiB of signal): the native node's backward
    peaks at most 3 signals above the starting allocation (y, gx, one of slack for workspace and allocator rounding); the
    torch twin holds K = 16 materialised terms and exceeds 8 -- the measurement sees what it claims."""
    import grafx_amd.processors as P

    R, C, L, K = 32, 2, 65536, 16
    signal = R * C * L * 4
    m = P.ChebyshevDistortion(max_order=K, use_tanh=True).cuda()
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(R, C, L, generator=gen) * 1.8 - 0.9).cuda().requires_grad_()
    ps = {"basis_weights": (torch.randn(R, K, generator=gen) * 0.5).cuda().requires_grad_(),
          "log_pre_gain": (-(torch.randn(R, 1, generator=gen) * 0.5).abs()).cuda().requires_grad_()}
    gy = torch.randn(R, C, L, generator=gen).cuda()

    def peak_above_start(forward):
        torch.cuda.synchronize()
        start = torch.cuda.memory_allocated()
        y = forward(x, **ps)
        torch.cuda.reset_peak_memory_stats()
        grads = torch.autograd.grad(y, [x, *ps.values()], grad_outputs=gy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - start, grads

    native, g_native = peak_above_start(m)
    del g_native
    twin, g_twin = peak_above_start(m.torch_forward)
    del g_twin
    print(f"peak above start: native {native / signal:.2f} signals, torch twin {twin / signal:.2f} signals")
    assert native <= 3 * signal, native / signal
    assert twin > 8 * signal, twin / signal
