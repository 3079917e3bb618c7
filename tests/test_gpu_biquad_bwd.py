"""The one-pass native backward of the exact biquad cascade (gfx_biquad_cascade_bwd_f32, ops.biquad_cascade_bwd,
autograd.BiquadCascadeFn / BiquadCascadeStateFn).

The yardstick is torch autograd in float64 through the plain direct-form-II loop `df2` of test_gpu_recursive_iir_state.py
(that file explains why it is the pin).  The error of a gradient tensor is max |got - want| / max |want|, the bound the
project's GRAD_TOL = 2e-4.  One exception, written down where it is made (`check`): a gradient whose float64 value lies
below float32's normal range everywhere has no relative error to speak of and is held to be as small instead.  And one
premise (`float32_attains`): the random inputs of a case are drawn again when float32 autograd through the same loop on
the CPU is itself not within half the bound under the state-only loss -- decided by that loop alone, before the kernel runs;
the shapes it happens on are pinned (REDRAWS: one)."""
import functools

import pytest
import torch

from test_gpu_recursive_iir_state import GRAD_TOL, coeffs, df2

pytestmark = pytest.mark.gpu
NAMES = ("x", "Bs", "As", "zi")
TINY = 1e-30     # float32's smallest normal number is 1.2e-38: below this scale a float32 result has lost its digits


def grad_err(got, want):
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max()).item()


def check(what, names, got, want, tol=GRAD_TOL):
    """Every gradient tensor within ``tol``.  A state cotangent alone reaches zi only through r^L (r the pole radius): at
    L = 1537 that is 1e-36 and less in float64 and next to nothing in float32, and the numerator of a single section is not
    reached by it at all (exactly zero): such a tensor is required to be below TINY too."""
    for name, g, w in zip(names, got, want):
        assert g is not None and tuple(g.shape) == tuple(w.shape), f"{what}: grad {name} {None if g is None else g.shape}"
        assert torch.isfinite(g).all(), f"{what}: grad {name} is not finite"
        if w.abs().max() < TINY:
            assert g.abs().max() < 2 * TINY, f"{what}: grad {name} should vanish, got {g.abs().max().item():.2e}"
            continue
        err = grad_err(g, w)
        print(f"{what}: grad {name} {err:.2e}")
        assert err <= tol, f"{what}: grad {name} {err:.2e} > {tol:g}"


def reference_grads(x, Bs, As, zi, p, q):
    """float64 autograd through df2 -> the gradients of (x, Bs, As[, zi]): from silence (zi None) one tuple for the loss
    <y, p>; from a state three, for <y, p> + <zf, q>, for <y, p> alone and for <zf, q> alone."""
    leaves = [t.double().requires_grad_(True) for t in ((x, Bs, As) if zi is None else (x, Bs, As, zi))]
    y, zf, _ = df2(*leaves)
    out = []
    losses = [(p, q)] if zi is None else [(p, None), (None, q)]
    for i, (pp, qq) in enumerate(losses):
        loss = 0.0
        if pp is not None:
            loss = loss + (y * pp.double()).sum()
        if qq is not None:
            loss = loss + (zf * qq.double()).sum()
        grads = torch.autograd.grad(loss, leaves, retain_graph=i + 1 < len(losses), allow_unused=True)
        # (a leaf the loss does not reach -- the numerator of a single section under a state-only loss -- has gradient zero)
        out.append(tuple(torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)))
    if zi is not None:      # the gradient is linear in the cotangents: both terms = the sum of the two
        out.insert(0, tuple(a + b for a, b in zip(*out)))
    return out


def loop(x, Bs, As, zi):
    """df2's recursion in the dtype of its arguments (df2 itself computes in float64 whatever it is given)."""
    R, C, L = x.shape
    Cf, K = Bs.shape[1], Bs.shape[2]
    Co = max(C, Cf)
    y, zf = x.expand(R, Co, L), []
    for k in range(K):
        b = (Bs[:, :, k] / As[:, :, k, :1]).expand(R, Co, 3)
        a = (As[:, :, k] / As[:, :, k, :1]).expand(R, Co, 3)
        w1, w2, out = zi[:, :, k, 0], zi[:, :, k, 1], []
        for n in range(L):
            w = y[..., n] - a[..., 1] * w1 - a[..., 2] * w2
            out.append(b[..., 0] * w + b[..., 1] * w1 + b[..., 2] * w2)
            w2, w1 = w1, w
        y = torch.stack(out, -1)
        zf.append(torch.stack([w1, w2], -1))
    return y, torch.stack(zf, 2)


def float32_attains(x, Bs, As, zi, q, want, tol):
    """The premise of the bound on a draw: float32 autograd through the same loop on the CPU -- the reference's own float32
    error, nothing of the kernel -- is within ``tol`` of float64 for the state-only loss.  That loss reaches the early samples
    and zi only through r^L, the far tail of the recursion, whose phase every float32 evaluation gets wrong by about
    L eps / tan(theta): the a0-normalised coefficients are rounded before the first sample is filtered.  With a pole at 0.93
    and 2.93 rad and L = 513 the float32 loop is 3.2e-4 from float64 on dL/dzi: no float32 recursion meets 2e-4 there."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, Bs, As, zi)]
    grads = torch.autograd.grad((loop(*leaves)[1] * q).sum(), leaves, allow_unused=True)
    return all(w.abs().max() < TINY or (g is not None and grad_err(g, w) <= tol) for g, w in zip(grads, want))


# The shapes whose first draw float32 itself does not attain, and how many draws each discards.  Pinned: a case that needs
# another number of draws fails, so worse conditioning cannot hide behind more redraws.
REDRAWS = {(2, 2, 3, 513): 1}


@functools.lru_cache(maxsize=None)
def case(C, Cf, K, L):
    """The inputs and float64 gradients of one shape.  A draw on which float32 itself is not within half the bound
    (float32_attains) is drawn again: the bound can only be asked where the number format attains it.  REDRAWS holds how
    often that happens, shape by shape."""
    R, Co = 3, max(C, Cf)
    allowed = REDRAWS.get((C, Cf, K, L), 0)
    for draw in range(allowed + 1):
        torch.manual_seed(1000 * K + 100 * C + 10 * Cf + L + 10000 * draw)
        x = torch.randn(R, C, L)
        Bs, As = coeffs(R, Cf, K, seed=7 * K + 3 * C + Cf + L + 10000 * draw)
        zi = torch.randn(R, Co, K, 2)
        p, q = torch.randn(R, Co, L), torch.randn(R, Co, K, 2)
        both, y_only, zf_only = reference_grads(x, Bs, As, zi, p, q)
        attained = float32_attains(x, Bs, As, zi, q, zf_only, GRAD_TOL / 2)
        assert attained == (draw == allowed), \
            f"C={C}/{Cf} K={K} L={L}: draw {draw} is {'within' if attained else 'beyond'} float32, REDRAWS says {allowed} redraws"
    silent = reference_grads(x, Bs, As, None, p, None)[0]
    return x, Bs, As, zi, p, q, silent, both, y_only, zf_only


@pytest.mark.parametrize("L", [1, 2, 7, 512, 513, 1000, 1537])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("C,Cf", [(2, 1), (1, 2), (2, 2), (1, 1)])
def test_gradients_against_float64_autograd(C, Cf, K, L):
    from grafx_amd.autograd import BiquadCascadeFn, BiquadCascadeStateFn

    x, Bs, As, zi, p, q, silent, both, y_only, zf_only = case(C, Cf, K, L)
    what = f"C={C}/{Cf} K={K} L={L}"
    pc, qc = p.cuda(), q.cuda()

    ours = [t.cuda().requires_grad_(True) for t in (x, Bs, As)]
    (BiquadCascadeFn.apply(*ours) * pc).sum().backward()
    check(what + " from silence", NAMES[:3], [t.grad for t in ours], silent)

    for label, want, use_y, use_zf in (("y and zf", both, True, True), ("y only", y_only, True, False),
                                       ("zf only", zf_only, False, True)):
        ours = [t.cuda().requires_grad_(True) for t in (x, Bs, As, zi)]
        y, zf = BiquadCascadeStateFn.apply(*ours)
        loss = ((y * pc).sum() if use_y else 0.0) + ((zf * qc).sum() if use_zf else 0.0)
        loss.backward()
        check(f"{what} from a state, {label}", NAMES, [t.grad for t in ours], want)


# ------------------------------------------------------------------------------------------------- long cascade
@functools.lru_cache(maxsize=None)
def long_case():
    torch.manual_seed(32)
    R, C, K, L = 2, 2, 32, 520
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, C, K, seed=320, equaliser=True)
    zi = 0.1 * torch.randn(R, C, K, 2)
    p, q = torch.randn(R, C, L), torch.randn(R, C, K, 2)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in (x, Bs, As, zi)]
        y, zf = loop(*leaves)
        if dtype == torch.float64:     # the loop above IS df2
            y2, zf2, _ = df2(x, Bs, As, zi)
            assert torch.equal(y.detach(), y2) and torch.equal(zf.detach(), zf2)
        grads[dtype] = torch.autograd.grad((y * p.to(dtype)).sum() + (zf * q.to(dtype)).sum(), leaves)
    return x, Bs, As, zi, p, q, grads[torch.float64], grads[torch.float32]


def test_long_cascade_of_32_equaliser_sections():
    """K = 32 sections, L = 520 (a ragged second tile): the bound is 2e-4 or twice what float32 autograd through the same
    loop on the CPU is from float64, whichever is larger -- the kernel must be as close to float64 as float32 allows.
    Measured on the MI355X (EXPERIMENTS.md, "Biquad cascade backward"), kernel / float32 loop: x 5.30e-07 / 4.30e-07,
    Bs 3.24e-07 / 9.78e-07, As 6.22e-07 / 8.31e-07, zi 7.45e-07 / 3.17e-07.  Both are printed by this test."""
    from grafx_amd.autograd import BiquadCascadeStateFn

    x, Bs, As, zi, p, q, want, cpu32 = long_case()
    ours = [t.cuda().requires_grad_(True) for t in (x, Bs, As, zi)]
    y, zf = BiquadCascadeStateFn.apply(*ours)
    ((y * p.cuda()).sum() + (zf * q.cuda()).sum()).backward()
    bad = []
    for name, got, w64, w32 in zip(NAMES, ours, want, cpu32):
        err, noise = grad_err(got.grad, w64), grad_err(w32, w64)
        print(f"K=32 L=520 grad {name}: kernel {err:.2e}, float32 loop on the CPU {noise:.2e} (both against float64)")
        if not err <= max(GRAD_TOL, 2 * noise):
            bad.append(f"grad {name}: kernel {err:.2e} vs float32 loop {noise:.2e}")
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------- the direct call
@functools.lru_cache(maxsize=None)
def direct_case():
    """(B, n) = (2, 3) rows, C = 2, Cf = 1, K = 3, L = 700 on the GPU, with the full call's results."""
    from grafx_amd import ops

    torch.manual_seed(5)
    B, n, C, K, L = 2, 3, 2, 3, 700
    x, gy = torch.randn(B * n, C, L).cuda(), torch.randn(B * n, C, L).cuda()
    Bs, As = (t.cuda() for t in coeffs(B * n, 1, K, seed=51))
    zi, gzf = torch.randn(B * n, C, K, 2).cuda(), torch.randn(B * n, C, K, 2).cuda()
    full = ops.biquad_cascade_bwd(x, gy, Bs, As, zi=zi, gzf=gzf)
    return (B, n, C, K, L), x, gy, Bs, As, zi, gzf, full


def test_direct_call_matches_float64():
    (B, n, C, K, L), x, gy, Bs, As, zi, gzf, full = direct_case()
    want = reference_grads(x.cpu(), Bs.cpu(), As.cpu(), zi.cpu(), gy.cpu(), gzf.cpu())[0]
    check("ops.biquad_cascade_bwd", NAMES, full, want)


@pytest.mark.parametrize("name", NAMES)
def test_each_gradient_alone(name):
    from grafx_amd import ops

    _, x, gy, Bs, As, zi, gzf, full = direct_case()
    got = ops.biquad_cascade_bwd(x, gy, Bs, As, zi=zi, gzf=gzf, want=(name,))
    for other, g, f in zip(NAMES, got, full):
        if other == name:
            assert torch.equal(g, f), f"want=({name!r},): not the bits of the full call"
        else:
            assert g is None, f"want=({name!r},): {other} was returned too"
    with pytest.raises(ValueError):
        ops.biquad_cascade_bwd(x, gy, Bs, As, want=())
    with pytest.raises(ValueError):
        ops.biquad_cascade_bwd(x, gy, Bs, As, want=("y",))


def test_two_calls_give_equal_bits():
    from grafx_amd import ops

    _, x, gy, Bs, As, zi, gzf, full = direct_case()
    again = ops.biquad_cascade_bwd(x, gy, Bs, As, zi=zi, gzf=gzf)
    for name, a, b in zip(NAMES, again, full):
        assert torch.equal(a, b), f"grad {name} differs between two calls"


def test_strided_views_of_a_nan_filled_buffer_with_an_unaligned_start():
    from grafx_amd import ops

    (B, n, C, K, L), x, gy, Bs, As, zi, gzf, full = direct_case()
    buf = torch.full((B, 11, C, L + 5), float("nan"), device="cuda")
    xv, gv, ov = buf[:, 1:4, :, 1:L + 1], buf[:, 4:7, :, 1:L + 1], buf[:, 7:10, :, 1:L + 1]
    assert xv.data_ptr() % 16 != 0 and gv.data_ptr() % 16 != 0 and ov.data_ptr() % 16 != 0
    xv.copy_(x.view(B, n, C, L))
    gv.copy_(gy.view(B, n, C, L))
    before = buf.clone()
    gx, gB, gA, gzi = ops.biquad_cascade_bwd(xv, gv, Bs, As, zi=zi, gzf=gzf, out=ov)
    assert gx.data_ptr() == ov.data_ptr()
    for name, got, want in zip(NAMES, (ov.reshape(B * n, C, L), gB, gA, gzi), full):
        assert torch.equal(got, want), f"strided views: grad {name} is not the contiguous call's"
    after = buf.clone()
    after[:, 7:10, :, 1:L + 1] = float("nan")
    assert torch.equal(after.isnan(), before.isnan()), "something outside the view of out was written"
    assert torch.equal(torch.nan_to_num(after), torch.nan_to_num(before)), "x or gy changed"
    # the kernel's vector path (16-byte aligned rows) gives the same bits
    wide = torch.full((B, 11, C, L + 4), float("nan"), device="cuda")
    xa, ga, oa = wide[:, 1:4, :, :L], wide[:, 4:7, :, :L], wide[:, 7:10, :, :L]
    assert xa.data_ptr() % 16 == 0 and L % 4 == 0
    xa.copy_(x.view(B, n, C, L))
    ga.copy_(gy.view(B, n, C, L))
    ops.biquad_cascade_bwd(xa, ga, Bs, As, zi=zi, gzf=gzf, out=oa, want=("x",))
    assert torch.equal(oa.reshape(B * n, C, L), full[0]) and wide[..., L:].isnan().all() and wide[:, 10].isnan().all()


def test_overlapping_destinations_and_a_short_workspace_are_refused_with_everything_unchanged():
    from grafx_amd import ops

    (B, n, C, K, L), x, gy, Bs, As, zi, gzf, _ = direct_case()
    buf = torch.randn(B, 8, C, L, device="cuda")
    before = buf.clone()
    xv, gv = buf[:, 0:3], buf[:, 3:6]
    for label, out in (("out is x", xv), ("out is gy", gv), ("out over x's shifted range", buf[:, 2:5]),
                       ("out over gy's shifted range", buf[:, 5:8])):
        with pytest.raises(ValueError, match="must not share memory"):
            ops.biquad_cascade_bwd(xv, gv, Bs, As, out=out)
        assert torch.equal(buf, before), label
    need = ops.biquad_cascade_bwd_ws_bytes(B * n, C, K, L)
    short = torch.zeros(need - 1, dtype=torch.uint8, device="cuda")
    out = torch.full((B * n, C, L), 7.0, device="cuda")
    with pytest.raises(ValueError, match="workspace"):
        ops.biquad_cascade_bwd(x, gy, Bs, As, out=out, ws=short)
    assert not short.any() and (out == 7.0).all()
    with pytest.raises(ValueError, match="must not share memory"):
        ops.biquad_cascade_bwd(x, gy, Bs, As, ws=x.view(torch.uint8).reshape(-1))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    got = ops.biquad_cascade_bwd(x, gy, Bs, As, zi=zi, gzf=gzf, ws=ws)
    for name, a, b in zip(NAMES, got, direct_case()[-1]):
        assert torch.equal(a, b), f"a caller's workspace: grad {name}"


# ------------------------------------------------------------------------------------------------- many rows
@pytest.mark.parametrize("K,C,Cf", [(1, 1, 1), (3, 1, 2), (3, 2, 1)])
def test_rows_beyond_the_grid_edge(K, C, Cf):
    """65 601 rows (an odd count: with one channel the last pair has no partner) of 64 samples against the float64 loop, every
    row by its own peak, and slices of 16 384 rows -- even starts, the same pairs -- give the bits of the big call."""
    from grafx_amd import ops

    torch.manual_seed(K + 2 * C + 4 * Cf)
    R, L, Co = 65601, 64, max(C, Cf)
    x, gy = torch.randn(R, C, L), torch.randn(R, Co, L)
    Bs, As = coeffs(R, Cf, K, seed=90 + K, rmax=0.9)
    zi, gzf = torch.randn(R, Co, K, 2), torch.randn(R, Co, K, 2)
    want = reference_grads(x, Bs, As, zi, gy, gzf)[0]
    dev = [t.cuda() for t in (x, gy, Bs, As, zi, gzf)]
    big = ops.biquad_cascade_bwd(*dev[:4], zi=dev[4], gzf=dev[5])
    for name, g, w in zip(NAMES, big, want):
        assert torch.isfinite(g).all(), name
        d = (g.cpu().double() - w).reshape(R, -1).abs().amax(1) / w.reshape(R, -1).abs().amax(1)
        print(f"K={K} C={C}/{Cf} grad {name}: worst row {d.max().item():.2e} (row {d.argmax().item()})")
        assert d.max() <= GRAD_TOL, f"grad {name}: row {d.argmax().item()} is {d.max().item():.2e} from float64"
    for sl in (slice(0, 16384), slice(65535 - 8192, 65535 + 8192), slice(R - 16384, R)):
        sl = slice(sl.start - sl.start % 2, sl.stop)
        part = ops.biquad_cascade_bwd(*(t[sl] for t in dev[:4]), zi=dev[4][sl], gzf=dev[5][sl])
        for name, a, b in zip(NAMES, part, big):
            assert torch.equal(a, b[sl]), f"grad {name}: rows {sl.start}..{sl.stop} differ from the big call"


# ------------------------------------------------------------------------------------------------- streams
def test_consumer_order_on_a_side_stream():
    """x and gy are filled late on the side stream: the call made there must read them, and give the default stream's bits."""
    from grafx_amd import ops
    from stream_order import mismatches, ordered_call

    _, x, gy, Bs, As, zi, gzf, full = direct_case()
    ops.biquad_cascade_bwd(x, gy, Bs, As, zi=zi, gzf=gzf)          # warm: code objects loaded, attributes set
    x_late, gy_late = torch.randn_like(x), torch.randn_like(gy)
    got = ordered_call(lambda: ops.biquad_cascade_bwd(x_late, gy_late, Bs, As, zi=zi, gzf=gzf),
                       [(x_late, x), (gy_late, gy)], label="biquad_cascade_bwd")
    assert not mismatches(got, full), mismatches(got, full)


# ------------------------------------------------------------------------------------------------- the Functions
def test_training_output_is_the_inference_output():
    from grafx_amd import ops
    from grafx_amd.processors import IIRFilter

    torch.manual_seed(6)
    x = torch.randn(3, 2, 1000).cuda()
    Bs, As = (t.cuda() for t in coeffs(3, 2, 3, seed=61))
    m = IIRFilter(order=2, backend="lfilter", flashfftconv=False)
    y = m(x.clone().requires_grad_(), Bs, As)
    assert y.requires_grad and torch.equal(y, ops.biquad_cascade(x, Bs, As))
    zi = torch.randn(3, 2, 3, 2).cuda()
    y, zf = m(x, Bs.clone().requires_grad_(), As, state=zi, return_state=True)
    y0, zf0 = ops.biquad_cascade(x, Bs, As, zi=zi, return_state=True)
    assert y.requires_grad and zf.requires_grad and torch.equal(y, y0) and torch.equal(zf, zf0)


def test_the_tape_holds_no_section_outputs():
    """Forward and backward of an 8-section cascade allocate y, gx and less than one more signal tensor (the workspace, the
    coefficient gradients, allocator rounding); one saved tensor per section would be 8 on top."""
    from grafx_amd.processors import IIRFilter

    torch.manual_seed(7)
    R, C, L, K = 16, 2, 65536, 8
    x = torch.randn(R, C, L, device="cuda").requires_grad_()
    Bs, As = (t.cuda().requires_grad_() for t in coeffs(R, C, K, seed=71))
    gy = torch.randn(R, C, L, device="cuda")
    m = IIRFilter(order=2, backend="lfilter", flashfftconv=False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = m(x, Bs, As)
    y.backward(gy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    one = R * C * L * 4
    print(f"peak {peak / one:.2f} signal tensors above the inputs")
    assert x.grad is not None and Bs.grad is not None and As.grad is not None
    assert peak <= 3 * one, f"forward + backward held {peak / one:.2f} signal tensors"


@pytest.mark.parametrize("which", ["peq_ssm", "geq_lfilter"])
def test_an_equaliser_on_the_exact_backend_takes_an_optimiser_step(which):
    import grafx_amd.processors as P

    torch.manual_seed(8)
    R, L = 2, 700
    if which == "peq_ssm":
        m = P.ParametricEqualizer(num_filters=4, backend="ssm", flashfftconv=False).cuda()
    else:
        m = P.GraphicEqualizer(scale="third_octave", sr=48000, backend="lfilter", flashfftconv=False).cuda()
    sizes = {k: (s,) if isinstance(s, int) else tuple(s) for k, s in m.parameter_size().items()}
    params = {k: (0.3 * torch.randn(R, *s, device="cuda")).requires_grad_() for k, s in sizes.items()}
    start = {k: v.detach().clone() for k, v in params.items()}
    x = torch.randn(R, 2, L, device="cuda")
    target = torch.randn(R, 2, L, device="cuda")
    opt = torch.optim.Adam(list(params.values()), lr=1e-2)
    loss = (m(x, **params) - target).square().mean()
    loss.backward()
    for k, v in params.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().max() > 0, f"{which}: grad of {k}"
    opt.step()
    for k, v in params.items():
        assert torch.isfinite(v).all() and not torch.equal(v.detach(), start[k]), f"{which}: {k} did not move"


# ------------------------------------------------------------------------------------------------- more than two channels
@pytest.mark.parametrize("C,Cf", [(3, 1), (1, 3), (4, 1), (1, 4), (3, 3)])
def test_broadcasts_over_more_than_two_channels(C, Cf):
    """A pair of row-channels is a row's channels only when there are two: with three or four, shared coefficients (C, 1)
    or a shared input (1, C) are passed to the kernel expanded and the channels of the result added by the wrapper; (3, 3)
    has pairs that straddle two rows.  Through both Functions and through the direct call into a strided view."""
    from grafx_amd import ops
    from grafx_amd.autograd import BiquadCascadeFn, BiquadCascadeStateFn

    torch.manual_seed(40 + 5 * C + Cf)
    R, K, L, Co = 3, 2, 600, max(C, Cf)
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, Cf, K, seed=400 + 5 * C + Cf)
    zi = torch.randn(R, Co, K, 2)
    p, q = torch.randn(R, Co, L), torch.randn(R, Co, K, 2)
    what = f"C={C}/{Cf}"
    ours = [t.cuda().requires_grad_(True) for t in (x, Bs, As)]
    (BiquadCascadeFn.apply(*ours) * p.cuda()).sum().backward()
    check(what + " from silence", NAMES[:3], [t.grad for t in ours], reference_grads(x, Bs, As, None, p, None)[0])
    want = reference_grads(x, Bs, As, zi, p, q)[0]
    ours = [t.cuda().requires_grad_(True) for t in (x, Bs, As, zi)]
    y, zf = BiquadCascadeStateFn.apply(*ours)
    ((y * p.cuda()).sum() + (zf * q.cuda()).sum()).backward()
    check(what + " from a state", NAMES, [t.grad for t in ours], want)
    buf = torch.full((1, 5, C, L + 3), float("nan"), device="cuda")
    ov = buf[:, 1:4, :, 1:L + 1]
    got = ops.biquad_cascade_bwd(x.cuda(), p.cuda(), Bs.cuda(), As.cuda(), zi=zi.cuda(), gzf=q.cuda(), out=ov)
    assert got[0].data_ptr() == ov.data_ptr()
    for name, a, b in zip(NAMES, (ov.reshape(R, C, L), *got[1:]), ours):
        assert torch.equal(a, b.grad), f"{what}: the direct call's grad {name} is not the Function's"
    assert buf[:, 0].isnan().all() and buf[:, 4].isnan().all() and buf[..., 0].isnan().all() and buf[..., L + 1:].isnan().all()


def test_the_c_entry_refuses_a_broadcast_it_cannot_sum():
    from grafx_amd import _lib, ops

    R, K, L = 2, 2, 64
    x1, x4, g = (torch.randn(R, c, L, device="cuda") for c in (1, 4, 4))
    c1, c4 = (torch.ones(R, c, K, 3, device="cuda") for c in (1, 4))
    gx1, gx4, gB = torch.zeros_like(x1), torch.zeros_like(x4), torch.zeros_like(c1)
    ws = torch.empty(ops.biquad_cascade_bwd_ws_bytes(R, 4, K, L), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(x, gx, coef, gcoef):
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        return _lib.lib().gfx_biquad_cascade_bwd_f32(ptr(x), ops.rowmap(x)[0], ptr(g), ops.rowmap(g)[0], ptr(gx),
                                                     ops.rowmap(x)[0], ptr(coef), ptr(coef), 0, 0, ptr(gcoef), 0, 0,
                                                     ws.data_ptr(), ws.numel(), R, x.shape[1], coef.shape[1], K, L, stream)

    assert call(x4, gx4, c1, gB) == -1          # shared coefficients, four channels, their gradient asked
    assert call(x1, gx1, c4, None) == -1        # shared input, four channels, its gradient asked
    torch.cuda.synchronize()
    assert not gx1.any() and not gx4.any() and not gB.any()
    assert call(x4, gx4, c1, None) == 0         # the signal gradient alone needs no sum over channels
    torch.cuda.synchronize()
    assert gx4.any()


# ------------------------------------------------------------------------------------------------- the second launch
def test_more_pairs_than_one_launch_takes():
    """The entry launches 2^22 pairs of row-channels at a time: 2^23 + 2050 one-channel rows of 4 samples make a second
    launch of 1025 pairs, whose pairs and workspace offsets start at pair0 = 2^22.  The rows on both sides of that seam
    against the float64 loop, and as a call of their own (even start: the same pairs) for the bits."""
    from grafx_amd import ops

    torch.manual_seed(23)
    seam, K, L = 1 << 23, 1, 4
    R = seam + 2050
    x, gy = torch.randn(R, 1, L, device="cuda"), torch.randn(R, 1, L, device="cuda")
    sl = slice(seam - 1024, R)
    Bsl, Asl = coeffs(R - sl.start, 1, K, seed=230, rmax=0.9)
    Bs = torch.tensor([1.0, 0.5, 0.25], device="cuda").expand(R, 1, K, 3).contiguous()
    As = torch.tensor([1.0, -0.5, 0.3], device="cuda").expand(R, 1, K, 3).contiguous()
    Bs[sl], As[sl] = Bsl.cuda(), Asl.cuda()
    zi, gzf = torch.randn(R, 1, K, 2, device="cuda"), torch.randn(R, 1, K, 2, device="cuda")
    big = ops.biquad_cascade_bwd(x, gy, Bs, As, zi=zi, gzf=gzf)
    part = ops.biquad_cascade_bwd(x[sl], gy[sl], Bs[sl], As[sl], zi=zi[sl], gzf=gzf[sl])
    want = reference_grads(x[sl].cpu(), Bsl, Asl, zi[sl].cpu(), gy[sl].cpu(), gzf[sl].cpu())[0]
    n = R - sl.start
    for name, b, a, w in zip(NAMES, big, part, want):
        assert torch.isfinite(b).all(), name
        assert torch.equal(b[sl], a), f"grad {name}: the rows around pair 2^22 differ from their own call"
        d = (a.cpu().double() - w).reshape(n, -1).abs().amax(1) / w.reshape(n, -1).abs().amax(1)
        assert d.max() <= GRAD_TOL, f"grad {name}: row {sl.start + d.argmax().item()} is {d.max().item():.2e} from float64"


# ------------------------------------------------------------------------------------------------- the checkpoint pass
def test_checkpoints_are_the_forward_states():
    """The checkpoint pass runs a copy of the forward's tables and scan: what it leaves in the workspace for the tile that
    starts at sample 1024 -- per pair, tile and section (w[n0-1], w[n0-2]) of both row-channels -- is the state the
    forward returns after 1024 samples, within the forward's own 1e-5 of the row's peak |w| (the forward's zf is its
    rerun's value, the checkpoint the scan's total: the same number from two roundings, so not the same bits)."""
    from grafx_amd import ops

    torch.manual_seed(24)
    R, C, K, L = 3, 2, 3, 1300
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, C, K, seed=240)
    zi = torch.randn(R, C, K, 2)
    _, zf64, peak = df2(x[..., :1024], Bs, As, zi)
    xc, Bc, Ac, zc = x.cuda(), Bs.cuda(), As.cuda(), zi.cuda()
    zf = ops.biquad_cascade(xc[..., :1024].contiguous(), Bc, Ac, zi=zc, return_state=True)[1]
    ws = torch.zeros(ops.biquad_cascade_bwd_ws_bytes(R, C, K, L), dtype=torch.uint8, device="cuda")
    ops.biquad_cascade_bwd(xc, torch.randn(R, C, L, device="cuda"), Bc, Ac, zi=zc, ws=ws)
    # (pair = row, tile, section, [w1 ch0, w1 ch1, w2 ch0, w2 ch1]) -> (row, channel, section, [w1, w2])
    ck = ws.view(torch.float32).view(R, 3, K, 2, 2)[:, 2].permute(0, 3, 1, 2)
    for what, got in (("checkpoint", ck), ("forward", zf)):
        err = ((got.cpu().double() - zf64).abs().amax(dim=(1, 2, 3)) / peak).max().item()
        print(f"state after 1024 samples, {what}: {err:.2e} of the row's peak |w|")
        assert err <= 1e-5, f"{what}: {err:.2e}"
    first = ws.view(torch.float32).view(R, 3, K, 2, 2)[:, 0].permute(0, 3, 1, 2)
    assert torch.equal(first, zc), "the first tile's checkpoint is zi"
