"""The attack / release envelope state across calls of Ballistics (`zi` / `zf` of `gfx_ballistics_f32`, `gfx_ballistics_energy_f32`,
`gfx_dynamics_ballistics_f32`, `gfx_ballistics_bwd_f32`; `ops.ballistics(zi=, return_state=)`, `BallisticsStateFn`,
`Ballistics / BallisticsEnvelopeFollower / Compressor / NoiseGate(..., state=, return_state=)`): a signal processed in blocks,
each block entering with the envelope the block before left, is the signal processed in one call.

The forward kernels return the float32 sequential recursion bit for bit, so the comparisons of envelopes and states here are
EXACT (`torch.equal` on int32 views) against a float32 numpy loop with the same arithmetic as `oracle._attack_release` --
`(one - c) * prev + c * x`, every operation rounded once -- that starts from `zi` instead of the oracle's fixed 1.  The first
test shows, on the CPU, that this loop with zi = 1 IS the oracle's on the inputs used below: the premise of every equality
that follows.  Both sides get the same float32 coefficients (`coefficients=True`), as in tests/test_gpu_ballistics.py.

Gradients are compared with float64 autograd through the plain loop written in torch (the branch chosen by `torch.where` on
a detached comparison), at the adjoint's standing bounds: gx within 2e-6 of max |gx_ref|, gz within 1e-4 of max |gz_ref|
(test_chunked_adjoint_at_the_console_size_against_float64_on_sample_rows); gzi, the same quantity as the carry those bounds
cover, within 2e-6 of max(max |gx_ref|, max |gzi_ref|)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from conftest import assert_close

gpu = pytest.mark.gpu
TOL = 1e-5
SCHEDULES = ["chunks", "rows"]
# (rows, length): the single-pass walk, two chunks, the lg >= 4 retry with longer chunks, rows sharing a wave, more rows than
# a 64-row group; L % 4 != 0 takes the element-wise loads
SHAPES = [(1, 1), (3, 64), (5, 1001), (64, 4100), (300, 16384), (4097, 1024)]
CUTS = [1, 3, 64, 65, 255, 256, 257]


def _coef(R, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(R, 2, generator=g) * (hi - lo) + lo).float()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def loop(x, at, rt, zi=None):
    """y[-1] = zi (None: 1);  c = at if x[n] < y[n-1] else rt;  y[n] = (1 - c) y[n-1] + c x[n] in float32, one rounding per
    operation -> (y (R, L), zf (R,) = y[:, L-1])."""
    xs, a, r = (t.detach().cpu().numpy().astype(np.float32) for t in (x, at, rt))
    prev = np.ones(xs.shape[0], dtype=np.float32) if zi is None else zi.detach().cpu().numpy().astype(np.float32).copy()
    one = np.float32(1)
    y = np.empty_like(xs)
    for n in range(xs.shape[1]):
        c = np.where(xs[:, n] < prev, a, r)
        prev = (one - c) * prev + c * xs[:, n]
        y[:, n] = prev
    return torch.from_numpy(y), torch.from_numpy(prev.copy())


@functools.lru_cache(maxsize=None)
def case(R, L):
    """Input, coefficients, a random entering state in [0, 2) and the local loop from it (computed once per shape)."""
    torch.manual_seed(R * 131 + L)
    u = torch.rand(R, L) * 2.0
    coef = _coef(R, 0.02, 0.98, R + L)
    zi = torch.rand(R) * 2.0
    y, zf = loop(u, coef[:, 0], coef[:, 1], zi)
    return u, coef, zi, y, zf


@functools.lru_cache(maxsize=None)
def slow_case():
    """test_slow_coefficients_take_the_whole_row_walk_and_stay_exact's rows: every other one with coefficients around 2.5e-3,
    whose warm-up fits no chunk -- the whole-row pass walks them and has to read zi again."""
    R, L = 9, 32768
    torch.manual_seed(R)
    u = torch.rand(R, L) * 3.0
    coef = _coef(R, 0.3, 0.9, 5)
    coef[::2] = _coef(R, 2e-3, 3e-3, 6)[::2]
    zi = torch.rand(R) * 2.0
    y, zf = loop(u, coef[:, 0], coef[:, 1], zi)
    return u, coef, zi, y, zf


def blocks_of(L, cuts):
    cuts = [c for c in cuts if 0 < c < L]
    return list(zip([0] + cuts, cuts + [L]))


def in_blocks(fn, L, cuts, zi):
    """fn(lo, hi, zi) -> (y, zf) block by block, the state handed on -> (concatenated y, last zf)."""
    ys, z = [], zi
    for lo, hi in blocks_of(L, cuts):
        y, z = fn(lo, hi, z)
        ys.append(y)
    return torch.cat(ys, -1), z


# ------------------------------------------------------------------------------------------------ the premise (CPU)
def test_the_local_loop_from_one_is_the_oracles_loop():
    for R, L in SHAPES:
        u, coef, _, _, _ = case(R, L)
        y, zf = loop(u, coef[:, 0], coef[:, 1])
        ref = oracle.ballistics_coefficients(u, coef[:, 0], coef[:, 1])
        assert torch.equal(_bits(y), _bits(ref)) and torch.equal(_bits(zf), _bits(ref[:, -1])), (R, L)
    u, coef, _, _, _ = slow_case()
    assert torch.equal(_bits(loop(u, coef[:, 0], coef[:, 1])[0]), _bits(oracle.ballistics_coefficients(u, coef[:, 0], coef[:, 1])))
    for C in (1, 2):
        x, coef, _ = energy_case(C)
        e = x.square().mean(-2)
        assert torch.equal(_bits(loop(e, coef[:, 0], coef[:, 1])[0]), _bits(oracle.ballistics_coefficients(e, coef[:, 0], coef[:, 1])))


# ------------------------------------------------------------------------------------------------ bit equality
@gpu
@pytest.mark.parametrize("R,L", SHAPES)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_no_state_and_a_state_of_ones_are_the_existing_call(R, L, schedule):
    from grafx_amd import ops

    u, coef, _, _, _ = case(R, L)
    uc, cc = u.cuda(), coef.cuda()
    old = ops.ballistics(uc, cc, coefficients=True, schedule=schedule)
    for what, zi in (("zi = None", None), ("zi = ones", torch.ones(R, device="cuda"))):
        y, zf = ops.ballistics(uc, cc, coefficients=True, schedule=schedule, zi=zi, return_state=True)
        assert torch.equal(_bits(y), _bits(old)), what
        assert zf.shape == (R,) and zf.dtype == torch.float32 and torch.equal(_bits(zf), _bits(old[:, -1])), what
    assert torch.equal(_bits(ops.ballistics(uc, cc, coefficients=True, schedule=schedule, zi=torch.ones(R, device="cuda"))),
                       _bits(old))


@gpu
@pytest.mark.parametrize("R,L", SHAPES)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_split_equals_whole_equals_the_sequential_loop(R, L, schedule):
    """A random entering state; the row cut at 1, 3, 64, 65, 255, 256, 257 and L - 1 (where they fit) and into blocks of 37."""
    from grafx_amd import ops

    u, coef, zi, y_ref, zf_ref = case(R, L)
    uc, cc, zc = u.cuda(), coef.cuda(), zi.cuda()
    keep = zc.clone()
    y, zf = ops.ballistics(uc, cc, coefficients=True, schedule=schedule, zi=zc, return_state=True)
    assert torch.equal(_bits(y), _bits(y_ref)), f"one call vs the loop: {(y.cpu() - y_ref).abs().max():.3e}"
    assert torch.equal(_bits(zf), _bits(zf_ref)) and torch.equal(zc, keep)

    def run(lo, hi, z):
        return ops.ballistics(uc[:, lo:hi], cc, coefficients=True, schedule=schedule, zi=z, return_state=True)

    for cuts in [[c] for c in CUTS + [L - 1]] + [list(range(37, L, 37))]:
        if not blocks_of(L, cuts)[1:]:
            continue
        yb, zb = in_blocks(run, L, cuts, zc)
        assert torch.equal(_bits(yb), _bits(y)), f"cut at {cuts[:3]}: {(yb - y).abs().max():.3e}"
        assert torch.equal(_bits(zb), _bits(zf)), f"cut at {cuts[:3]}: final state"


@gpu
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_slow_rows_walked_whole_start_from_the_state(schedule):
    from grafx_amd import ops

    u, coef, zi, y_ref, zf_ref = slow_case()
    uc, cc, zc = u.cuda(), coef.cuda(), zi.cuda()
    flags = []
    y, zf = ops.ballistics(uc, cc, coefficients=True, schedule=schedule, zi=zc, return_state=True, flags=flags)
    if schedule == "chunks":
        assert flags[0].cpu().tolist() == [1, 0] * 4 + [1]       # the slow rows went to the whole-row pass
    assert torch.equal(_bits(y), _bits(y_ref)) and torch.equal(_bits(zf), _bits(zf_ref))
    yb, zb = in_blocks(lambda lo, hi, z: ops.ballistics(uc[:, lo:hi], cc, coefficients=True, schedule=schedule, zi=z,
                                                        return_state=True), u.shape[1], [10000], zc)
    assert torch.equal(_bits(yb), _bits(y_ref)) and torch.equal(_bits(zb), _bits(zf_ref))


@functools.lru_cache(maxsize=None)
def energy_case(C):
    R, L = 6, 4096
    torch.manual_seed(R + L + C)
    return torch.randn(R, C, L), _coef(R, 0.05, 0.9, C), torch.rand(R) * 2.0


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_energy_source_with_state(C, schedule):
    """env = ballistics(mean_c x^2) in one pass over x: squares, channel sum and the division by C each rounded
    (x.square().mean(-2)), then the recursion from zi -- on (6, C, 4096) and on a strided (B, n, C, L) view of a buffer."""
    from grafx_amd import ops

    x, coef, zi = energy_case(C)
    R, _, L = x.shape
    y_ref, zf_ref = loop(x.square().mean(-2), coef[:, 0], coef[:, 1], zi)
    cc, zc = coef.cuda(), zi.cuda()
    buf = torch.randn(2, 7, C, L, device="cuda")
    buf[:, 2:5] = x.view(2, 3, C, L).cuda()
    for what, src in (("rows", x.cuda()), ("strided view", buf[:, 2:5])):
        y, zf = ops.ballistics_energy(src, cc, coefficients=True, schedule=schedule, zi=zc, return_state=True)
        assert torch.equal(_bits(y), _bits(y_ref)) and torch.equal(_bits(zf), _bits(zf_ref)), what
        for cuts in ([1], [255], [256], [2048], [4095], list(range(37, L, 370))):
            yb, zb = in_blocks(lambda lo, hi, z: ops.ballistics_energy(src[..., lo:hi], cc, coefficients=True, schedule=schedule,
                                                                       zi=z, return_state=True), L, cuts, zc)
            assert torch.equal(_bits(yb), _bits(y_ref)) and torch.equal(_bits(zb), _bits(zf_ref)), (what, cuts[:2])


@gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("knee,gate", [("hard", False), ("quadratic", True), ("exponential", False)])
def test_one_pass_compressor_with_state(C, knee, gate):
    """gfx_dynamics_ballistics_f32 never stores the envelope: its zf is the zf of ops.ballistics_energy on the same
    input bit for bit; its output in two blocks is the one-call output -- the same bits when both blocks (and the whole) have
    lengths that are multiples of 4 (the same kernel instantiation), within 1e-5 otherwise."""
    from grafx_amd import ops

    R, L = 6, 4096
    torch.manual_seed(40 + C + len(knee))
    x = (torch.randn(R, C, L) * 0.3).cuda()
    p = [torch.randn(R, 1, device="cuda") for _ in range(3)]
    za = torch.randn(R, 2, device="cuda")
    zi = (torch.rand(R) * 2.0).cuda()
    for schedule in SCHEDULES:
        old = ops.dynamics_ballistics(x, *p, za, knee, gate, schedule=schedule)
        y0, zf0 = ops.dynamics_ballistics(x, *p, za, knee, gate, schedule=schedule, return_state=True)
        assert torch.equal(_bits(y0), _bits(old)), "zi = None is the existing call"
        assert torch.equal(_bits(zf0), _bits(ops.ballistics_energy(x, za, schedule=schedule, return_state=True)[1]))
        y, zf = ops.dynamics_ballistics(x, *p, za, knee, gate, schedule=schedule, zi=zi, return_state=True)
        env, zf_env = ops.ballistics_energy(x, za, schedule=schedule, zi=zi, return_state=True)
        assert torch.equal(_bits(zf), _bits(zf_env)) and torch.equal(_bits(zf), _bits(env[:, -1]))
        for cut in (2048, 1000, 1001):

            def run(lo, hi, z):
                return ops.dynamics_ballistics(x[..., lo:hi], *p, za, knee, gate, schedule=schedule, zi=z, return_state=True)

            for what, z_in, want, want_zf in (("zi", zi, y, zf), ("None", None, old, zf0)):
                yb, zb = in_blocks(run, L, [cut], z_in)
                assert torch.equal(_bits(zb), _bits(want_zf)), (schedule, cut, what)
                err = float((yb - want).abs().max() / want.abs().max())
                print(f"one-pass {knee} gate={gate} C={C} {schedule} cut {cut} zi={what}: max |diff| / max |y| = {err:.2e}")
                if cut % 4 == 0:
                    assert torch.equal(_bits(yb), _bits(want)), (schedule, cut, what, err)
                else:
                    assert_close(yb.cpu(), want.cpu(), TOL, f"one-pass compressor cut at {cut}")


# ------------------------------------------------------------------------------------------------ gradients
def loop64(x, z, zi):
    """The plain loop in torch (differentiable): -> (y, zf)."""
    at, rt = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1])
    prev, ys = zi, []
    for n in range(x.shape[1]):
        c = torch.where((x[:, n] < prev).detach(), at, rt)
        prev = (1 - c) * prev + c * x[:, n]
        ys.append(prev)
    return torch.stack(ys, -1), prev


@functools.lru_cache(maxsize=None)
def grad_case(R, L):
    torch.manual_seed(R + L)
    x = torch.rand(R, L) * 2
    z = torch.randn(R, 2) * 1.5
    z[3, 0] = -4.0                                       # c = 0.018
    zi = torch.rand(R) * 2.0
    p, q = torch.randn(R, L), torch.randn(R)
    refs = {}
    for what, wp, wq, state in (("both", 1.0, 1.0, zi), ("y", 1.0, 0.0, zi), ("zf", 0.0, 1.0, zi), ("stateless", 1.0, 0.0, None)):
        leaves = [t.double().requires_grad_(True) for t in (x, z, zi if state is not None else torch.ones(R))]
        y, zf = loop64(*leaves)
        (wp * (y * p.double()).sum() + wq * (zf * q.double()).sum()).backward()
        refs[what] = [t.grad for t in leaves]
    return x, z, zi, p, q, refs


def check_grads(got, ref, what):
    """gx 2e-6 of max |gx_ref|, gz 1e-4 of max |gz_ref|, gzi 2e-6 of max(max |gx_ref|, max |gzi_ref|)."""
    gx, gz = got[0].cpu().double(), got[1].cpu().double()
    ex, ez = (gx - ref[0]).abs().max().item(), (gz - ref[1]).abs().max().item()
    sx, sz = ref[0].abs().max().item(), ref[1].abs().max().item()
    print(f"{what}: gx {ex / sx:.2e} of max |gx_ref|, gz {ez / sz:.2e} of max |gz_ref|")
    assert torch.isfinite(gx).all() and torch.isfinite(gz).all(), what
    assert ex <= 2e-6 * sx, f"{what}: gx {ex / sx:.2e}"
    assert ez <= 1e-4 * sz, f"{what}: gz {ez / sz:.2e}"
    if len(got) > 2:
        gzi = got[2].cpu().double()
        ei, si = (gzi - ref[2]).abs().max().item(), max(sx, ref[2].abs().max().item())
        print(f"{what}: gzi {ei / si:.2e} of max(max |gx_ref|, max |gzi_ref|)")
        assert torch.isfinite(gzi).all() and ei <= 2e-6 * si, f"{what}: gzi {ei / si:.2e}"


@gpu
@pytest.mark.parametrize("R,L", [(6, 600), (130, 5000)])
def test_gradients_with_state_against_float64(R, L):
    from grafx_amd.autograd import BallisticsFn, BallisticsStateFn

    x, z, zi, p, q, refs = grad_case(R, L)
    # the premise: the existing stateless adjoint meets its standing bounds on these inputs
    xs, zs = x.cuda().requires_grad_(True), z.cuda().requires_grad_(True)
    (BallisticsFn.apply(xs, zs) * p.cuda()).sum().backward()
    check_grads([xs.grad, zs.grad], refs["stateless"], f"({R}, {L}) stateless premise")
    for what, wp, wq in (("both", True, True), ("y", True, False), ("zf", False, True)):
        leaves = [t.cuda().requires_grad_(True) for t in (x, z, zi)]
        y, zf = BallisticsStateFn.apply(*leaves)
        loss = ((y * p.cuda()).sum() if wp else 0) + ((zf * q.cuda()).sum() if wq else 0)
        loss.backward()
        check_grads([t.grad for t in leaves], refs[what], f"({R}, {L}) cotangent on {what}")


@gpu
def test_chunked_adjoint_with_state_equals_the_whole_row_adjoint():
    """(130, 40000): nine chunks -- the first 64-row group takes the warm-up form, the second (coefficients ~ 2.5e-3) and the
    ragged third the two-pass aggregate form, where gzi comes from the chunk that holds sample 0 after the carry chain.
    The bounds of test_chunked_adjoint_equals_the_whole_row_adjoint; gzi as the carry, 1e-6 of max(|gx|, |gzi|)."""
    from grafx_amd import ops

    R, L = 130, 40000
    torch.manual_seed(R + L)
    x = torch.rand(R, L, device="cuda") * 2
    z = torch.randn(R, 2, device="cuda") * 1.5
    z[70:] = torch.randn(R - 70, 2, device="cuda") * 0.5 - 6.0
    z[3, 0] = -4.0
    zi = torch.rand(R, device="cuda") * 2
    y = ops.ballistics(x, z, zi=zi)
    g = torch.randn(R, L, device="cuda")
    g[:, 4096:] *= 1e-3          # what reaches sample 0 of the slow rows comes through the carry chain
    gx_c, gz_c, gi_c = ops.ballistics_bwd(x, y, g, z, schedule="chunks", zi=zi)
    gx_r, gz_r, gi_r = ops.ballistics_bwd(x, y, g, z, schedule="rows", zi=zi)
    scale = max(gx_r.abs().max().item(), gi_r.abs().max().item())
    print(f"gx {float((gx_c - gx_r).abs().max() / gx_r.abs().max()):.2e} gz {float((gz_c - gz_r).abs().max() / gz_r.abs().max()):.2e} "
          f"gzi {float((gi_c - gi_r).abs().max()) / scale:.2e}")
    assert (gx_c - gx_r).abs().max() <= 1e-6 * gx_r.abs().max()
    assert (gz_c - gz_r).abs().max() <= 2e-5 * gz_r.abs().max()
    assert (gi_c - gi_r).abs().max() <= 1e-6 * scale
    assert gi_r[70:].abs().min() > 0                     # (the slow rows' carries are not trivially zero)
    # zi = ones is the stateless adjoint
    y1 = ops.ballistics(x, z)
    one = ops.ballistics_bwd(x, y1, g, z, schedule="chunks", zi=torch.ones(R, device="cuda"))
    old = ops.ballistics_bwd(x, y1, g, z, schedule="chunks")
    assert torch.equal(one[0], old[0]) and torch.equal(one[1], old[1])


@gpu
def test_back_propagation_through_two_chained_blocks():
    """Cut at 217 of 600: the gradients of the one-call BallisticsFn run, within the chunk-against-rows bounds (gx 1e-6,
    gz 2e-5 of their maxima)."""
    from grafx_amd.processors import Ballistics

    x, z, _, p, _, _ = grad_case(6, 600)
    m, cut, pc = Ballistics(), 217, p.cuda()
    one = [t.cuda().requires_grad_(True) for t in (x, z)]
    (m(*one) * pc).sum().backward()
    two = [t.cuda().requires_grad_(True) for t in (x, z)]
    y1, s = m(two[0][:, :cut], two[1], return_state=True)
    y2, s = m(two[0][:, cut:], two[1], state=s, return_state=True)
    assert s.requires_grad and s.shape == (6,)
    (torch.cat([y1, y2], -1) * pc).sum().backward()
    for name, got, want, tol in (("x", two[0].grad, one[0].grad, 1e-6), ("z_alpha", two[1].grad, one[1].grad, 2e-5)):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"through two blocks, grad {name}: {err:.2e}")
        assert err <= tol, f"through two blocks, grad {name}: {err:.2e}"


# ------------------------------------------------------------------------------------------------ surface
def _params(m, R, seed):
    g = torch.Generator().manual_seed(seed)
    p = {k: torch.randn(R, v, generator=g) for k, v in m.parameter_size().items()}
    p["log_threshold"] = 4.0 + 0.3 * p["log_threshold"]     # the threshold between the block's envelope (~0.09) and 1
    for k in ("z_alpha_pre", "z_alpha_post"):
        if k in p:
            p[k] = p[k] - 2.0                                # coefficients around 0.12: a seam of some tens of samples
    return {k: v.cuda() for k, v in p.items()}


@gpu
@pytest.mark.parametrize("cls", ["Compressor", "NoiseGate"])
@pytest.mark.parametrize("gain_smoother", [None, "ballistics"])
@pytest.mark.parametrize("knee", ["hard", "quadratic", "exponential"])
def test_dynamics_processors_in_two_blocks(cls, gain_smoother, knee):
    import grafx_amd.processors as P

    R, C, L, cut = 3, 2, 900, 401
    S = 1 if gain_smoother is None else 2
    m = getattr(P, cls)(energy_smoother="ballistics", gain_smoother=gain_smoother, knee=knee, flashfftconv=False).cuda()
    params = _params(m, R, len(knee) + S)
    torch.manual_seed(13)
    x = (torch.randn(R, C, L) * 0.3).cuda()
    with torch.no_grad():
        want = m(x, **params)
        y1, s1 = m(x[..., :cut], **params, return_state=True)
        y2, s2 = m(x[..., cut:], **params, state=s1, return_state=True)
        y2_only = m(x[..., cut:], **params, state=s1)
        _, s_one = m(x, **params, return_state=True)
        cold = m(x[..., cut:], **params)
    assert s1.shape == (R, S) and s2.shape == (R, S) and s1.dtype == torch.float32 and torch.equal(y2, y2_only)
    assert torch.equal(_bits(s2[:, 0]), _bits(s_one[:, 0]))          # the energy envelope is exact
    assert_close(s2.cpu(), s_one.cpu(), TOL, f"{cls} {knee} S={S}: state after two blocks")
    assert_close(torch.cat([y1, y2], -1).cpu(), want.cpu(), TOL, f"{cls} {knee} S={S} in two blocks")
    seam = (torch.cat([y1, cold], -1) - want).abs().max() / want.abs().max()
    assert seam > 1e-3, f"no seam without the state: {seam:.2e}"
    # a (B, n, C, L) view of a wider buffer: state (B, n, S); rows as above
    buf = torch.zeros(1, 5, C, L, device="cuda")
    buf[:, 1:4] = x.view(1, 3, C, L)
    with torch.no_grad():
        v1, t1 = m(buf[:, 1:4, :, :cut], **params, return_state=True)
        v2, t2 = m(buf[:, 1:4, :, cut:], **params, state=t1, return_state=True)
    assert t1.shape == (1, 3, S) and t2.shape == (1, 3, S) and v1.shape == (1, 3, C, cut)
    assert torch.equal(_bits(t2.view(R, S)[:, 0]), _bits(s_one[:, 0]))
    assert_close(torch.cat([v1, v2], -1).view(R, C, L).cpu(), want.cpu(), TOL, f"{cls} {knee} S={S}: 4-D view in two blocks")


@gpu
def test_dynamics_blocks_on_aligned_lengths_are_the_one_call_bits():
    import grafx_amd.processors as P

    R, C, L, cut = 3, 2, 4096, 2048
    m = P.Compressor(energy_smoother="ballistics", knee="quadratic", flashfftconv=False).cuda()
    params = _params(m, R, 3)
    torch.manual_seed(14)
    x = (torch.randn(R, C, L) * 0.3).cuda()
    with torch.no_grad():
        want = m(x, **params)
        y1, s = m(x[..., :cut], **params, return_state=True)
        y2, s = m(x[..., cut:], **params, state=s, return_state=True)
    assert torch.equal(_bits(torch.cat([y1, y2], -1)), _bits(want))


@gpu
def test_shared_parameter_rows_with_a_state():
    import grafx_amd.processors as P

    B, n, C, L, cut = 2, 3, 2, 900, 401
    m = P.Compressor(energy_smoother="ballistics", knee="quadratic", flashfftconv=False).cuda()
    params = _params(m, n, 5)
    torch.manual_seed(15)
    x = (torch.randn(B, n, C, L) * 0.3).cuda()
    with torch.no_grad():
        want = m(x, **params, _shared_rows=n)
        y1, s = m(x[..., :cut], **params, _shared_rows=n, return_state=True)
        y2, s = m(x[..., cut:], **params, _shared_rows=n, state=s, return_state=True)
    assert s.shape == (B, n, 1)
    assert_close(torch.cat([y1, y2], -1).reshape(want.shape).cpu(), want.cpu(), TOL, "shared parameter rows in two blocks")


@gpu
@pytest.mark.parametrize("gain_smoother", [None, "ballistics"])
def test_differentiable_dynamics_in_two_blocks(gain_smoother):
    """The training path (torch ops around BallisticsStateFn): two chained blocks against the one-call differentiable forward.
    Both sides are float32 evaluations of the same derivative, each within the adjoint's standing 1e-4 of exact for the
    coefficient gradients, the loosest of its bounds: 2e-4 of the gradient's maximum between them."""
    import grafx_amd.processors as P

    R, C, L, cut = 3, 2, 900, 401
    m = P.Compressor(energy_smoother="ballistics", gain_smoother=gain_smoother, knee="quadratic", flashfftconv=False).cuda()
    params = _params(m, R, 7)
    torch.manual_seed(16)
    x = (torch.randn(R, C, L) * 0.3).cuda()
    p = torch.randn(R, C, L, device="cuda")
    one = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    xo = x.clone().requires_grad_(True)
    want = m(xo, **one)
    (want * p).sum().backward()
    two = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    xt = x.clone().requires_grad_(True)
    y1, s = m(xt[..., :cut], **two, return_state=True)
    y2, s = m(xt[..., cut:], **two, state=s, return_state=True)
    assert s.requires_grad and s.shape == (R, 1 if gain_smoother is None else 2)
    y = torch.cat([y1, y2], -1)
    assert_close(y.detach().cpu(), want.detach().cpu(), TOL, "differentiable path in two blocks")
    (y * p).sum().backward()
    for name, got, ref in [("x", xt.grad, xo.grad)] + [(k, two[k].grad, one[k].grad) for k in params]:
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"differentiable dynamics in two blocks, grad {name}: {err:.2e}")
        assert torch.isfinite(got).all() and err <= 2e-4, f"grad {name}: {err:.2e}"


@gpu
def test_ballistics_and_its_envelope_follower_in_two_blocks():
    import grafx_amd.processors as P
    from grafx_amd.processors.core.envelope import Ballistics

    R, C, L, cut = 3, 2, 900, 401
    torch.manual_seed(17)
    x = (torch.randn(R, C, L) * 0.3).cuda()
    z = (torch.randn(R, 2) - 2.0).cuda()
    e = x.square().mean(-2)
    for what, m, src in (("Ballistics", Ballistics(), e), ("BallisticsEnvelopeFollower", P.BallisticsEnvelopeFollower(), x)):
        with torch.no_grad():
            want = m(src, z)
            y1, s = m(src[..., :cut], z, return_state=True)
            y2, s2 = m(src[..., cut:], z, state=s, return_state=True)
            y2_only = m(src[..., cut:], z, state=s)
            cold = m(src[..., cut:], z)
            _, s_one = m(src, z, return_state=True)
        assert s.shape == (R,) and s.dtype == torch.float32 and torch.equal(y2, y2_only), what
        assert torch.equal(_bits(s2), _bits(s_one)), what
        if what == "Ballistics":
            assert torch.equal(_bits(torch.cat([y1, y2], -1)), _bits(want)) and torch.equal(_bits(s2), _bits(want[:, -1]))
        else:
            assert_close(torch.cat([y1, y2], -1).cpu(), want.cpu(), TOL, what + " in two blocks")
        assert (torch.cat([y1, cold], -1) - want).abs().max() > 1e-3 * want.abs().max(), what + ": no seam without the state"


@gpu
def test_the_truncated_one_pole_refuses_state():
    import grafx_amd.processors as P

    R, C, L = 2, 2, 256
    x = torch.randn(R, C, L, device="cuda")
    m = P.Compressor(flashfftconv=False).cuda()                      # the default "iir" energy smoother
    params = {k: torch.randn(R, v, device="cuda") for k, v in m.parameter_size().items()}
    f = P.IIREnvelopeFollower(flashfftconv=False).cuda()
    z = torch.randn(R, 1, device="cuda")
    for call in (lambda: m(x, **params, return_state=True), lambda: m(x, **params, state=torch.ones(R, 1, device="cuda")),
                 lambda: f(x, z, return_state=True), lambda: f(x, z, state=torch.ones(R, device="cuda"))):
        with pytest.raises(ValueError, match=r"iir_len.*ballistics"):
            call()
    mixed = P.Compressor(energy_smoother="ballistics", gain_smoother="iir", flashfftconv=False).cuda()
    mp = {k: torch.randn(R, v, device="cuda") for k, v in mixed.parameter_size().items()}
    with pytest.raises(ValueError, match="iir_len"):
        mixed(x, **mp, return_state=True)


@gpu
def test_bad_states_are_refused():
    from grafx_amd import _lib, ops
    import grafx_amd.processors as P

    R, L = 4, 64
    u, z = torch.rand(R, L, device="cuda"), torch.randn(R, 2, device="cuda")
    x = torch.randn(R, 2, L, device="cuda")
    p = [torch.randn(R, 1, device="cuda") for _ in range(3)]
    bad = (torch.ones(R + 1, device="cuda"), torch.ones(R, 1, device="cuda"), torch.ones(R, device="cuda", dtype=torch.float64),
           torch.ones(R), torch.ones(2 * R, device="cuda")[::2])
    for zi in bad:
        with pytest.raises(ValueError, match="zi must be"):
            ops.ballistics(u, z, zi=zi)
        with pytest.raises(ValueError, match="zi must be"):
            ops.ballistics_energy(x, z, zi=zi)
        with pytest.raises(ValueError, match="zi must be"):
            ops.dynamics_ballistics(x, *p, z, "quadratic", False, zi=zi)
        with pytest.raises(ValueError, match="zi must be"):
            ops.ballistics_bwd(u, u, u, z, zi=zi)
    m = P.Compressor(energy_smoother="ballistics", gain_smoother="ballistics", flashfftconv=False).cuda()
    params = {k: torch.randn(R, v, device="cuda") for k, v in m.parameter_size().items()}
    for state in (torch.ones(R, 1, device="cuda"), torch.ones(R, device="cuda"), torch.ones(R, 2), torch.ones(R, 2, device="cuda").double()):
        with pytest.raises(ValueError, match="state must be"):
            m(x, **params, state=state)
    # zf sharing memory with zi at the C entry: later launches re-read zi, so it is refused (unlike the biquad's in-place state)
    y, zi, ws = torch.empty_like(u), torch.ones(R + 1, device="cuda"), torch.zeros(4 * R, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib()
    for zf in (zi, zi[1:]):
        assert lib.gfx_ballistics_f32(u.data_ptr(), z.data_ptr(), 0, zi.data_ptr(), zf.data_ptr(), y.data_ptr(), R, L,
                                      ws.data_ptr(), ws.numel(), stream) == ops.GFX_EINVAL
        assert lib.gfx_ballistics_energy_f32(x.data_ptr(), ops.rowmap(x)[0], 2, z.data_ptr(), 0, zi.data_ptr(), zf.data_ptr(),
                                             y.data_ptr(), R, L, ws.data_ptr(), ws.numel(), stream) == ops.GFX_EINVAL
        out = torch.empty_like(x)
        assert lib.gfx_dynamics_ballistics_f32(x.data_ptr(), ops.rowmap(x)[0], out.data_ptr(), ops.rowmap(out)[0],
                                               p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), z.data_ptr(), R, R, 2, L,
                                               1, 0, zi.data_ptr(), zf.data_ptr(), ws.data_ptr(), ws.numel(),
                                               stream) == ops.GFX_EINVAL
    torch.cuda.synchronize()
