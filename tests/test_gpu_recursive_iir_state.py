"""Filter state across calls of the exact recursive IIR cascade (`gfx_biquad_cascade_state_f32`, `ops.biquad_cascade(zi=,
return_state=)`, `BiquadCascadeStateFn`, `IIRFilter(..., state=, return_state=)`): a signal processed in blocks, each block
entering with the state the block before left, is the signal processed in one call -- outputs, final state and gradients.

The reference is a plain direct-form-II loop in float64, written here:
    w[n] = u[n] - a1 w[n-1] - a2 w[n-2],   y[n] = b0 w[n] + b1 w[n-1] + b2 w[n-2]      (b = B / a0, a = A / a0)
with the state (w[n-1], w[n-2]) per row-channel and section, (R, Cout, K, 2).  Outputs are held to the kernel's standing
1e-5 (conftest.assert_close); a state to 1e-5 of its row's peak |w|.  Every pole set used with that bound is first shown to
meet it on the existing stateless call."""
import functools

import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
TOL = 1e-5
GRAD_TOL = 2e-4     # test_recursive_backends_are_differentiable: max |got - want| / max |want|


def coeffs(R, Cf, K, seed, rmax=0.95, equaliser=False):
    """Stable sections with a0 != 1: poles at radius 0.5 .. rmax, numerators around (1, 0, 0).  equaliser: every section's
    zeros at its poles' angle and 0.8 .. 1 of their radius instead, as the bands of an equaliser have them -- what a long
    cascade needs to be well conditioned in float32 at all (32 sections with unrelated random numerators: a plain
    sequential float32 recursion is itself 3e-5 .. 1e-4 from float64; with these 1e-6)."""
    g = torch.Generator().manual_seed(seed)
    radius = 0.5 + (rmax - 0.5) * torch.rand(R, Cf, K, generator=g)
    theta = 0.1 + 2.9 * torch.rand(R, Cf, K, generator=g)
    a0 = 1.0 + 0.2 * torch.rand(R, Cf, K, generator=g)
    As = torch.stack([torch.ones_like(radius), -2 * radius * torch.cos(theta), radius.square()], -1) * a0.unsqueeze(-1)
    if equaliser:
        rz = radius * (0.8 + 0.2 * torch.rand(R, Cf, K, generator=g))
        return torch.stack([torch.ones_like(rz), -2 * rz * torch.cos(theta), rz.square()], -1), As
    Bs = 0.5 * torch.randn(R, Cf, K, 3, generator=g)
    Bs[..., 0] += 1.0
    return Bs, As


def df2(x, Bs, As, zi=None, quirk=False):
    """The float64 reference (differentiable): x (R, C, L), Bs / As (R, Cf, K, 3), zi (R, Co, K, 2) or None
    -> y (R, Co, L), zf (R, Co, K, 2), the rows' peak |w| (R,).  quirk: upstream's "ssm", every section's recursion driven
    by the ORIGINAL input and only its direct term b0 by the section before."""
    R, C, L = x.shape
    Cf, K = Bs.shape[1], Bs.shape[2]
    Co = max(C, Cf)
    x, Bs, As = x.double(), Bs.double(), As.double()
    zi = torch.zeros(R, Co, K, 2, dtype=torch.float64) if zi is None else zi.double()
    x0 = x.expand(R, Co, L)
    y, zf, peak = x0, [], zi.detach().abs().amax(dim=(1, 2, 3))
    for k in range(K):
        b = (Bs[:, :, k] / As[:, :, k, :1]).expand(R, Co, 3)
        a = (As[:, :, k] / As[:, :, k, :1]).expand(R, Co, 3)
        u = x0 if quirk else y
        w1, w2, out = zi[:, :, k, 0], zi[:, :, k, 1], []
        for n in range(L):
            w = u[..., n] - a[..., 1] * w1 - a[..., 2] * w2
            if quirk:
                out.append(b[..., 0] * y[..., n] + (b[..., 1] - b[..., 0] * a[..., 1]) * w1
                           + (b[..., 2] - b[..., 0] * a[..., 2]) * w2)
            else:
                out.append(b[..., 0] * w + b[..., 1] * w1 + b[..., 2] * w2)
            w2, w1 = w1, w
            peak = torch.maximum(peak, w.detach().abs().amax(1))
        y = torch.stack(out, -1)
        zf.append(torch.stack([w1, w2], -1))
    return y, torch.stack(zf, 2), peak


def assert_state_close(zf, ref, peak, what):
    """Every row's state within TOL of the row's peak |w| (the scale the recursion's rounding errors have)."""
    assert zf.shape == ref.shape and zf.dtype == torch.float32, f"{what}: {tuple(zf.shape)} {zf.dtype}"
    err = ((zf.detach().cpu().double() - ref).abs().amax(dim=(1, 2, 3)) / peak).max().item()
    print(f"{what}: state error {err:.2e} of the row's peak |w|")
    assert err <= TOL, f"{what}: state error {err:.2e} of the row's peak |w| > {TOL:g}"


def stateless_meets_the_bound(x, Bs, As, y64, what, quirk=False):
    """The premise of every 1e-5 below: the existing call is that close to float64 on these inputs."""
    from grafx_amd import ops

    y = ops.biquad_cascade(x.cuda(), Bs.cuda(), As.cuda(), ssm_quirk=quirk)
    assert_close(y.cpu(), y64.float(), TOL, what + ": stateless call vs float64")
    return y


def in_blocks(x, Bs, As, cuts, zi=None, quirk=False):
    """x through ops.biquad_cascade block by block (cuts: the block boundaries), the state handed on."""
    from grafx_amd import ops

    ys, z = [], zi
    for lo, hi in zip([0] + list(cuts), list(cuts) + [x.shape[-1]]):
        y, z = ops.biquad_cascade(x[..., lo:hi], Bs, As, ssm_quirk=quirk, zi=z, return_state=True)
        ys.append(y)
    return torch.cat(ys, -1), z


# ---------------------------------------------------------------------------------------------- whole-wave form
@functools.lru_cache(maxsize=None)
def wave_case():
    """R = 3, C = 2, K = 3, L = 1000 (one full 512-sample tile and a ragged one), from silence and from a random state."""
    torch.manual_seed(11)
    R, C, K, L = 3, 2, 3, 1000
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, C, K, seed=12)
    zi = torch.randn(R, C, K, 2)
    return x, Bs, As, zi, df2(x, Bs, As), df2(x, Bs, As, zi)


def test_zero_state_is_the_old_call():
    from grafx_amd import ops

    x, Bs, As, _, (y64, zf64, peak), _ = wave_case()
    y_old = stateless_meets_the_bound(x, Bs, As, y64, "zero state")
    xc, Bc, Ac = x.cuda(), Bs.cuda(), As.cuda()
    for what, zi in (("zi = zeros", torch.zeros(3, 2, 3, 2, device="cuda")), ("zi = None", None)):
        y, zf = ops.biquad_cascade(xc, Bc, Ac, zi=zi, return_state=True)
        assert torch.equal(y, y_old), f"{what}: the output differs from the stateless call's"
        assert_state_close(zf, zf64, peak, what)


@pytest.mark.parametrize("cuts", [(1,), (2,), (7,), (8,), (9,), (127,), (128,), (129,), (511,), (512,), (513,), (998,), (999,),
                                  tuple(range(37, 1000, 37))], ids=lambda c: f"cut{c[0]}" if len(c) == 1 else "blocks_of_37")
def test_split_equals_whole_on_the_whole_wave_form(cuts):
    from grafx_amd import ops

    x, Bs, As, _, (y64, zf64, peak), _ = wave_case()
    stateless_meets_the_bound(x, Bs, As, y64, "whole wave")
    xc, Bc, Ac = x.cuda(), Bs.cuda(), As.cuda()
    y, zf = in_blocks(xc, Bc, Ac, cuts)
    assert_close(y.cpu(), y64.float(), TOL, f"blocks at {cuts[:3]} vs float64")
    assert_state_close(zf, zf64, peak, f"blocks at {cuts[:3]} vs float64")
    zf_one = ops.biquad_cascade(xc, Bc, Ac, return_state=True)[1]
    assert_state_close(zf, zf_one.cpu().double(), peak, f"blocks at {cuts[:3]} vs the one-call state")


@pytest.mark.parametrize("L", [1, 2, 8, 512, 513])
def test_state_at_short_and_tile_sized_lengths(L):
    """L - 1 in the first sample (w[L-2] is then the ENTERING state), within the first lane, at a tile's last sample and in
    the first sample of the next tile; from a random state, and handed on into a second block of the same length."""
    from grafx_amd import ops

    torch.manual_seed(L)
    R, C, K = 3, 2, 3
    x = torch.randn(R, C, 2 * L)
    Bs, As = coeffs(R, C, K, seed=20 + L)
    zi = torch.randn(R, C, K, 2)
    stateless_meets_the_bound(x, Bs, As, df2(x, Bs, As)[0], f"L = {L}")
    y64, zf64, peak = df2(x, Bs, As, zi)
    y1_64, z1_64, _ = df2(x[..., :L], Bs, As, zi)
    xc, Bc, Ac = x.cuda(), Bs.cuda(), As.cuda()
    y1, z1 = ops.biquad_cascade(xc[..., :L].contiguous(), Bc, Ac, zi=zi.cuda(), return_state=True)
    assert_close(y1.cpu(), y1_64.float(), TOL, f"L = {L}: first block")
    assert_state_close(z1, z1_64, peak, f"L = {L}: first block")
    y2, z2 = ops.biquad_cascade(xc[..., L:].contiguous(), Bc, Ac, zi=z1, return_state=True)
    assert_close(torch.cat([y1, y2], -1).cpu(), y64.float(), TOL, f"L = {L}: both blocks")
    assert_state_close(z2, zf64, peak, f"L = {L}: second block")


def test_non_zero_entering_state():
    from grafx_amd import ops

    x, Bs, As, zi, (y0_64, _, _), (y64, zf64, peak) = wave_case()
    stateless_meets_the_bound(x, Bs, As, y0_64, "entering state")
    assert (y64 - y0_64).abs().max() > 0.1 * y64.abs().max()      # the state is heard
    y, zf = ops.biquad_cascade(x.cuda(), Bs.cuda(), As.cuda(), zi=zi.cuda(), return_state=True)
    assert_close(y.cpu(), y64.float(), TOL, "random zi vs float64")
    assert_state_close(zf, zf64, peak, "random zi")
    y, zf = in_blocks(x.cuda(), Bs.cuda(), As.cuda(), (300, 777), zi=zi.cuda())
    assert_close(y.cpu(), y64.float(), TOL, "random zi in three blocks vs float64")
    assert_state_close(zf, zf64, peak, "random zi in three blocks")


# ---------------------------------------------------------------------------------------------- sixteen-lane form
def test_split_equals_whole_on_the_sixteen_lane_form():
    """8192 stereo rows = 8192 pairs: sixteen lanes per pair, four pairs a wave (one per DPP row), 128-sample tiles.  A
    sample of rows against float64 -- the first and the last pair, and pairs in a wave's second, third and fourth DPP row --
    and every row split against whole."""
    from grafx_amd import ops

    torch.manual_seed(3)
    R, C, K, L = 8192, 2, 2, 300
    rows = [0, 1, 2, 3, 4097, 6002, 7003, 8188, 8191]
    assert {r % 4 for r in rows} == {0, 1, 2, 3}
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, C, K, seed=31)
    zi = torch.randn(R, C, K, 2)
    xc, Bc, Ac, zc = x.cuda(), Bs.cuda(), As.cuda(), zi.cuda()
    y0_64 = df2(x[rows], Bs[rows], As[rows])[0]
    assert_close(ops.biquad_cascade(xc, Bc, Ac)[rows].cpu(), y0_64.float(), TOL, "sixteen lanes: stateless call vs float64")
    y64, zf64, peak = df2(x[rows], Bs[rows], As[rows], zi[rows])
    y_one, zf_one = ops.biquad_cascade(xc, Bc, Ac, zi=zc, return_state=True)
    assert_close(y_one[rows].cpu(), y64.float(), TOL, "sixteen lanes: one call vs float64")
    assert_state_close(zf_one[rows], zf64, peak, "sixteen lanes: one call")
    for cut in (77, 128, 129):
        y, zf = in_blocks(xc, Bc, Ac, (cut,), zi=zc)
        assert_close(y[rows].cpu(), y64.float(), TOL, f"sixteen lanes: cut at {cut} vs float64")
        assert_state_close(zf[rows], zf64, peak, f"sixteen lanes: cut at {cut}")
        assert_close(y, y_one, TOL, f"sixteen lanes: cut at {cut} vs one call, every row")
        assert_close(zf, zf_one, TOL, f"sixteen lanes: cut at {cut} vs one call, every row's state")


# ---------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("R,C,Cf,K,quirk", [(3, 1, 1, 3, False),      # odd row-channel total: the last lane pair has no partner
                                            (3, 1, 2, 3, False), (3, 2, 1, 3, False),
                                            (2, 2, 2, 1, False), (2, 2, 2, 32, False),
                                            (3, 2, 2, 3, True)],     # "ssm" with K = 3: the quirk
                         ids=["odd", "Cin1_Cf2", "Cin2_Cf1", "K1", "K32", "ssm_K3"])
def test_state_geometry(R, C, Cf, K, quirk):
    torch.manual_seed(R + 2 * C + 4 * Cf + K)
    L, cut = 700, 301
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, Cf, K, seed=40 + K + C + 2 * Cf, rmax=0.9 if K == 32 else 0.95, equaliser=K == 32)
    zi = torch.randn(R, max(C, Cf), K, 2)
    stateless_meets_the_bound(x, Bs, As, df2(x, Bs, As, quirk=quirk)[0], "geometry", quirk=quirk)
    y64, zf64, peak = df2(x, Bs, As, zi, quirk=quirk)
    y, zf = in_blocks(x.cuda(), Bs.cuda(), As.cuda(), (cut,), zi=zi.cuda(), quirk=quirk)
    assert_close(y.cpu(), y64.float(), TOL, "two blocks vs float64")
    assert_state_close(zf, zf64, peak, "two blocks")


def test_state_with_a_strided_view_and_an_unaligned_input():
    from grafx_amd import ops

    torch.manual_seed(5)
    B, n, C, K, L, cut = 2, 3, 2, 3, 700, 301
    x = torch.randn(B * n, C, L)
    Bs, As = coeffs(B * n, C, K, seed=51)
    zi = torch.randn(B * n, C, K, 2)
    stateless_meets_the_bound(x, Bs, As, df2(x, Bs, As)[0], "views")
    y64, zf64, peak = df2(x, Bs, As, zi)
    Bc, Ac = Bs.cuda(), As.cuda()
    # a (B, n, C, L) view of a wider buffer, in and out; the rows around it stay untouched
    buf = torch.zeros(B, 8, C, L, device="cuda")
    buf[:, 1:4] = x.view(B, n, C, L).cuda()
    z = zi.cuda()
    for lo, hi in ((0, cut), (cut, L)):
        _, z = ops.biquad_cascade(buf[:, 1:4, :, lo:hi], Bc, Ac, out=buf[:, 4:7, :, lo:hi], zi=z, return_state=True)
    assert_close(buf[:, 4:7].reshape(B * n, C, L).cpu(), y64.float(), TOL, "strided view in two blocks")
    assert_state_close(z, zf64, peak, "strided view in two blocks")
    assert torch.equal(buf[:, 7], torch.zeros_like(buf[:, 7])) and torch.equal(buf[:, 0], torch.zeros_like(buf[:, 0]))
    # rows that start 4 bytes off a 16-byte boundary: the scalar-load branch
    wide = torch.zeros(B * n, C, L + 1, device="cuda")
    wide[..., 1:] = x.cuda()
    xu = wide[..., 1:]
    assert xu.data_ptr() % 16 == 4
    y, z = in_blocks(xu, Bc, Ac, (cut,), zi=zi.cuda())
    assert_close(y.cpu(), y64.float(), TOL, "unaligned input in two blocks")
    assert_state_close(z, zf64, peak, "unaligned input in two blocks")


def test_state_updated_in_place():
    """zi == zf at the C entry: a pair's states are read before its first tile and written in its last."""
    from grafx_amd import _lib, ops

    x, Bs, As, zi, _, (y64, zf64, peak) = wave_case()
    R, C, L = x.shape
    K = Bs.shape[2]
    xc, Bc, Ac, z = x.cuda(), Bs.cuda(), As.cuda(), zi.cuda().clone()
    y = torch.empty_like(xc)
    for lo, hi in ((0, 300), (300, L)):
        xb, yb = xc[..., lo:hi], y[..., lo:hi]
        ops.check(_lib.lib().gfx_biquad_cascade_state_f32(xb.data_ptr(), ops.rowmap(xb)[0], yb.data_ptr(), ops.rowmap(yb)[0],
                                                          Bc.data_ptr(), Ac.data_ptr(), z.data_ptr(), z.data_ptr(), R, C, C, K,
                                                          hi - lo, 0, torch.cuda.current_stream().cuda_stream),
                  "gfx_biquad_cascade_state_f32")
    assert_close(y.cpu(), y64.float(), TOL, "state updated in place")
    assert_state_close(z, zf64, peak, "state updated in place")


def test_first_order_sections_carry_one_state_value():
    from grafx_amd.processors import IIRFilter

    torch.manual_seed(6)
    R, C, K, L, cut = 3, 2, 3, 700, 301
    x = torch.randn(R, C, L)
    pole = torch.tensor([0.5, -0.9, 0.95]).expand(R, 1, K)
    As = torch.stack([1.1 * torch.ones_like(pole), -1.1 * pole], -1)
    Bs = torch.stack([0.7 * torch.ones_like(pole), 0.3 * torch.ones_like(pole)], -1) + 0.05 * torch.randn(R, 1, K, 2)
    zi = torch.randn(R, C, K, 2)
    zi[..., 1] = 0.0
    B3, A3 = torch.nn.functional.pad(Bs, (0, 1)), torch.nn.functional.pad(As, (0, 1))
    stateless_meets_the_bound(x, B3, A3, df2(x, B3, A3)[0], "first order")
    y64, zf64, peak = df2(x, B3, A3, zi)
    m = IIRFilter(order=1, backend="lfilter", flashfftconv=False)
    xc, Bc, Ac = x.cuda(), Bs.cuda(), As.cuda()
    with torch.no_grad():
        y1, z1 = m(xc[..., :cut], Bc, Ac, state=zi.cuda(), return_state=True)
        y2, z2 = m(xc[..., cut:], Bc, Ac, state=z1, return_state=True)
    assert z1.shape == (R, C, K, 2) and not z1[..., 1].any() and not z2[..., 1].any()
    assert_close(torch.cat([y1, y2], -1).cpu(), y64.float(), TOL, "first-order sections in two blocks")
    zf64[..., 1] = 0.0
    assert_state_close(z2, zf64, peak, "first-order sections in two blocks")


# ---------------------------------------------------------------------------------------------- gradients
def grad_err(got, want):
    return ((got.cpu().double() - want).abs().max() / want.abs().max()).item()


@pytest.mark.parametrize("backend,K,C,Cf", [("lfilter", 1, 2, 2), ("lfilter", 3, 2, 2), ("lfilter", 3, 1, 2), ("lfilter", 3, 2, 1),
                                            ("ssm", 2, 2, 2)])
def test_gradients_with_state(backend, K, C, Cf):
    """d(<y, p> + <zf, q>) / d(x, Bs, As, zi) against float64 autograd through the plain loop; L = 600 crosses a tile seam."""
    from grafx_amd.processors import IIRFilter

    torch.manual_seed(7 * K + C + 2 * Cf)
    R, L = 2, 600
    Co = max(C, Cf)
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, Cf, K, seed=60 + K + C + 2 * Cf)
    zi = torch.randn(R, Co, K, 2)
    p, q = torch.randn(R, Co, L), torch.randn(R, Co, K, 2)
    ref = [t.double().requires_grad_(True) for t in (x, Bs, As, zi)]
    y64, zf64, _ = df2(*ref, quirk=backend == "ssm")
    ((y64 * p.double()).sum() + (zf64 * q.double()).sum()).backward()
    ours = [t.cuda().requires_grad_(True) for t in (x, Bs, As, zi)]
    y, zf = IIRFilter(order=2, backend=backend, flashfftconv=False)(*ours[:3], state=ours[3], return_state=True)
    assert (y.detach().cpu().double() - y64.detach()).abs().max() <= 2e-5 * y64.detach().abs().max()
    ((y * p.cuda()).sum() + (zf * q.cuda()).sum()).backward()
    for name, got, want in zip(("x", "Bs", "As", "zi"), ours, ref):
        assert got.grad is not None and got.grad.shape == want.grad.shape, name
        err = grad_err(got.grad, want.grad)
        print(f"{backend} K={K} C={C}/{Cf} grad {name}: {err:.2e}")
        assert err <= GRAD_TOL, f"{backend} K={K} C={C}/{Cf} grad {name}: {err:.2e}"


def test_state_function_takes_cotangents_for_either_output_alone():
    from grafx_amd.autograd import BiquadCascadeStateFn

    torch.manual_seed(8)
    R, C, K, L = 2, 2, 3, 600
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, C, K, seed=70)
    zi = torch.randn(R, C, K, 2)
    q = torch.randn(R, C, K, 2)
    ref = [t.double().requires_grad_(True) for t in (x, Bs, As, zi)]
    (df2(*ref)[1] * q.double()).sum().backward()
    ours = [t.cuda().requires_grad_(True) for t in (x, Bs, As, zi)]
    (BiquadCascadeStateFn.apply(*ours)[1] * q.cuda()).sum().backward()
    for name, got, want in zip(("x", "Bs", "As", "zi"), ours, ref):
        err = grad_err(got.grad, want.grad)
        assert err <= GRAD_TOL, f"state-only loss, grad {name}: {err:.2e}"


def test_back_propagation_through_blocks():
    """Two chained IIRFilter calls over a split signal: the gradients of the one-call run (the stateless BiquadCascadeFn)."""
    from grafx_amd.processors import IIRFilter

    torch.manual_seed(9)
    R, C, K, L, cut = 2, 2, 3, 600, 217
    x = torch.randn(R, C, L)
    Bs, As = coeffs(R, C, K, seed=80)
    p = torch.randn(R, C, L).cuda()
    m = IIRFilter(order=2, backend="lfilter", flashfftconv=False)
    one = [t.cuda().requires_grad_(True) for t in (x, Bs, As)]
    (m(*one) * p).sum().backward()
    two = [t.cuda().requires_grad_(True) for t in (x, Bs, As)]
    y1, s = m(two[0][..., :cut], two[1], two[2], return_state=True)
    y2, s = m(two[0][..., cut:], two[1], two[2], state=s, return_state=True)
    assert s.requires_grad
    (torch.cat([y1, y2], -1) * p).sum().backward()
    for name, got, want in zip(("x", "Bs", "As"), two, one):
        err = grad_err(got.grad, want.grad.cpu().double())
        print(f"through blocks, grad {name}: {err:.2e}")
        assert err <= GRAD_TOL, f"through blocks, grad {name}: {err:.2e}"


# ---------------------------------------------------------------------------------------------- surface
def test_the_frequency_sampled_backend_refuses_state():
    from grafx_amd.processors import IIRFilter

    m = IIRFilter(order=2, backend="fsm", flashfftconv=False, fsm_fir_len=64)
    x, (Bs, As) = torch.randn(2, 2, 256).cuda(), (t.cuda() for t in coeffs(2, 2, 1, seed=90))
    with pytest.raises(ValueError, match="no recursive state.*recursive backends"):
        m(x, Bs, As, state=torch.zeros(2, 2, 1, 2, device="cuda"))
    with pytest.raises(ValueError, match="no recursive state.*recursive backends"):
        m(x, Bs, As, return_state=True)


def test_bad_states_are_refused():
    from grafx_amd import ops
    from grafx_amd.processors import IIRFilter

    x, (Bs, As) = torch.randn(2, 2, 64).cuda(), (t.cuda() for t in coeffs(2, 2, 3, seed=91))
    for bad in (torch.zeros(2, 2, 3, device="cuda"), torch.zeros(2, 2, 2, 2, device="cuda"), torch.zeros(2, 1, 3, 2, device="cuda"),
                torch.zeros(2, 2, 3, 2, device="cuda", dtype=torch.float64), torch.zeros(2, 2, 3, 2),
                torch.zeros(2, 2, 3, 4, device="cuda")[..., ::2]):
        with pytest.raises(ValueError):
            ops.biquad_cascade(x, Bs, As, zi=bad)
    m = IIRFilter(order=2, backend="lfilter", flashfftconv=False)
    with pytest.raises(ValueError):
        m(x, Bs, As, state=torch.zeros(2, 2, 2, 2, device="cuda"))
    with pytest.raises(ValueError):
        m(x, Bs.requires_grad_(), As, state=torch.zeros(2, 2, 2, 2, device="cuda"))


@pytest.mark.parametrize("channel", ["mono", "stereo", "midside"])
def test_parametric_equalizer_in_two_blocks(channel):
    import grafx_amd.processors as P

    torch.manual_seed(10)
    R, K, L, cut = 3, 4, 900, 401
    m = P.ParametricEqualizer(num_filters=K, processor_channel=channel, backend="lfilter", flashfftconv=False).cuda()
    params = {k: 0.3 * torch.randn(R, *shape, device="cuda") for k, shape in m.parameter_size().items()}
    x = torch.randn(R, 2, L, device="cuda")
    with torch.no_grad():
        want = m(x, **params)
        y1, s = m(x[..., :cut], **params, return_state=True)
        y2, s2 = m(x[..., cut:], **params, state=s, return_state=True)
        y2_only = m(x[..., cut:], **params, state=s)
    assert s.shape == (R, 2, K, 2) and s2.shape == s.shape and torch.equal(y2, y2_only)
    assert_close(torch.cat([y1, y2], -1).cpu(), want.cpu(), TOL, f"ParametricEqualizer({channel}) in two blocks")
    assert (torch.cat([y1, m(x[..., cut:], **params)], -1) - want).abs().max() > 1e-3 * want.abs().max()    # the seam without it


def test_biquad_filter_in_two_blocks():
    import grafx_amd.processors as P

    torch.manual_seed(12)
    R, K, L, cut = 3, 2, 900, 401
    m = P.BiquadFilter(num_filters=K, backend="lfilter", flashfftconv=False).cuda()
    params = {k: 0.3 * torch.randn(R, *((shape,) if isinstance(shape, int) else shape), device="cuda")
              for k, shape in m.parameter_size().items()}
    x = torch.randn(R, 2, L, device="cuda")
    with torch.no_grad():
        want = m(x, **params)
        y1, s = m(x[..., :cut], **params, return_state=True)
        y2, s = m(x[..., cut:], **params, state=s, return_state=True)
    assert s.shape == (R, 2, K, 2)
    assert_close(torch.cat([y1, y2], -1).cpu(), want.cpu(), TOL, "BiquadFilter in two blocks")
