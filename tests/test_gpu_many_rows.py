"""Kernel entry points at row counts beyond the launch-grid limits ("Row counts and launch geometry").

The other GPU files sweep the length of a row; here the rows are short and there are more than 65 535 of them, so that
the row loops of the capped grids (`for (r = blockIdx.y; r < R; r += gridDim.y)`), the host-side launch splits and the
32-bit block arithmetic of the entries whose rows ride on grid.x all run past their first lap.

Every case is built so that a wrong row cannot pass: signals and every per-row parameter are drawn per row from a seeded
generator and row r is scaled by a power of two that depends on r (`_scale`), outputs passed as ``out=`` start as NaN, and

* check A compares with the float64 evaluation of the same formulas on the CPU, row by row (conftest.assert_close_rows),
  at the tolerance the existing small-shape test of the op asserts (cited at each use; conftest.NORTH_STAR_TOL where the
  op has only been tested through a processor);
* check B requires the big call to equal, bit for bit, the same op on slices of at most 4096 rows: the first rows, the
  rows around 65 535, the last rows (ops whose rows are independent and whose kernel does not depend on the launch size).

Parameters stay in the ranges of the existing tests (standard deviation <= 1 around the initial values), where the
float32 oracle itself is within the same tolerances of float64: the float64 formulas below are the oracle's own
(oracle.processors / oracle.lti on .double() inputs) or plain torch, and none of them depends on the row count.
"""
import math
import zlib

import pytest
import torch

import oracle
from conftest import NORTH_STAR_TOL, assert_close_rows
from oracle.lti import linear_convolve

pytestmark = pytest.mark.gpu

R_EDGE = (65535, 65536, 65601)
R_BIG = 65601
KNEES = ("hard", "quadratic", "exponential")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _scale(R, span=11):
    """Row r scaled by 2 ** ((7 r) % span - span // 2): a row processed with another row's data is an O(1) error."""
    return torch.exp2(((torch.arange(R) * 7) % span - span // 2).float())


def _signal(g, R, C, L, span=11):
    return torch.randn(R, C, L, generator=g) * _scale(R, span)[:, None, None]


def _slices(R, edge=65535):
    """First rows, the rows around `edge` (where the second lap / the second launch starts), last rows."""
    out = [slice(0, min(R, 4096)), slice(max(0, R - 4096), R)]
    if edge - 8 < R:
        out.insert(1, slice(max(0, edge - 8), min(R, edge + 8)))
    return out


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _view(x, n):
    """The rows of x (R, C, L) as a strided (R / n, n, C, L) view of a larger buffer (the render's signal buffer)."""
    R, C, L = x.shape
    buf = _nan(R // n, n + 1, C, L)
    buf[:, :n] = x.view(R // n, n, C, L)
    return buf[:, :n]


def _inner(R):
    return 3 if R % 3 == 0 else 1


def _same_bits(big, fn, R, what, edge=65535):
    """Check B: fn(slice) -> the op on those rows alone; must equal the big call's rows bit for bit."""
    for s in _slices(R, edge):
        part = fn(s)
        assert torch.equal(big[s], part), f"{what}: rows {s.start}..{s.stop} differ from the same rows computed alone"


def _finite(t, what):
    assert torch.isfinite(t).all(), f"{what}: rows left unwritten (NaN sentinel) or not finite"


def _dyn_params(g, R):
    # around the processors' initial values with the spread create_empty_parameters(std <= 1) gives them (thresholds
    # within 2.5 standard deviations: T = log_threshold - 6 stays between the loud and the silent anchor of test_dyn_gain)
    return (torch.randn(R, generator=g).clamp(-2.5, 2.5), 0.5 * torch.randn(R, generator=g), 0.5 * torch.randn(R, generator=g))


def _log_gain64(G, lt, lr, lk, knee, gate):
    m = (oracle.OracleNoiseGate if gate else oracle.OracleCompressor)(energy_smoother=None, knee=knee)
    return m.log_gain(G, lt.double()[:, None] - 6, lr.double()[:, None], lk.double()[:, None])


# ------------------------------------------------------------------------------------- capped grid.y + row loop
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("R,C,L", [(R_BIG, 2, 64), (R_BIG, 1, 5), (65535, 2, 1), (65536, 1, 260)])
def test_energy(R, C, L, view):
    from grafx_amd import ops

    x = _signal(_gen("energy", R, C, L), R, C, L)
    xd = _view(x.cuda(), _inner(R)) if view else x.cuda()
    e = ops.energy(xd)
    # tolerance: the op is tested through the dynamics processors only -> the north star
    assert_close_rows(e.cpu(), x.double().square().mean(1), NORTH_STAR_TOL, f"energy R={R}")
    flat = x.cuda()
    _same_bits(e, lambda s: ops.energy(flat[s]), R, "energy")


@pytest.mark.parametrize("R,C,L,exp_gain,view", [(65535, 2, 64, False, False), (65536, 2, 64, True, True), (R_BIG, 2, 64, False, True),
                                                 (R_BIG, 2, 64, True, False), (R_BIG, 1, 1, True, True), (R_BIG, 2, 5, False, False),
                                                 (R_BIG, 1, 260, False, True), (R_BIG, 1, 260, True, False)])
def test_apply_gain(R, C, L, exp_gain, view):
    from grafx_amd import ops

    g = _gen("apply_gain", R, C, L, exp_gain)
    x, gain = _signal(g, R, C, L), 0.5 * torch.randn(R, L, generator=g)
    n = _inner(R)
    out = _view(_nan(R, C, L), n) if view else _nan(R, C, L)
    y = ops.apply_gain(_view(x.cuda(), n) if view else x.cuda(), gain.cuda(), exp_gain=exp_gain, out=out)
    y = y.reshape(R, C, L)
    _finite(y, "apply_gain")
    gd = gain.double().exp() if exp_gain else gain.double()
    # tolerance: tested through the dynamics processors only -> the north star
    assert_close_rows(y.cpu(), gd[:, None, :] * x.double(), NORTH_STAR_TOL, f"apply_gain R={R}")
    xc, gc = x.cuda(), gain.cuda()
    _same_bits(y, lambda s: ops.apply_gain(xc[s], gc[s], exp_gain=exp_gain), R, "apply_gain")


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("R,C,L", [(R_BIG, 1, 64), (R_BIG, 2, 64), (65536, 2, 5), (R_BIG, 2, 260)])
def test_stereo_gain(R, C, L, view):
    from grafx_amd import ops

    g = _gen("stereo_gain", R, C, L)
    x, lg = _signal(g, R, C, L), 0.5 * torch.randn(R, 2, generator=g)
    n = _inner(R)
    out = _view(_nan(R, 2, L), n) if view else _nan(R, 2, L)
    y = ops.stereo_gain(_view(x.cuda(), n) if view else x.cuda(), lg.cuda(), out=out).reshape(R, 2, L)
    _finite(y, "stereo_gain")
    want = oracle.OracleStereoGain()(x.double().expand(R, 2, L), lg.double())
    # tolerance: test_gpu_processors / smoke reach it through StereoGain only -> the north star
    assert_close_rows(y.cpu(), want, NORTH_STAR_TOL, f"stereo_gain R={R} C={C}")
    xc, lc = x.cuda(), lg.cuda()
    _same_bits(y, lambda s: ops.stereo_gain(xc[s], lc[s]), R, "stereo_gain")


@pytest.mark.parametrize("log_out", [False, True])
@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("knee", KNEES)
def test_dyn_gain(knee, gate, log_out):
    """Every row holds one loud and one silent sample (energy 100 and 0: 8 above and 3 below any threshold here), so that
    its log-gain has an O(1) peak whatever the rest of the row does: a row that merely grazes its threshold has a log-gain
    of ~1e-3 that is the difference of two numbers near 10, i.e. ~1e-4 relative in ANY float32 evaluation."""
    from grafx_amd import ops

    R, L = R_BIG, 64
    g = _gen("dyn_gain", knee, gate, log_out)
    env = (torch.randn(R, L, generator=g) * _scale(R)[:, None]).square()
    env[:, 0], env[:, 1] = 100.0, 0.0
    lt, lr, lk = _dyn_params(g, R)
    got = ops.dyn_gain(env.cuda(), lt.cuda(), lr.cuda(), lk.cuda(), knee, gate, log_out)
    want = _log_gain64(torch.log(env.double() + 1e-5), lt, lr, lk, knee, gate)
    # tolerance: tested through Compressor / NoiseGate only -> the north star
    assert_close_rows(got.cpu(), want if log_out else want.exp(), NORTH_STAR_TOL, f"dyn_gain {knee} gate={gate}")
    ec, p = env.cuda(), [t.cuda() for t in (lt, lr, lk)]
    _same_bits(got, lambda s: ops.dyn_gain(ec[s], p[0][s], p[1][s], p[2][s], knee, gate, log_out), R, "dyn_gain")


@pytest.mark.parametrize("R,C,L,knee,gate,param_rows",
                         [(R_BIG, 2, 64, k, g, p) for k in KNEES for g in (False, True) for p in (None, 5)]
                         + [(65536, 1, 260, "quadratic", g, p) for g in (False, True) for p in (None, 5)])
def test_dyn_gain_apply(R, C, L, knee, gate, param_rows):
    from grafx_amd import ops

    g = _gen("dyn_gain_apply", R, C, L, knee, gate, param_rows)
    x = _signal(g, R, C, L)
    env = (torch.randn(R, L, generator=g) * _scale(R)[:, None]).square()
    P = R if param_rows is None else param_rows
    lt, lr, lk = _dyn_params(g, P)
    n = _inner(R)
    y = ops.dyn_gain_apply(_view(x.cuda(), n), env.cuda(), lt.cuda(), lr.cuda(), lk.cuda(), knee, gate,
                           out=_view(_nan(R, C, L), n), param_rows=param_rows).reshape(R, C, L)
    _finite(y, "dyn_gain_apply")
    idx = torch.arange(R) % P
    gain = _log_gain64(torch.log(env.double() + 1e-5), lt[idx], lr[idx], lk[idx], knee, gate).exp()
    # tolerance: tested through Compressor / NoiseGate only -> the north star
    assert_close_rows(y.cpu(), gain[:, None, :] * x.double(), NORTH_STAR_TOL, f"dyn_gain_apply {knee} gate={gate}")
    if param_rows is None:   # (with shared parameters a slice would have to start on a multiple of param_rows)
        xc, ec, p = x.cuda(), env.cuda(), [t.cuda() for t in (lt, lr, lk)]
        _same_bits(y, lambda s: ops.dyn_gain_apply(xc[s], ec[s], p[0][s], p[1][s], p[2][s], knee, gate), R, "dyn_gain_apply")


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("knee", KNEES)
def test_dyn_gain_bwd(knee, gate):
    """Against float64 autograd of the oracle's gain curve.  x and gy are positive, so that the three parameter gradients
    of a row are sums of terms of one sign: their float32 error stays relative to the row's own values.  With the quadratic
    knee the envelope is drawn per row on the sloped side of ITS knee (0.5 .. 3.5 above T + W for the compressor, between
    the floor log(1e-5) and T - W - 0.5 for the gate): inside the knee the slope is proportional to G - (T -+ W), a
    difference of two numbers near 10 known to ~1e-6, so a sample that grazes the knee has a slope -- and an envelope
    gradient -- good to ~1e-3 only in ANY float32 evaluation, the reference's included; that is a property of the curve,
    not of the row count (the knee's inside is compared at small shapes through the processors' gradient tests)."""
    from grafx_amd import ops

    R, C, L = R_BIG, 2, 64     # (L <= 256: one workgroup per row, so the parameter sums have one order -> check B)
    g = _gen("dyn_gain_bwd", knee, gate)
    x, gy = _signal(g, R, C, L).abs(), torch.randn(R, C, L, generator=g).abs()
    env = (torch.randn(R, L, generator=g) * _scale(R)[:, None]).square()
    lt, lr, lk = _dyn_params(g, R)
    if knee == "quadratic":
        lk = lk.clamp(-1, 1)
        T, W, u = lt.double()[:, None] - 6, lk.double().exp()[:, None] / 2, torch.rand(R, L, generator=g).double()
        Gt = (T - W - 0.5) - u * (T - W - 0.5 + 11.4) if gate else T + W + 0.5 + 3 * u
        env = (Gt.exp() - 1e-5).float()
    gain, denv, gp = ops.dyn_gain_bwd(x.cuda(), gy.cuda(), env.cuda(), lt.cuda(), lr.cuda(), lk.cuda(), knee, gate)
    e64 = env.double().requires_grad_(True)
    p64 = [t.double().requires_grad_(True) for t in (lt, lr, lk)]
    gain64 = _log_gain64(torch.log(e64 + 1e-5), *p64, knee, gate).exp()
    ((gy.double() * x.double()).sum(1) * gain64).sum().backward()
    # tolerance: tested through the compressor's training step only -> the north star
    assert_close_rows(gain.cpu(), gain64.detach(), NORTH_STAR_TOL, f"dyn_gain_bwd gain {knee} gate={gate}")
    assert_close_rows(denv.cpu(), e64.grad, NORTH_STAR_TOL, f"dyn_gain_bwd denv {knee} gate={gate}")
    want_gp = torch.stack([torch.zeros(R, dtype=torch.float64) if p.grad is None else p.grad for p in p64], -1)
    if knee == "hard":
        want_gp, gp = want_gp[:, :2], gp[:, :2]      # no knee parameter
    assert_close_rows(gp.cpu(), want_gp, NORTH_STAR_TOL, f"dyn_gain_bwd gparams {knee} gate={gate}")
    c = [t.cuda() for t in (x, gy, env, lt, lr, lk)]
    for k, big in enumerate((gain, denv, gp)):
        _same_bits(big, lambda s: ops.dyn_gain_bwd(*(t[s] for t in c), knee, gate)[k][:, : big.shape[1]], R, "dyn_gain_bwd")
    # the inside of the knee and signed samples beyond the first lap: bits only (no tolerance involved)
    c[0], c[1] = _signal(g, R, C, L).cuda(), torch.randn(R, C, L, generator=g).cuda()
    c[2] = (torch.randn(R, L, generator=g) * _scale(R)[:, None]).square().cuda()
    free = ops.dyn_gain_bwd(*c, knee, gate)
    for k, big in enumerate(free):
        _finite(big, "dyn_gain_bwd")
        _same_bits(big, lambda s: ops.dyn_gain_bwd(*(t[s] for t in c), knee, gate)[k], R, "dyn_gain_bwd (any envelope)")


@pytest.mark.parametrize("R,C,L", [(R_BIG, 2, 64), (65536, 1, 5), (R_BIG, 1, 260)])
def test_dyn_dx(R, C, L):
    from grafx_amd import ops

    g = _gen("dyn_dx", R, C, L)
    x, gy = _signal(g, R, C, L), torch.randn(R, C, L, generator=g)
    gain, de = torch.rand(R, L, generator=g), torch.randn(R, L, generator=g)
    n = _inner(R)
    gx = ops.dyn_dx(_view(x.cuda(), n), _view(gy.cuda(), n), gain.cuda(), de.cuda())
    want = gain.double()[:, None] * gy.double() + (2.0 / C) * de.double()[:, None] * x.double()
    # tolerance: tested through the compressor's training step only -> the north star
    assert_close_rows(gx.cpu(), want, NORTH_STAR_TOL, f"dyn_dx R={R}")
    c = [t.cuda() for t in (x, gy, gain, de)]
    _same_bits(gx, lambda s: ops.dyn_dx(*(t[s] for t in c)), R, "dyn_dx")


@pytest.mark.parametrize("R,iir_len", [(R_BIG, 1), (R_BIG, 64), (R_BIG, 300), (65535, 64), (65536, 300)])
def test_onepole_fir(R, iir_len):
    from grafx_amd import ops

    # (standard deviation 1, as the processors' parameters: the reference forms 1 - sigmoid(z) in float32, good to
    # 6e-8 / (1 - a) relative, i.e. within the tolerance only while a <= 0.994, z <= 5)
    z = torch.randn(R, generator=_gen("onepole_fir", R, iir_len))
    h = ops.onepole_fir(z.cuda(), iir_len)
    # tolerance: tested through the compressor's "iir" smoother only -> the north star
    assert_close_rows(h.cpu(), oracle.one_pole_fir(z.double()[:, None], iir_len), NORTH_STAR_TOL, f"onepole_fir N={iir_len}")
    zc = z.cuda()
    _same_bits(h, lambda s: ops.onepole_fir(zc[s], iir_len), R, "onepole_fir")


def _waveshaper64(x, mode, pre, p0, p1, inverse_post, remove_dc):
    x = x.double()
    pre = pre.double().exp()[:, None, None]
    u = pre * (x - (x.mean(-1, keepdim=True) if remove_dc else 0))
    if mode == 0:
        b = p0.double()[:, None, None]
        y = torch.tanh(u + b) - torch.tanh(b)
    elif mode == 1:   # nonlinear.py:163-166: thresholds split as (kn, kp), hardness as (gp, gn)
        gp, gn = (p0.double()[:, k, None, None].exp() for k in (0, 1))
        kn, kp = (torch.sigmoid(p1.double()[:, k, None, None]) for k in (0, 1))
        bp, bn = torch.tanh(kp), -torch.tanh(kn)
        hi = (1 - bp) / gp * torch.tanh(gp * (u - kp)) + bp
        lo = (1 + bn) / gn * torch.tanh(gn * (u + kn)) + bn
        y = torch.where(u > kp, hi, torch.where(u < -kn, lo, torch.tanh(u)))
    else:
        w = torch.tanh(p0.double())
        terms = [torch.ones_like(u), u]
        for k in range(2, w.shape[1]):
            terms.append(terms[-1] * u if mode == 2 else 2 * u * terms[-1] - terms[-2])
        y = sum(w[:, k, None, None] * terms[k] for k in range(w.shape[1]))
    return y / pre if inverse_post else y


@pytest.mark.parametrize("mode,R,remove_dc,misaligned",
                         [(0, 65535, False, False), (0, 65536, True, True)]
                         + [(m, R_BIG, dc, mis) for m in range(4) for dc, mis in ((False, False), (True, False), (True, True))])
def test_waveshaper(mode, R, remove_dc, misaligned):
    """Rows scaled by 1/4 .. 4 (a narrower span than elsewhere: a row of tiny samples through tanh(u + b) - tanh(b) is a
    difference of two O(1) numbers in any float32 evaluation)."""
    from grafx_amd import ops

    C, L = 2, 37 if misaligned else 64
    g = _gen("waveshaper", mode, R, remove_dc, misaligned)
    x = _signal(g, R, C, L, span=5)
    pre = 0.3 * torch.randn(R, generator=g)
    p0 = 0.3 * torch.randn(*((R,) if mode == 0 else (R, 2) if mode == 1 else (R, 4)), generator=g)
    p1 = torch.randn(R, 2, generator=g) if mode == 1 else None
    inv = mode < 2
    if misaligned:    # rows that start 4 bytes off a 16-byte boundary: the scalar path
        base = torch.empty(R * C * L + 1, device="cuda")
        xd = base[1:].view(R, C, L)
        xd.copy_(x)
    else:
        xd = x.cuda()
    kw = dict(log_pre_gain=pre.cuda(), p0=p0.cuda(), p1=None if p1 is None else p1.cuda(), inverse_post_gain=inv,
              remove_dc=remove_dc)
    y = ops.waveshaper(xd, mode, out=_nan(R, C, L), **kw)
    _finite(y, "waveshaper")
    # tolerance: test_gpu_next_rows2.py::test_waveshapers asserts 2e-5 (and conftest holds every test outside the
    # committed allow-list to 1e-5)
    assert_close_rows(y.cpu(), _waveshaper64(x, mode, pre, p0, p1, inv, remove_dc), 2e-5, f"waveshaper mode {mode} R={R}")

    def alone(s):
        k = dict(kw, log_pre_gain=kw["log_pre_gain"][s], p0=kw["p0"][s], p1=None if p1 is None else kw["p1"][s])
        return ops.waveshaper(xd[s], mode, **k)

    if not misaligned:     # (a slice of the misaligned view starts on another alignment: another code path)
        _same_bits(y, alone, R, "waveshaper")


@pytest.mark.parametrize("R,C,L", [(R_BIG, 2, 64), (65536, 1, 5), (524297, 2, 8)])
def test_row_mean(R, C, L):
    """(524297, 2): 16 * 65535 + 34 row-channels, past the kernel's own grid cap.  Rows carry an offset of three times
    their scale, so that every mean is compared relative to itself."""
    from grafx_amd import ops

    g = _gen("row_mean", R, C, L)
    x = (torch.randn(R, C, L, generator=g) + 3) * _scale(R)[:, None, None]
    n = _inner(R)
    m = ops.row_mean(_view(x.cuda(), n))
    # tolerance: tested through the remove_dc option of the distortions only -> the north star
    assert_close_rows(m.cpu().view(-1, 1), x.double().mean(-1).view(-1, 1), NORTH_STAR_TOL, f"row_mean R={R}")
    xc = x.cuda()
    _same_bits(m.view(R, C), lambda s: ops.row_mean(xc[s]).view(-1, C), R, "row_mean")


# ------------------------------------------------------------------------------------- host-side launch split
@pytest.mark.parametrize("R", R_EDGE)
@pytest.mark.parametrize("n", [8, 65])
def test_rdft(R, n):
    from grafx_amd import ops

    x = torch.randn(R, n, generator=_gen("rdft", R, n)) * _scale(R)[:, None]
    X = torch.view_as_real(ops.rdft(x.cuda())).reshape(R, -1)
    want = torch.view_as_real(torch.fft.rfft(x.double())).reshape(R, -1)
    assert_close_rows(X.cpu(), want, 2e-6, f"rdft n={n} R={R}")     # test_gpu_small_dft.py::test_rdft_matches_rfft
    xc = x.cuda()
    _same_bits(X, lambda s: torch.view_as_real(ops.rdft(xc[s])).reshape(s.stop - s.start, -1), R, "rdft")


@pytest.mark.parametrize("R", R_EDGE)
def test_stft(R):
    from grafx_amd import ops

    T, n_fft, hop = 40, 16, 4
    x = (torch.rand(R, T, generator=_gen("stft", R)) * 2 - 1) * _scale(R)[:, None]
    w = torch.hann_window(n_fft)
    got = torch.view_as_real(ops.stft(x.cuda(), w.cuda(), hop))
    want = torch.view_as_real(torch.stft(x.double(), n_fft=n_fft, hop_length=hop, window=w.double(), return_complex=True))
    assert got.shape == want.shape
    # test_gpu_next_rows2.py::test_native_stft_matches_torch_stft
    assert_close_rows(got.reshape(R, -1).cpu(), want.reshape(R, -1), 2e-6, f"stft R={R}")
    xc, wc = x.cuda(), w.cuda()
    _same_bits(got, lambda s: torch.view_as_real(ops.stft(xc[s], wc, hop)), R, "stft")


@pytest.mark.parametrize("fade", [False, True])
@pytest.mark.parametrize("R,C", [(32767, 2), (32768, 2), (40001, 2), (65601, 1), (21900, 3)])
def test_noise_shaping_ir(R, C, fade):
    """(32768, 2) and (40001, 2): 65 535 row-channels per launch is an odd number, the second launch of a stereo call used
    to start in the middle of a row (and the call to fail)."""
    from grafx_amd import ops

    K, ir_len, T = 4, 48, 64
    g = _gen("noise_shaping_ir", R, C, fade)
    noise = torch.rand(C, K, T, generator=g) * 2 - 1
    ld, lf, zf = (torch.randn(R, C, K, generator=g) for _ in range(3))
    lgain = torch.randn(R, C, K, generator=g) * _scale(R)[:, None, None]
    lo, hi = -0.2, -0.005    # log-amplitude slopes per sample (FilteredNoiseShapingReverb's are of this sign; short IR)
    dev = lambda t: t.cuda()  # noqa: E731
    ir = ops.noise_shaping_ir(dev(noise), dev(ld), dev(lgain), dev(lf) if fade else None, dev(zf) if fade else None,
                              ir_len, lo, hi)
    t = torch.arange(ir_len, dtype=torch.float64)
    lo32, hi32 = float(torch.tensor(lo)), float(torch.tensor(hi))      # the entry takes them as float32
    d = torch.sigmoid(ld.double()) * (hi32 - lo32) + lo32
    env = torch.exp(t * d[..., None])
    if fade:
        f = torch.sigmoid(lf.double()) * (d - lo32) + lo32
        env = env - torch.sigmoid(zf.double())[..., None] * torch.exp(t * f[..., None])
    want = (noise.double()[None, :, :, :ir_len] * lgain.double()[..., None] * env).sum(2)
    # tolerance: tested through FilteredNoiseShapingReverb only -> the north star
    assert_close_rows(ir.cpu(), want, NORTH_STAR_TOL, f"noise_shaping_ir R={R} C={C}")
    c = [dev(p) for p in (ld, lgain, lf, zf)]
    _same_bits(ir, lambda s: ops.noise_shaping_ir(dev(noise), c[0][s], c[1][s], c[2][s] if fade else None,
                                                  c[3][s] if fade else None, ir_len, lo, hi), R, "noise_shaping_ir",
               edge=65535 // C)


@pytest.fixture
def small_alias_workspace():
    from grafx_amd import ops

    old = ops.set_alias_workspace_cap(1 << 30)     # keep the chirp-z workspace of these row counts at 1 GiB
    yield
    ops.set_alias_workspace_cap(old)


@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("rows,rows_per_chunk", [(R_BIG, None), (R_BIG, 1024), (R_BIG, 16383), (R_BIG, 16384), (R_BIG, 70000),
                                                 (40001, None), (40001, 16384), (40001, 70000)])
def test_odd_alias(rows, pairs, rows_per_chunk, monkeypatch, small_alias_workspace):
    """rows_per_chunk above what one call of the one-transform-per-row entry accepts (16 383 rows) is clamped, not refused."""
    from grafx_amd import ops

    monkeypatch.setattr(ops, "ALIAS_PAIRS", pairs)
    P = 101
    z = torch.randn(rows, P, generator=_gen("odd_alias", rows, pairs, rows_per_chunk)) * _scale(rows)[:, None]
    got = ops.odd_alias(z.cuda(), rows_per_chunk=rows_per_chunk)
    want = torch.fft.irfft(torch.fft.rfft(z.double()))
    # tolerance: test_gpu_odd_alias.py::test_odd_alias_matches_float64_fft (3e-6 below P = 700 000)
    assert_close_rows(got.cpu(), want, 3e-6, f"odd_alias rows={rows} pairs={pairs} chunk={rows_per_chunk}")
    if not pairs:     # (the pair form scales a row by its partner's maximum too: a slice pairs the same rows only from an even start)
        zc = z.cuda()
        _same_bits(got, lambda s: ops.odd_alias(zc[s], rows_per_chunk=rows_per_chunk), rows, "odd_alias")


@pytest.mark.parametrize("rows_per_chunk", [1024, 16384, 70000])
def test_odd_alias_adjoint(rows_per_chunk, small_alias_workspace):
    from grafx_amd import ops

    rows, P = R_BIG, 101
    g = torch.randn(rows, P - 1, generator=_gen("odd_alias_adjoint", rows_per_chunk)) * _scale(rows)[:, None]
    got = ops.odd_alias_adjoint(g.cuda(), P, rows_per_chunk=rows_per_chunk)
    zd = torch.zeros(rows, P, dtype=torch.float64, requires_grad=True)
    torch.fft.irfft(torch.fft.rfft(zd)).backward(g.double())
    # tolerance: test_gpu_odd_alias.py::test_odd_alias_adjoint_matches_float64_autograd
    assert_close_rows(got.cpu(), zd.grad, 3e-6, f"odd_alias_adjoint chunk={rows_per_chunk}")
    gc = g.cuda()
    _same_bits(got, lambda s: ops.odd_alias_adjoint(gc[s], P, rows_per_chunk=rows_per_chunk), rows, "odd_alias_adjoint")


# ------------------------------------------------------------------------------------- rows on grid.x
def _fir64(x, h, h_rows, Lout):
    """y[r, c, n] = sum_k h[r % h_rows, cf, k] x[r, cx, n - k] in float64, channels broadcast."""
    R, L = x.shape[0], x.shape[-1]
    hh = h.double()[torch.arange(R) % h_rows]
    C = max(x.shape[1], hh.shape[1])
    xx, hh = x.double().expand(R, C, L), hh.expand(R, C, hh.shape[-1])
    y = torch.zeros(R, C, Lout, dtype=torch.float64)
    for k in range(hh.shape[-1]):
        n = min(L, Lout - k)
        if n > 0:
            y[..., k : k + n] += hh[..., k : k + 1] * xx[..., :n]
    return y


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("h_rows", [None, 3])
@pytest.mark.parametrize("N,L,Cin,Cf", [(5, 64, 2, 1), (5, 64, 1, 2), (300, 64, 1, 1)])
def test_fftconv(N, L, Cin, Cf, h_rows, view):
    """fir_spectrum + fftconv, schedule "tile" pinned for check B ("auto" may take the persistent kernel for a launch of
    this size and the tile kernel for a slice); "auto" itself is held to check A, with tee= where the shape allows it."""
    from grafx_amd import ops

    R = R_BIG
    g = _gen("fftconv", N, L, Cin, Cf, h_rows)
    x = _signal(g, R, Cin, L)
    hr = R if h_rows is None else h_rows
    h = torch.randn(hr, Cf, N, generator=g) * _scale(hr)[:, None, None] / math.sqrt(N)
    Hs = ops.fir_spectrum(h.cuda().reshape(hr * Cf, N))
    n, Cout = _inner(R), max(Cin, Cf)
    xd = _view(x.cuda(), n) if view else x.cuda()
    want = _fir64(x, h, hr, L)
    y = ops.fftconv(xd, Hs, N, Cf, out=_view(_nan(R, Cout, L), n) if view else _nan(R, Cout, L), h_rows=h_rows,
                    schedule="tile").reshape(R, Cout, L)
    _finite(y, "fftconv")
    assert_close_rows(y.cpu(), want, 1e-5, f"fftconv tile N={N}")       # test_gpu_fftconv.py::test_single_partition_causal
    tee = _nan(R, Cin, L) if ops.fftconv_can_tee(Cin, Cf, L, L, 0, N) else None
    ya = ops.fftconv(xd, Hs, N, Cf, out=_nan(R, Cout, L), tee=tee, h_rows=h_rows)
    _finite(ya, "fftconv auto")
    assert_close_rows(ya.cpu(), want, 1e-5, f"fftconv auto N={N}")
    if tee is not None:
        assert torch.equal(tee, x.cuda()), "fftconv tee: the copy of the input differs"
    if h_rows is None:
        xc, hc = x.cuda(), h.cuda()
        _same_bits(y, lambda s: ops.fftconv(xc[s], ops.fir_spectrum(hc[s].reshape(-1, N)), N, Cf, schedule="tile"), R, "fftconv")


@pytest.mark.parametrize("h_rows", [None, 3])
@pytest.mark.parametrize("N,Cin,Cf", [(5, 2, 1), (65, 1, 2)])
def test_fir_direct(N, Cin, Cf, h_rows):
    from grafx_amd import ops

    R, L = R_BIG, 64
    g = _gen("fir_direct", N, Cin, Cf, h_rows)
    x = _signal(g, R, Cin, L)
    hr = R if h_rows is None else h_rows
    h = torch.randn(hr, Cf, N, generator=g) * _scale(hr)[:, None, None] / math.sqrt(N)
    n, Cout = _inner(R), max(Cin, Cf)
    y = ops.fir_direct(_view(x.cuda(), n), h.cuda(), out=_view(_nan(R, Cout, L), n), h_rows=hr).reshape(R, Cout, L)
    _finite(y, "fir_direct")
    # tolerance: the one of the convolution it replaces (test_gpu_fftconv.py::test_single_partition_causal)
    assert_close_rows(y.cpu(), _fir64(x, h, hr, L), 1e-5, f"fir_direct N={N}")
    if h_rows is None:
        xc, hc = x.cuda(), h.cuda()
        _same_bits(y, lambda s: ops.fir_direct(xc[s], hc[s]), R, "fir_direct")


@pytest.mark.parametrize("K,C,Cf", [(1, 2, 1), (3, 1, 2), (3, 2, 2)])
def test_biquad_cascade(K, C, Cf):
    """Check B on slices of 16 384 rows: from 8192 pairs of row-channels on the cascade runs on the sixteen-lanes-per-pair
    kernel, as the big call does (test_gpu_recursive_iir.py compares that form with the whole-wave one)."""
    from grafx_amd import ops

    R, L = R_BIG, 64
    g = _gen("biquad_cascade", K, C, Cf)
    x = _signal(g, R, C, L)
    rad, th = 0.5 + 0.4 * torch.rand(R, Cf, K, generator=g), 3.0 * torch.rand(R, Cf, K, generator=g)
    As = torch.stack([torch.ones_like(rad), -2 * rad * torch.cos(th), rad * rad], -1)
    Bs = torch.stack([torch.ones_like(rad), -1.6 * torch.cos(th), 0.64 * torch.ones_like(rad)], -1)
    Cout, n = max(C, Cf), _inner(R)
    y = ops.biquad_cascade(_view(x.cuda(), n), Bs.cuda(), As.cuda(), out=_view(_nan(R, Cout, L), n)).reshape(R, Cout, L)
    _finite(y, "biquad_cascade")
    ref = x.double().expand(R, Cout, L)
    for k in range(K):   # plain direct-form recursion in float64
        b, a = Bs[:, :, k].double().expand(R, Cout, 3), As[:, :, k].double().expand(R, Cout, 3)
        out = torch.zeros_like(ref)
        w1 = torch.zeros(R, Cout, dtype=torch.float64)
        w2 = torch.zeros_like(w1)
        for i in range(L):
            w = ref[..., i] - a[..., 1] * w1 - a[..., 2] * w2
            out[..., i] = b[..., 0] * w + b[..., 1] * w1 + b[..., 2] * w2
            w2, w1 = w1, w
        ref = out
    # test_gpu_recursive_iir.py::test_recursive_cascade_matches_float64_direct_form_across_tile_boundaries
    assert_close_rows(y.cpu(), ref, 2e-5, f"biquad_cascade K={K}")
    xc, Bc, Ac = x.cuda(), Bs.cuda(), As.cuda()
    for sl in (slice(0, 16384), slice(65535 - 8192, 65535 + 8192), slice(R - 16384, R)):   # (even starts: the same pairs)
        sl = slice(sl.start - sl.start % 2, sl.stop)
        assert torch.equal(y[sl], ops.biquad_cascade(xc[sl], Bc[sl], Ac[sl])), f"biquad_cascade rows {sl.start}..{sl.stop}"


@pytest.mark.parametrize("n", [8, 65])
def test_irdft(n):
    from grafx_amd import ops

    R, K = R_BIG, n // 2 + 1
    g = _gen("irdft", n)
    Xc = torch.complex(torch.randn(R, K, generator=g), torch.randn(R, K, generator=g)) * _scale(R)[:, None]
    Xr = torch.randn(R, K, generator=g).abs() * _scale(R)[:, None]
    for X in (Xc, Xr):
        got = ops.irdft(X.cuda(), n)
        want = torch.fft.irfft(X.to(torch.complex128), n=n)
        # test_gpu_next_rows2.py::test_small_inverse_real_dft_matches_torch_irfft
        assert_close_rows(got.cpu(), want, 2e-6, f"irdft n={n}")
        Xd = X.cuda()
        _same_bits(got, lambda s: ops.irdft(Xd[s], n), R, "irdft")


@pytest.mark.parametrize("C", [1, 2])
def test_onepole_and_onepole_energy(C):
    from grafx_amd import ops

    R, L, N = R_BIG, 64, 33
    g = _gen("onepole", C)
    x, z = _signal(g, R, C, L), torch.randn(R, generator=g)
    u = x.square().mean(1)
    want = torch.relu(linear_convolve(x.double().square().mean(1), oracle.one_pole_fir(z.double()[:, None], N)))
    got = ops.onepole(u.cuda(), z.cuda(), N)
    # tolerance: tested through the compressor's "iir" smoother only -> the north star
    assert_close_rows(got.cpu(), want, NORTH_STAR_TOL, "onepole")
    rm = {}
    got_e = ops.onepole_energy(_view(x.cuda(), _inner(R)), z.cuda(), N, rowmax=rm)
    assert_close_rows(got_e.cpu(), want, NORTH_STAR_TOL, "onepole_energy")
    assert rm["words"].shape == (R,)
    uc, xc, zc = u.cuda(), x.cuda(), z.cuda()
    _same_bits(got, lambda s: ops.onepole(uc[s], zc[s], N), R, "onepole")
    _same_bits(got_e, lambda s: ops.onepole_energy(xc[s], zc[s], N), R, "onepole_energy")


@pytest.mark.parametrize("shelving", [True, False])
def test_peq_coeffs_and_iir_fsm_fir(shelving):
    from grafx_amd import ops

    R, K, N = R_BIG, 3, 65
    g = _gen("peq", shelving)
    w0, qi, lg = (0.5 * torch.randn(R, 1, K, generator=g) for _ in range(3))
    Bs, As = ops.peq_coeffs(w0.cuda(), qi.cuda(), lg.cuda(), use_shelving=shelving)
    B64, A64 = oracle.peq_biquad_coefficients(w0.double(), qi.double(), lg.double(), shelving)
    # tolerance: tested through ParametricEqualizer only -> the north star
    assert_close_rows(Bs.cpu().reshape(-1, 3), B64.reshape(-1, 3), NORTH_STAR_TOL, "peq_coeffs Bs")
    assert_close_rows(As.cpu().reshape(-1, 3), A64.reshape(-1, 3), NORTH_STAR_TOL, "peq_coeffs As")
    c = [t.cuda() for t in (w0, qi, lg)]
    _same_bits(Bs, lambda s: ops.peq_coeffs(*(t[s] for t in c), use_shelving=shelving)[0], R, "peq_coeffs Bs")
    _same_bits(As, lambda s: ops.peq_coeffs(*(t[s] for t in c), use_shelving=shelving)[1], R, "peq_coeffs As")
    plan = ops.iir_fsm_plan(N, Bs.device)
    h = ops.iir_fsm_fir(Bs, As, N, plan)
    # taps of the float32 coefficients the kernel was given, in float64; tolerance: ParametricEqualizer only -> north star
    want = oracle.iir_fsm_fir(Bs.cpu().double(), As.cpu().double(), N).reshape(R, N)
    assert_close_rows(h.cpu(), want, NORTH_STAR_TOL, "iir_fsm_fir N=65")
    _same_bits(h, lambda s: ops.iir_fsm_fir(Bs[s], As[s], N, plan), R, "iir_fsm_fir")
    h64 = ops.iir_fsm_fir(Bs.double(), As.double(), N, plan)
    assert_close_rows(h64.cpu(), want, NORTH_STAR_TOL, "iir_fsm_fir (float64 coefficients) N=65")


@pytest.mark.parametrize("normalized", [False, True])
def test_biquad_coeffs(normalized):
    from grafx_amd import ops

    R, K = R_BIG, 2
    g = _gen("biquad_coeffs", normalized)
    Bin, a1, a2 = torch.randn(R, K, 3, generator=g), torch.randn(R, K, generator=g), torch.randn(R, K, generator=g)
    A0 = torch.rand(R, K, generator=g) + 0.5 if normalized else None
    Bs, As = ops.biquad_coeffs(Bin.cuda(), a1.cuda(), a2.cuda(), None if A0 is None else A0.cuda())
    B64, A64 = oracle.biquad_coefficients(Bin.double(), a1.double(), a2.double(), None if A0 is None else A0.double())
    # tolerance: tested through BiquadFilter only -> the north star
    assert_close_rows(Bs.cpu().reshape(-1, 3), B64.reshape(-1, 3), NORTH_STAR_TOL, "biquad_coeffs Bs")
    assert_close_rows(As.cpu().reshape(-1, 3), A64.reshape(-1, 3), NORTH_STAR_TOL, "biquad_coeffs As")
    c = [t.cuda() for t in (Bin, a1, a2)] + [None if A0 is None else A0.cuda()]
    for k, big in enumerate((Bs, As)):
        _same_bits(big, lambda s: ops.biquad_coeffs(*(None if t is None else t[s] for t in c))[k], R, "biquad_coeffs")


@pytest.mark.parametrize("schedule", ["oneshot", "rows"])
@pytest.mark.parametrize("smoother,C,L,param_rows", [(0, 2, 64, None), (0, 2, 64, 5), (1, 2, 64, None), (1, 2, 64, 5),
                                                     (1, 1, 1024, None)])
def test_dynamics_fused(smoother, C, L, schedule, param_rows):
    """The compressor in one launch (rows on grid.x: R * nchunks workgroups, or the one-shot tile grid) against the
    oracle's Compressor in float64 (iir_len = 33: L + iir_len - 1 is even, the reference's convolution is then the linear
    one).  Check B with the schedule pinned, for per-row parameters (shared ones would need slices on multiples of 5)."""
    from grafx_amd import ops

    R, N = R_BIG, 33
    g = _gen("dynamics_fused", smoother, C, L, param_rows)
    x = _signal(g, R, C, L)
    P = R if param_rows is None else param_rows
    lt, lr, lk = _dyn_params(g, P)
    z = torch.randn(P, generator=g)
    n = _inner(R)
    u1 = _nan(R, L) if smoother == 1 else None
    y = ops.dynamics_fused(_view(x.cuda(), n), lt.cuda(), lr.cuda(), lk.cuda(), z.cuda(), smoother, N, "quadratic", False,
                           out=_view(_nan(R, C, L), n), param_rows=param_rows, schedule=schedule, u1_out=u1).reshape(R, C, L)
    _finite(y, "dynamics_fused")
    if u1 is not None:
        _finite(u1, "dynamics_fused u1_out")
    m = oracle.OracleCompressor(energy_smoother="iir" if smoother else None, knee="quadratic", iir_len=N)
    idx = torch.arange(R) % P
    col = lambda t: t[idx].double()[:, None]  # noqa: E731
    want = m(x.double(), col(lt), col(lr), col(lk), col(z) if smoother else None)
    # tolerance: test_gpu_edge_cases.py::test_compressor_ragged_lengths holds the processor to the north star
    assert_close_rows(y.cpu(), want, NORTH_STAR_TOL, f"dynamics_fused smoother={smoother} L={L} {schedule}")
    if param_rows is None:
        xc, pc = x.cuda(), [t.cuda() for t in (lt, lr, lk, z)]
        _same_bits(y, lambda s: ops.dynamics_fused(xc[s], *(t[s] for t in pc), smoother, N, "quadratic", False, schedule=schedule),
                   R, f"dynamics_fused {schedule}")


# ------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize("J", [1, 3])
def test_gather_sum_and_fanout(J):
    """A batch above 65 535 (it rides on grid.z): slices of the batch, not a refusal."""
    from grafx_amd import ops

    B, V, C, L = R_BIG, 4, 2, 64
    buf = torch.randn(B, V, C, L, generator=_gen("gather_sum", J)) * _scale(B)[:, None, None, None]
    dests = [[0, 1], [2], [0, 2, 3]][:J] if J == 3 else [[1, 3]]
    src = torch.tensor([s for d in dests for s in d])
    seg = torch.tensor([0] + [sum(len(d) for d in dests[: j + 1]) for j in range(J)])
    want = torch.stack([sum(buf[:, s].double() for s in d) for d in dests], 1)
    bc = buf.cuda()
    out = ops.gather_sum(bc, src.cuda(), seg.cuda(), _nan(B, J, C, L))
    _finite(out, "gather_sum")
    # tolerance: tested through render_grafx only -> the north star
    assert_close_rows(out.cpu(), want, NORTH_STAR_TOL, f"gather_sum J={J}")
    _same_bits(out, lambda s: ops.gather_sum(bc[s], src.cuda(), seg.cuda(), _nan(s.stop - s.start, J, C, L)), B, "gather_sum")
    uniq = sorted({s for d in dests for s in d})
    mask = torch.tensor([sum(1 << j for j, d in enumerate(dests) if s in d) for s in uniq])
    fan = _nan(B, J, C, L)
    assert ops.gather_sum_fanout(bc, torch.tensor(uniq).cuda(), mask.cuda(), fan), "gather_sum_fanout refused the call"
    assert torch.equal(fan, out), "gather_sum_fanout differs from gather_sum"


def test_gather_sum_names_its_limit():
    from grafx_amd import ops

    buf, out = torch.zeros(1, 1, 1, 4, device="cuda"), torch.zeros(1, 65536, 1, 4, device="cuda")
    with pytest.raises(ValueError, match="65535"):
        ops.gather_sum(buf, torch.zeros(65536, dtype=torch.int64, device="cuda"),
                       torch.arange(65537, device="cuda"), out)


# ------------------------------------------------------------------------------------- training path, rows on grid.x
def test_fir_grad_and_reversed_spectra():
    from grafx_amd import ops

    R, Cx, Cg, L, N, off = R_BIG, 2, 1, 64, 5, 0
    g = _gen("fir_grad")
    x, gy = _signal(g, R, Cx, L), torch.randn(R, Cg, L, generator=g)
    n = _inner(R)
    gh = ops.fir_grad(_view(x.cuda(), n), _view(gy.cuda(), n), N, off)
    P = 2 * L + N     # gh[k] = sum_m x[m] g[m - off + k] as a float64 FFT correlation (test_gpu_fftconv.py's reference)
    c = torch.fft.irfft(torch.fft.rfft(gy.double(), n=P) * torch.fft.rfft(x.double(), n=P).conj(), n=P)
    want = c[..., (torch.arange(N) - off) % P]
    # test_gpu_fftconv.py::test_filter_gradient_correlation_matches_float64
    assert_close_rows(gh.cpu(), want, 2e-5, "fir_grad")
    xc, gc = x.cuda(), gy.cuda()
    _same_bits(gh, lambda s: ops.fir_grad(xc[s], gc[s], N, off), R, "fir_grad")

    def slots(t, rows):  # (filters, 17 slots, 256 threads, 4 floats); slot 16 is written by thread 0 only
        return t.view(torch.float32).view(rows, -1, 17, 256, 4)

    # test_gpu_fftconv.py::test_reversed_spectra_equal_the_spectra_of_the_flipped_copy: the same bits
    rev, flipped = ops.fir_spectrum_reversed(_view(xc, n)), ops.fir_spectrum(xc.flip(-1).reshape(R * Cx, L))
    a, b = slots(rev, R * Cx), slots(flipped, R * Cx)
    assert torch.equal(a[:, :, :16], b[:, :, :16]) and torch.equal(a[:, :, 16, 0], b[:, :, 16, 0]), "fir_spectrum_reversed"
    for s in _slices(R):
        part = slots(ops.fir_spectrum_reversed(xc[s]), (s.stop - s.start) * Cx)
        big = a[s.start * Cx : s.stop * Cx]
        assert torch.equal(big[:, :, :16], part[:, :, :16]) and torch.equal(big[:, :, 16, 0], part[:, :, 16, 0])


@pytest.mark.parametrize("shelving", [True, False])
def test_peq_coeffs_bwd(shelving):
    """Against float64 autograd of the oracle's formulas.  A row of the comparison is everything row r produces: the
    gradients of its K biquads with respect to all three parameters (each is a short signed sum of products with the
    incoming gradients; one of them alone may cancel to any degree, whatever evaluates it in float32)."""
    from grafx_amd import ops

    R, K = R_BIG, 3
    g = _gen("peq_bwd", shelving)
    w0, qi, lg = (0.5 * torch.randn(R, 1, K, generator=g) for _ in range(3))
    gB, gA = torch.randn(R, 1, K, 3, generator=g), torch.randn(R, 1, K, 3, generator=g)
    got = ops.peq_coeffs_bwd(w0.cuda(), qi.cuda(), lg.cuda(), gB.cuda(), gA.cuda(), use_shelving=shelving)
    p64 = [t.double().requires_grad_(True) for t in (w0, qi, lg)]
    B64, A64 = oracle.peq_biquad_coefficients(*p64, shelving)
    want = torch.autograd.grad((B64 * gB.double()).sum() + (A64 * gA.double()).sum(), p64)
    # tolerance: tested through ParametricEqualizer's training step only -> the north star
    assert_close_rows(torch.cat([a.cpu().reshape(R, K) for a in got], 1), torch.cat([b.reshape(R, K) for b in want], 1),
                      NORTH_STAR_TOL, "peq_coeffs_bwd")
    c = [t.cuda() for t in (w0, qi, lg, gB, gA)]
    for k, big in enumerate(got):
        _same_bits(big, lambda s: ops.peq_coeffs_bwd(*(t[s] for t in c), use_shelving=shelving)[k], R, "peq_coeffs_bwd")


def test_iir_fsm_bwd():
    from grafx_amd import autograd as diff
    from grafx_amd import ops

    R, K, N = R_BIG, 2, 65
    g = _gen("iir_fsm_bwd")
    # the coefficients of test_gpu_autograd.py::test_fsm_taps_backward_matches_torch_autograd
    Bs = torch.randn(R, 1, K, 3, generator=g) * 0.2 + torch.tensor([1.0, 0, 0])
    As = torch.tensor([1.0, -1.2, 0.5]).expand(R, 1, K, 3) + 0.05 * torch.randn(R, 1, K, 3, generator=g)
    w = torch.randn(R, 1, N, generator=g) * _scale(R)[:, None, None]
    G = ops.rdft(w.cuda())
    gB, gA = ops.iir_fsm_bwd(Bs.cuda(), As.cuda(), G, diff._fsm_delays(N, G.device), N)
    B64, A64 = Bs.double().requires_grad_(True), As.double().requires_grad_(True)
    # G and the delay table are inputs of the entry: the reference evaluates oracle.lti.iir_fsm's formulas in float64 on
    # the values they hold (their float32 rounding is not the kernel's error)
    w64 = torch.fft.irfft(G.cpu().to(torch.complex128), n=N)
    D64 = diff._fsm_delays(N, G.device).cpu().to(torch.complex128)
    resp = ((B64.unsqueeze(-1) * D64).sum(-2) / (A64.unsqueeze(-1) * D64).sum(-2)).prod(-2)
    want = torch.autograd.grad((torch.fft.irfft(resp, dim=-1, n=N) * w64).sum(), (B64, A64))
    for a, b, name in zip((gB, gA), want, ("Bs", "As")):   # GRAD_TOL["fsm taps"] of test_gpu_autograd.py
        assert_close_rows(a.cpu().reshape(R, -1), b.reshape(R, -1), 1e-5, f"iir_fsm_bwd {name}")
    Bc, Ac, D = Bs.cuda(), As.cuda(), diff._fsm_delays(N, G.device)
    for k, big in enumerate((gB, gA)):
        _same_bits(big, lambda s: ops.iir_fsm_bwd(Bc[s], Ac[s], G[s], D, N)[k], R, "iir_fsm_bwd")


def test_iir_fsm_fir_native_length():
    """8200 filters of 8192 taps (65 601 of them would be 2.1 GB of taps): the power-of-two kernel, both coefficient types."""
    from grafx_amd import ops

    R, K, N = 8200, 2, 8192
    g = _gen("iir_fsm_native")
    Bs = torch.randn(R, 1, K, 3, generator=g) * 0.2 + torch.tensor([1.0, 0, 0])
    As = torch.tensor([1.0, -1.2, 0.5]).expand(R, 1, K, 3) + 0.05 * torch.randn(R, 1, K, 3, generator=g)
    plan = ops.iir_fsm_plan(N, torch.device("cuda"))
    want = oracle.iir_fsm_fir(Bs.double(), As.double(), N).reshape(R, N)
    # tolerance: test_gpu_next_rows2.py holds IIRFilter at these lengths to 1e-5
    assert_close_rows(ops.iir_fsm_fir(Bs.cuda(), As.cuda(), N, plan).cpu(), want, 1e-5, "iir_fsm_fir N=8192")
    assert_close_rows(ops.iir_fsm_fir(Bs.cuda().double(), As.cuda().double(), N, plan).cpu(), want, 1e-5, "iir_fsm_fir f64c N=8192")


def test_onepole_dz():
    from grafx_amd import ops

    R, L, N = R_BIG, 64, 17
    g = _gen("onepole_dz")
    gr, U, D = (torch.rand(R, L, generator=g) * _scale(R)[:, None] for _ in range(3))     # positive: sums of one sign
    coef = torch.rand(R, 4, generator=g) + 0.1
    da = ops.onepole_dz(gr.cuda(), U.cuda(), D.cuda(), coef.cuda(), N)
    g64, U64, D64, c64 = gr.double(), U.double(), D.double(), coef.double()
    sh = lambda t: torch.cat([torch.zeros(R, N, dtype=torch.float64), t[:, :-N]], 1)  # noqa: E731   t[n - N]
    u = c64[:, 0:1] * U64 + c64[:, 2:3] * sh(U64)
    d = c64[:, 1:2] * D64 + c64[:, 3:4] * sh(D64)
    want = (g64 * u).sum(1) + (g64[:, 1:] * d[:, :-1]).sum(1)
    # tolerance: tested through the stand-alone smoother's training step only -> the north star
    assert_close_rows(da.cpu().view(-1, 1), want.view(-1, 1), NORTH_STAR_TOL, "onepole_dz")
    c = [t.cuda() for t in (gr, U, D, coef)]
    _same_bits(da, lambda s: ops.onepole_dz(*(t[s] for t in c), N), R, "onepole_dz")


@pytest.mark.parametrize("path", ["kept scan", "rescan", "plain"])
def test_dynamics_bwd(path):
    """gx against float64 autograd of the oracle's compressor (exponential knee: smooth, so that no sample sits on a kink;
    gy has the sign of x, so that the parameter gradients of a row are sums of one sign); the pole gradient, whose terms
    change sign along a row, is compared between the paths by the test of the kept scan (2e-5 of the row, as
    test_gpu_autograd.py::test_compressor_backward_with_and_without_the_kept_scan_agree) and held to check B here."""
    from grafx_amd import ops

    R, C, L, N, knee = R_BIG, 2, 64, 33, "exponential"
    g = _gen("dynamics_bwd")
    x = _signal(g, R, C, L)
    gy = torch.randn(R, C, L, generator=g).abs() * torch.sign(x)
    lt, lr, lk = _dyn_params(g, R)
    z = torch.randn(R, generator=g)
    c = [t.cuda() for t in (x, gy, lt, lr, lk, z)]

    def run(t, s=slice(None)):
        t = [v[s] for v in t]
        if path == "kept scan":
            u1 = _nan(t[0].shape[0], L)
            ops.dynamics_fused(t[0], *t[2:], 1, N, knee, False, u1_out=u1, schedule="rows")
            return ops.dynamics_bwd(*t, N, knee, False, u1=u1, schedule="rows")
        return ops.dynamics_bwd(*t, N, knee, False, rescan=path == "rescan")

    gx, gp, da = run(c)
    for t in (gx, gp, da):
        _finite(t, f"dynamics_bwd {path}")
    x64 = x.double().requires_grad_(True)
    p64 = [t.double()[:, None].requires_grad_(True) for t in (lt, lr, lk)]
    m = oracle.OracleCompressor(energy_smoother="iir", knee=knee, iir_len=N)
    y = m(x64, *p64, z.double()[:, None])
    want = torch.autograd.grad((y * gy.double()).sum(), [x64] + p64)
    # tolerance: 1e-5, the GRAD_TOL entries of test_gpu_autograd.py
    assert_close_rows(gx.cpu(), want[0], 1e-5, f"dynamics_bwd gx {path}")
    assert_close_rows(gp.cpu(), torch.cat(want[1:], 1), 1e-5, f"dynamics_bwd gparams {path}")
    plain = ops.dynamics_bwd(*c, N, knee, False, rescan=False)[2]
    assert_close_rows(da.cpu().view(-1, 1), plain.cpu().view(-1, 1), 2e-5, f"dynamics_bwd dalpha {path} vs plain")
    if path != "rescan":    # (the rescan tiles add ordered partial sums per tile grid: pinned rows only for the others)
        for k, big in enumerate((gx, gp, da)):
            _same_bits(big, lambda s: run(c, s)[k], R, f"dynamics_bwd {path}")


@pytest.mark.parametrize("schedule", ["chunks", "rows"])
def test_ballistics_family(schedule):
    """The float32 sequential recursion bit for bit (oracle.ballistics_coefficients, as test_gpu_ballistics.py), from the rows,
    from a signal's energy, and inside the one-pass compressor (gain curve in float64 on that envelope)."""
    from grafx_amd import ops

    R, C, L = R_BIG, 2, 64
    g = _gen("ballistics", schedule)
    x = _signal(g, R, C, L)
    coef = torch.rand(R, 2, generator=g) * 0.96 + 0.02
    e = x.square().mean(-2)
    ref = oracle.ballistics_coefficients(e, coef[:, 0], coef[:, 1])
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    y = ops.ballistics(e.cuda(), coef.cuda(), coefficients=True, schedule=schedule)
    assert torch.equal(bits(y.cpu()), bits(ref)), "ballistics"
    n = _inner(R)
    ye = ops.ballistics_energy(_view(x.cuda(), n), coef.cuda(), coefficients=True, schedule=schedule)
    assert torch.equal(bits(ye.cpu()), bits(ref)), "ballistics_energy"
    za = torch.logit(coef.double()).float()                      # the compressor entry takes logits
    env = oracle.ballistics_coefficients(e, *torch.sigmoid(za).unbind(1))
    lt, lr, lk = _dyn_params(g, R)
    out = ops.dynamics_ballistics(_view(x.cuda(), n), lt.cuda(), lr.cuda(), lk.cuda(), za.cuda(), "exponential", False,
                                  out=_view(_nan(R, C, L), n), schedule=schedule).reshape(R, C, L)
    _finite(out, "dynamics_ballistics")
    gain = _log_gain64(torch.log(env.double() + 1e-5), lt, lr, lk, "exponential", False).exp()
    # tolerance: test_gpu_ballistics.py::test_compressor_with_the_ballistics_smoother_matches_the_oracle (1e-5)
    assert_close_rows(out.cpu(), gain[:, None, :] * x.double(), 1e-5, f"dynamics_ballistics {schedule}")
    ec, cc = e.cuda(), coef.cuda()
    _same_bits(y, lambda s: ops.ballistics(ec[s], cc[s], coefficients=True, schedule=schedule), R, "ballistics")


@pytest.mark.parametrize("schedule", ["chunks", "rows"])
def test_ballistics_bwd(schedule):
    """Against the float64 adjoint recursion of test_gpu_ballistics.py, every row (numpy, vectorised over rows)."""
    import numpy as np

    from grafx_amd import ops

    R, L = R_BIG, 64
    g = _gen("ballistics_bwd", schedule)
    x = torch.rand(R, L, generator=g) * 2
    z = torch.randn(R, 2, generator=g)
    gr = torch.rand(R, L, generator=g) * _scale(R)[:, None]
    y = ops.ballistics(x.cuda(), z.cuda(), schedule="rows")
    gx, gz = ops.ballistics_bwd(x.cuda(), y, gr.cuda(), z.cuda(), schedule=schedule)
    xs, ys, gs = x.double().numpy(), y.double().cpu().numpy(), gr.double().numpy()
    at, rt = torch.sigmoid(z.double()).numpy().T
    lam, carry, sa, sr = np.zeros((R, L)), np.zeros(R), np.zeros(R), np.zeros(R)
    for i in range(L - 1, -1, -1):
        yp = ys[:, i - 1] if i > 0 else np.ones(R)
        attack = xs[:, i] < yp
        c = np.where(attack, at, rt)
        l_ = gs[:, i] + carry
        lam[:, i] = c * l_
        d = l_ * (xs[:, i] - yp)
        sa, sr = sa + np.where(attack, d, 0.0), sr + np.where(attack, 0.0, d)
        carry = (1.0 - c) * l_
    # GRAD_TOL["ballistics gx"] / ["ballistics gz"] of test_gpu_autograd.py (1e-5)
    assert_close_rows(gx.cpu(), torch.from_numpy(lam), 1e-5, f"ballistics_bwd gx {schedule}")
    want = torch.from_numpy(np.stack([sa * at * (1 - at), sr * rt * (1 - rt)], 1))
    assert_close_rows(gz.cpu(), want, 1e-5, f"ballistics_bwd gz {schedule}")
    c = [x.cuda(), y, gr.cuda(), z.cuda()]
    if schedule == "rows":
        for k, big in enumerate((gx, gz)):
            _same_bits(big, lambda s: ops.ballistics_bwd(*(t[s] for t in c), schedule=schedule)[k], R, "ballistics_bwd")


# ------------------------------------------------------------------------------------- aliasing: the other forms
@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("rows_per_chunk", [None, 70000])
def test_odd_alias_precise(pairs, rows_per_chunk, monkeypatch, small_alias_workspace):
    from grafx_amd import ops

    monkeypatch.setattr(ops, "ALIAS_PAIRS", pairs)
    rows, P = R_BIG, 101
    z = torch.randn(rows, P, generator=_gen("odd_alias_precise", pairs)) * _scale(rows)[:, None]
    got = ops.odd_alias(z.cuda(), rows_per_chunk=rows_per_chunk, precise=True)
    want = torch.fft.irfft(torch.fft.rfft(z.double()))
    # test_gpu_odd_alias.py::test_precise_odd_alias_is_float64_accurate: 1.5e-7 of the sample + 1e-12 of the peak, per row here
    tol = 1.5e-7 * want.abs() + 1e-12 * want.abs().amax(-1, keepdim=True)
    assert ((got.double().cpu() - want).abs() <= tol).all(), "odd_alias precise"
    adj = ops.odd_alias_adjoint(z[:, : P - 1].cuda(), P, rows_per_chunk=rows_per_chunk or 1024, precise=True)
    zd = torch.zeros(rows, P, dtype=torch.float64, requires_grad=True)
    torch.fft.irfft(torch.fft.rfft(zd)).backward(z[:, : P - 1].double())
    assert_close_rows(adj.cpu(), zd.grad, 2e-7, "odd_alias_adjoint precise")     # the same test's adjoint bound


@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("P,R,C,rows_per_chunk", [(101, R_BIG, 1, None), (101, 21867, 3, 70000), (4001, 16403, 1, 70000),
                                                  (4001, 5467, 3, None)])
def test_odd_alias_rows_form(P, R, C, rows_per_chunk, pairs, monkeypatch, small_alias_workspace):
    """out=: the rows land in a strided (B, n, C, length) view (ymap of gfx_odd_alias_f32 / gfx_odd_alias_pair_f32 with row0 and the
    row map); 65 601 and 16 403 rows (an odd count past the one-row entry's 16 383), a slice of the result."""
    from grafx_amd import ops

    monkeypatch.setattr(ops, "ALIAS_PAIRS", pairs)
    n = _inner(R)
    lo, length = 3, P - 1 - 7
    z = torch.randn(R * C, P, generator=_gen("odd_alias_rows", P, R, C)) * _scale(R * C)[:, None]
    view = _view(_nan(R, C, length), n)
    got = ops.odd_alias(z.cuda(), lo, length, out=view, rows_per_chunk=rows_per_chunk)
    assert got is view
    _finite(view, "odd_alias out=")
    want = torch.fft.irfft(torch.fft.rfft(z.double()))[:, lo : lo + length]
    # tolerance: test_gpu_odd_alias.py::test_odd_alias_matches_float64_fft (3e-6)
    assert_close_rows(view.reshape(R * C, length).cpu(), want, 3e-6, f"odd_alias out= P={P}")
    # test_gpu_odd_alias.py::test_odd_alias_writes_strided_buffer_rows_in_place: the same values as the contiguous result
    assert torch.equal(view.reshape(R * C, length), ops.odd_alias(z.cuda(), lo, length, rows_per_chunk=rows_per_chunk))


# ------------------------------------------------------------------------------------- long rows, pipe, row maxima
@pytest.mark.parametrize("schedule", ["tile", "pipe", "auto"])
def test_fftconv_long_rows(schedule):
    """L = 1024 (65 601 x 1024: 0.27 GB in, 0.27 GB out), every schedule pinned; "auto" with rowmax=: where the kernel that
    ran leaves the rows' maxima, they are the bits of max |y| of each row."""
    from grafx_amd import ops

    R, L, N = R_BIG, 1024, 5
    g = _gen("fftconv_long")
    x = _signal(g, R, 1, L)
    h = torch.randn(R, 1, N, generator=g) * _scale(R)[:, None, None]
    Hs = ops.fir_spectrum(h.cuda().reshape(R, N))
    rm = {}
    y = ops.fftconv(x.cuda(), Hs, N, 1, out=_nan(R, 1, L), schedule=schedule, rowmax=rm if schedule == "auto" else None)
    _finite(y, "fftconv")
    assert_close_rows(y.cpu(), _fir64(x, h, R, L), 1e-5, f"fftconv L=1024 {schedule}")   # test_gpu_fftconv.py (1e-5)
    if "words" in rm:
        assert torch.equal(rm["words"].view(torch.float32), y.abs().amax(-1).reshape(-1)), "fftconv rowmax"
    if schedule != "auto":
        xc, hc = x.cuda(), h.cuda()
        _same_bits(y, lambda s: ops.fftconv(xc[s], ops.fir_spectrum(hc[s].reshape(-1, N)), N, 1, schedule=schedule), R,
                   f"fftconv {schedule}")


# ------------------------------------------------------------------------------------- fused routing sums, a whole render
def _render_graph():
    from grafx_amd.data import GRAFX, NodeConfigs

    G = GRAFX(config=NodeConfigs(["gain", "biquad"]))
    out_id, mix = G.add("out"), G.add("mix")
    for _ in range(2):
        _, last = G.add_serial_chain(["in", "gain", "biquad"])
        G.connect(last, mix)
    G.connect(mix, out_id)
    return G


def test_render_at_batch_65601():
    """in -> StereoGain -> BiquadFilter(fsm_fir_len = 65) -> two-source mix -> out at batch 65 601, L = 256, against the oracle
    render in float64 (as test_gpu_render.py at small batch): every stage of the render above the grid limit, the routing
    sums included (the gain stage's fused sum covers 65 535 graphs: the plain stage and gather_sum take over)."""
    from grafx_amd.data import convert_to_tensor
    from grafx_amd.processors import BiquadFilter, StereoGain
    from grafx_amd.render import prepare_render, render_grafx, reorder_for_fast_render
    from grafx_amd.utils import create_empty_parameters

    B, L = R_BIG, 256
    G = _render_graph()
    hip = {"gain": StereoGain().cuda(), "biquad": BiquadFilter(num_filters=1, flashfftconv=False, fsm_fir_len=65).cuda()}
    cpu = {"gain": oracle.OracleStereoGain(), "biquad": oracle.OracleBiquadFilter(num_filters=1, fsm_fir_len=65)}
    rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam"))
    torch.manual_seed(0)
    params = create_empty_parameters(hip, G, std=0.3)
    x = torch.randn(B, 2, 2, L, generator=_gen("render")) * _scale(B)[:, None, None, None]
    with torch.no_grad():
        want, _, _ = render_grafx(cpu, x.double(), {t: {k: v.detach().double() for k, v in d.items()} for t, d in params.items()}, rd)
        got, _, _ = render_grafx(hip, x.cuda(), {t: {k: v.detach().cuda() for k, v in d.items()} for t, d in params.items()},
                                 rd.to("cuda"))
    _finite(got, "render")
    assert_close_rows(got.cpu(), want, 1e-5, "render at batch 65601")      # test_gpu_render.py::test_cfg1_plumbing_graph


def test_fused_routing_sums_above_65535_graphs():
    """StereoGain with mix= (gain_mix_kernel) and the compressor with mix= (dyn_oneshot_mix_kernel) at 65 601 graphs of two
    rows summed into one destination: the sums equal gather_sum over the stage's rows whether the fused kernel took the
    call or left it (mix["done"] unset: the caller runs the gather-sum, as render_grafx does)."""
    from grafx_amd import ops

    B, n, C, L = R_BIG, 2, 2, 64
    g = _gen("mix")
    x = _signal(g, B * n, C, L).view(B, n, C, L)
    codes, n_acc, pre, post = ops.mix_schedule([[0, 1]], n)
    assert not pre and not post
    sched = torch.tensor(codes, dtype=torch.int64, device="cuda")
    src, seg = torch.tensor([0, 1], device="cuda"), torch.tensor([0, 2], device="cuda")
    lg = (0.5 * torch.randn(B * n, 2, generator=g)).cuda()
    lt, lr, lk = (t.cuda() for t in _dyn_params(g, B * n))
    z = torch.randn(B * n, generator=g).cuda()
    stages = {"stereo_gain": lambda xin, out, mix: ops.stereo_gain(xin, lg, out=out, mix=mix),
              "dynamics_fused": lambda xin, out, mix: ops.dynamics_fused(xin, lt, lr, lk, z, 1, 33, "quadratic", False, out=out, mix=mix)}
    for name, stage in stages.items():
        plain = stage(x.cuda(), _nan(B, n, C, L), None)
        want = ops.gather_sum(plain, src, seg, _nan(B, 1, C, L))
        mix = {"sched": sched, "n_acc": n_acc, "out": _nan(B, 1, C, L)}
        y = stage(x.cuda(), _nan(B, n, C, L), mix)
        assert torch.equal(y, plain), name
        if mix.get("done"):
            assert torch.equal(mix["out"], want), f"{name}: fused sums differ from gather_sum"
        _finite(want, name)
        ref = plain.double().cpu().sum(1, keepdim=True)
        assert_close_rows(want.cpu(), ref, NORTH_STAR_TOL, f"{name} sums")   # tested through render_grafx only -> north star
