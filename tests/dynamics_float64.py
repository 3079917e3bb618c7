"""Float64 yardstick of the dynamics backward (tests/test_dynamics_float64.py, tests/test_gpu_dynamics_bwd_float64.py): the
forward as the reference writes it (dynamics.py:390-405 compressor, 625-640 gate)

    e   = mean_c x^2
    env = relu(sum_{k < N} h[k] e[n - k]),   h[k] = (1 - a) a^k,   a = min(sigmoid(z), 1 - 1e-5)      (smoothed cases)
    G   = log(env + 1e-5)
    g   = log_gain(G, log_threshold - 6, log_ratio, log_knee)        the oracle's curves on doubles
    y   = exp(g) x

as torch ops in float64 on the CPU with the smoother as an explicit convolution, torch autograd of sum(y w) through it, and
inputs CONSTRUCTED so that no sample sits where a gradient jumps: the hard knees' corner G = T and the relu's env = 0.
Every row's threshold is the midpoint of the widest gap between neighbouring sorted values of its float64 G inside the
30 % .. 70 % quantiles, so a float32 evaluation (G good to about 1e-6) takes the same branch for every sample and both
sides of the knee are populated.  Not a test module."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import oracle

KNEES = ("hard", "quadratic", "exponential")
# the clamp of core/envelope.py:51-54 is written on a float32 tensor: its bound is the float32 nearest to 1 - 1e-5
A_MAX = float(torch.tensor(1 - 1e-5, dtype=torch.float32))
# the poles of a case, one per row: instant | short memory | the longest history a one-shot backward tile takes (OS_HMAX =
# 256 taps at a = 0.897) | just beyond it | a^257 = 0.18, a live truncation term | the clamp
ZS = (-20.0, 0.0, 2.16, 2.18, 5.0, 20.0)
# (L, N): just above one wave tile | one workgroup tile | two workgroup tiles and a ragged float4 | no multiple of four |
# N > L | a truncation term that is dead for all but the slowest rows
SHAPES = ((516, 257), (2048, 257), (4100, 257), (2999, 257), (516, 1023), (4100, 4001))
GAIN_LENGTHS = (516, 2999)      # the unsmoothed entries (dyn_gain_bwd, dyn_dx)
CHANNELS = (1, 2)
# every case of the GPU tests: the screening of tests/test_dynamics_float64.py runs over exactly these
SMOOTHED = tuple((L, N, knee, gate, C) for L, N in SHAPES for knee in KNEES for gate in (False, True) for C in CHANNELS)
UNSMOOTHED = tuple((L, knee, gate, C) for L in GAIN_LENGTHS for knee in KNEES for gate in (False, True) for C in CHANNELS)
MARGIN = 1e-4                  # |G - T| of every sample of a hard-knee row: a hundred times float32's rounding of G
MIN_REGION = 0.05               # every populated region of a curve holds this fraction of the row

# float32 inputs (z is None and N is 0 without the smoother; then `env` is the given float32 envelope of the entries that
# take one), and the float64 log-envelope the thresholds were placed on
Case = namedtuple("Case", "x w log_threshold log_ratio log_knee z N knee gate env")


def pole(z):
    """The clamped pole in float64 from the float32 parameter."""
    return torch.sigmoid(z.double().reshape(-1)).clamp(max=A_MAX)


def fir(a, N):
    """h (R, N) = (1 - a) a^k."""
    k = torch.arange(N, dtype=torch.float64)
    return (1 - a)[:, None] * a[:, None].pow(k)


def smooth(e, a, N):
    """The causal N-tap FIR of the rows of e (R, L) with fir(a, N), written as a convolution; before the relu."""
    R = e.shape[0]
    return F.conv1d(F.pad(e, (N - 1, 0))[None], fir(a, N).flip(-1)[:, None, :], groups=R)[0]


def smooth_by_recursion(e, a, N):
    """The same filter as u[n] = a u[n-1] + (1 - a) e[n] minus a^N u[n-N] (a loop over numpy doubles)."""
    e, a = e.numpy(), a.numpy()
    R, L = e.shape
    u = e * 0
    for n in range(L):
        u[:, n] = (a * u[:, n - 1] if n else 0) + (1 - a) * e[:, n]
    out = u.copy()
    if N < L:
        out[:, N:] -= (a ** N)[:, None] * u[:, :L - N]
    return torch.from_numpy(out)


def _curve(knee, gate):
    return (oracle.OracleNoiseGate if gate else oracle.OracleCompressor)(energy_smoother=None, knee=knee).log_gain


def forward(x, log_threshold, log_ratio, log_knee, knee, gate, a=None, N=0, env=None):
    """-> (y (R, C, L), gain (R, L)) in float64 from float64 tensors: the smoothed form with a pole ``a`` (R), the
    unsmoothed one without, or the curve on a given ``env``."""
    if env is None:
        env = x.square().mean(-2)
        if a is not None:
            env = torch.relu(smooth(env, a, N))
    G = torch.log(env + 1e-5)
    col = lambda t: t.reshape(-1, 1)  # noqa: E731
    gain = _curve(knee, gate)(G, col(log_threshold) - 6, col(log_ratio), col(log_knee)).exp()
    return gain[:, None, :] * x, gain


def _signal(R, C, L, seed):
    """Seeded noise of standard deviation 0.5 under a slow amplitude ramp (0.3 .. 1, rising in even rows and falling in
    odd ones): G spreads over more than two units even behind the slowest smoother, and no row is silent -- and the output
    gradient w = dL/dy: seeded noise with the sign of x, as in tests/test_gpu_many_rows.py, so that sum_c w x > 0 at every sample and the three parameter
    gradients of a row are sums of terms of one sign (each curve's dg/dT, dg/dlog_ratio and dg/dlog_knee keep their sign
    along G).  With a signed w they are what is left of ~L cancelling terms, and a relative error of such a remainder says
    nothing about the kernel: float32 torch autograd of the same expressions is then 1e-4 .. 1e-3 of a row's value away
    from float64, and so is every launch path."""
    gen = torch.Generator().manual_seed(seed)
    ramp = torch.exp(torch.linspace(-1.2, 0.0, L, dtype=torch.float64))
    ramp = torch.stack([ramp if r % 2 == 0 else ramp.flip(0) for r in range(R)])
    x = (0.5 * torch.randn(R, C, L, generator=gen, dtype=torch.float64) * ramp[:, None, :]).float()
    return x, torch.randn(R, C, L, generator=gen, dtype=torch.float32).abs() * torch.sign(x)


def _place(G, knee):
    """Per row of the float64 G (R, L): log_threshold with T = log_threshold - 6 in the widest gap of the sorted values
    between the 30 % and 70 % quantiles, and log_knee so that the knee [T - W, T + W] (quadratic: W = exp(log_knee) / 2;
    exponential: W = 2 / exp(log_knee), where the curve's slope is within 12 % of either arm's) ends no farther out
    than the 10 % / 90 % quantiles -- three populated regions.  float32, as the kernels take them."""
    s = G.sort(-1).values
    L = s.shape[-1]
    lo, hi = int(0.3 * L), int(0.7 * L)
    gaps = s[:, lo + 1:hi + 1] - s[:, lo:hi]
    at = gaps.argmax(-1) + lo
    rows = torch.arange(s.shape[0])
    T = 0.5 * (s[rows, at] + s[rows, at + 1])
    lt = (T + 6).float()
    T = lt.double() - 6                     # the threshold the float32 parameter stands for
    W = torch.minimum(T - s[:, int(0.1 * L)], s[:, int(0.9 * L)] - T)
    lk = (torch.log(2 * W) if knee != "exponential" else torch.log(2 / W)).float()
    return lt.reshape(-1, 1), lk.reshape(-1, 1)


def _ratios(R):
    return torch.linspace(-0.6, 0.9, R, dtype=torch.float32).reshape(-1, 1)     # ratios 1.5 .. 3.5


@functools.lru_cache(maxsize=None)
def _smoothed_signal(L, N, C):
    """(x, w, z, the float64 G) of a smoothed case: shared by its knees and processors, never written."""
    z = torch.tensor(ZS, dtype=torch.float32).reshape(-1, 1)
    x, w = _signal(len(ZS), C, L, seed=1000 * C + L + N)
    with torch.no_grad():
        G = torch.log(torch.relu(smooth(x.double().square().mean(-2), pole(z), N)) + 1e-5)
    return x, w, z, G


@functools.lru_cache(maxsize=None)
def case(L, N, knee, gate, C):
    """The smoothed case of a shape: six rows, one per pole of ZS.  Computed once, never written."""
    x, w, z, G = _smoothed_signal(L, N, C)
    lt, lk = _place(G, knee)
    return Case(x, w, lt, _ratios(len(ZS)), lk, z, N, knee, gate, None)


@functools.lru_cache(maxsize=None)
def gain_case(L, knee, gate, C):
    """The unsmoothed case of a length: six rows of the same kind of signal, and the float32 envelope e = mean_c x^2 that
    ops.dyn_gain_bwd is handed (the curve is evaluated on exactly these values)."""
    R = len(ZS)
    x, w = _signal(R, C, L, seed=2000 * C + L)
    env = x.double().square().mean(-2).float()
    lt, lk = _place(torch.log(env.double() + 1e-5), knee)
    return Case(x, w, lt, _ratios(R), lk, None, 0, knee, gate, env)


def _log_envelope(c):
    with torch.no_grad():
        if c.z is None:
            return torch.log(c.env.double() + 1e-5), c.env.double()
        env = smooth(c.x.double().square().mean(-2), pole(c.z), c.N)      # before the relu: its sign is the margin
        return torch.log(torch.relu(env) + 1e-5), env


def margin(c):
    """-> (the smallest |G - T| of every row, the smallest envelope of every row), float64 (R) each."""
    G, env = _log_envelope(c)
    return (G - (c.log_threshold.double() - 6)).abs().amin(-1), env.amin(-1)


def regions(c):
    """-> (R, 3): the fraction of a row's samples below, inside and above the knee (hard: nothing is inside)."""
    G, _ = _log_envelope(c)
    T = c.log_threshold.double() - 6
    if c.knee == "hard":
        W = torch.zeros_like(T)
    else:
        W = c.log_knee.double().exp() / 2 if c.knee == "quadratic" else 2 / c.log_knee.double().exp()
    below, above = G < T - W, G > T + W
    return torch.stack([m.double().mean(-1) for m in (below, ~below & ~above, above)], -1)


Grads = namedtuple("Grads", "gx gparams dalpha gain denv y")


_GRADS = {}     # id(case) -> (case, its Grads): computed once per case, never written


def _grads(c):
    leaf = lambda t: t.double().clone().requires_grad_(True)  # noqa: E731
    x, lt, lr, lk = leaf(c.x), leaf(c.log_threshold), leaf(c.log_ratio), leaf(c.log_knee)
    a = env = None
    if c.z is not None:
        a = pole(c.z).requires_grad_(True)
    elif c.env is not None:
        env = leaf(c.env)
    y, gain = forward(x, lt, lr, lk, c.knee, c.gate, a, c.N, env)
    wanted = [t for t in (x, lt, lr, lk, a, env) if t is not None]
    got = dict(zip(map(id, wanted), torch.autograd.grad((y * c.w.double()).sum(), wanted, allow_unused=True)))
    g = lambda t: None if t is None else got[id(t)]  # noqa: E731
    zero = torch.zeros_like(lt)
    gp = torch.cat([zero if g(t) is None else g(t) for t in (lt, lr, lk)], -1)     # the hard knees have no log_knee
    return Grads(g(x), gp, g(a), gain.detach(), g(env), y.detach())


def grads(c):
    """Float64 autograd of sum(y w) -> Grads: gx (R, C, L), gparams (R, 3) = d/d(log_threshold, log_ratio, log_knee),
    dalpha (R) = d/d(the clamped pole a), which is what ops.dynamics_bwd returns (None without the smoother), gain (R, L),
    and for a case on a given envelope denv (R, L) = d/d env -- there gx is the gradient with env held fixed."""
    if id(c) not in _GRADS:
        _GRADS[id(c)] = (c, _grads(c))
    return _GRADS[id(c)][1]


def dalpha_by_differences(c):
    """d sum(y w) / da by the five-point central difference in the clamped pole (float64), all rows in one batched call.
    The step is 1e-5 (1 - a) -- the taps are (1 - a) a^k, and the second derivative of the quadratic knee jumps at T +- W: a
    sample that crosses there inside the stencil adds an error in proportion to the step -- and never more than 1e-7,
    because next to a = 0 a sample's envelope is e[n] + a e[n-1] + ..., which varies on the scale (e[n] + 1e-5) / e[n-1],
    down to 4e-5 for the quietest sample behind a loud one.  A stencil
    point at which the relu switches is an error."""
    a = pole(c.z)
    args = [t.double() for t in (c.x, c.log_threshold, c.log_ratio, c.log_knee)]
    w, e = c.w.double(), c.x.double().square().mean(-2)
    step = (1e-5 * (1 - a)).clamp(max=1e-7)

    def f(k):
        if float(smooth(e, a + k * step, c.N).min()) <= 0:
            raise ValueError("the relu switches inside the difference stencil")
        return (forward(*args, c.knee, c.gate, a + k * step, c.N)[0] * w).sum((-2, -1))

    with torch.no_grad():
        return (8 * (f(1) - f(-1)) - (f(2) - f(-2))) / (12 * step)
