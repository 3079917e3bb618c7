"""The float64 yardstick of the loudness meter (not a test module): its own statement of the BS.1770 K-weighting, the
filter as scipy.signal.lfilter in float64, the sub-block energies and their gradient flip(K(flip(2 c y))), the gating
formula with its gradient by float64 autograd, and the inputs the tests share, drawn from seeded CPU generators.
Everything is computed once per argument set and handed out unchanged."""
import functools
import math

import numpy as np
import torch
from scipy.signal import lfilter

# hop, L, C, sample rate of the coefficients: the smallest shapes at which the kernels can still go wrong (tile: 1024 samples)
SHAPES = (
    (441, 1764, 1, 4410),        # exactly one block; odd hop: boundaries inside a lane's run; partial last tile
    (441, 1763, 1, 4410),        # three sub-blocks (the module refuses it: less than a block)
    (3, 100, 2, 4410),           # many sub-blocks per lane
    (1024, 8192, 2, 44100),      # boundaries on tile edges; the shortest hop whose sums the wave reduces (below: through LDS)
    (800, 16037, 2, 8000),       # 37 trailing samples
    (4800, 144001, 2, 48000),    # the standard's own coefficients, a long memory over many tiles
    (70000, 141000, 1, 48000),   # a sub-block over 69 tiles: more parts than the finishing wave has lanes
)
STRIDED = (4410, 131072, 2, 44100)   # read from a (B, n, C, L) slice
MANY = (130, 520, 1, 4410)           # 66000 row-channels
KINDS = ("noise", "bass", "dc")
ROWS = 2
GATING_RATES = (4410, 8000, 48000)
MARGIN = 0.5                          # LU between every block and either gate


def k_weighting(fs):
    """((b, a) of the shelf, (b, a) of the high-pass), a0 = 1, float64: the bilinear transform of the two analogue
    prototypes behind the table of BS.1770 (at 48 kHz: the table)."""
    def prototype(f0, Q):
        K = math.tan(math.pi * f0 / fs)
        return K, K / Q, 1.0 + K / Q + K * K

    K, KQ, a0 = prototype(1681.974450955533, 0.7071752369554196)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    shelf = (np.array([Vh + Vb * KQ + K * K, 2.0 * (K * K - Vh), Vh - Vb * KQ + K * K]) / a0,
             np.array([a0, 2.0 * (K * K - 1.0), 1.0 - KQ + K * K]) / a0)
    K, KQ, a0 = prototype(38.13547087602444, 0.5003270373238773)
    highpass = (np.array([1.0, -2.0, 1.0]), np.array([a0, 2.0 * (K * K - 1.0), 1.0 - KQ + K * K]) / a0)
    return shelf, highpass


def coef(fs):
    """(2, 5) float64 = (b0, b1, b2, a1, a2) per section: what ops.kweight_energy takes."""
    return torch.tensor([[*b, a[1], a[2]] for b, a in k_weighting(fs)], dtype=torch.float64)


def k_filter(x, fs):
    """The K-weighted signal along the last axis, float64, from silence."""
    y = np.asarray(x, dtype=np.float64)
    for b, a in k_weighting(fs):
        y = lfilter(b, a, y, axis=-1)
    return y


@functools.lru_cache(maxsize=None)
def signal(hop, L, C, fs, kind, rows=ROWS):
    """(rows, C, L) float32 on the CPU, seeded by the shape.  "noise": unit white noise; "bass": 0.5 sin(2 pi 30 n / fs) +
    1e-3 noise; "dc": 0.8 + 1e-3 noise.  Every row-channel has its own noise (and the sine its own phase)."""
    g = torch.Generator().manual_seed(7 * hop + L + 1000 * C + fs + rows)
    noise = torch.randn(rows, C, L, generator=g, dtype=torch.float64)
    if kind == "noise":
        x = noise
    elif kind == "bass":
        phase = torch.rand(rows, C, 1, generator=g, dtype=torch.float64)
        x = 0.5 * torch.sin(2 * math.pi * (30.0 * torch.arange(L, dtype=torch.float64) / fs + phase)) + 1e-3 * noise
    else:
        x = 0.8 + 1e-3 * noise
    return x.float()


def energies_of(x, fs, hop):
    """(..., L) float32 -> (..., L // hop) float64: the sums of squares of the K-weighted signal per sub-block."""
    y = k_filter(x.numpy(), fs)
    n_sub = y.shape[-1] // hop
    return torch.from_numpy(np.square(y[..., :n_sub * hop]).reshape(*y.shape[:-1], n_sub, hop).sum(-1))


def energy_grad_of(x, fs, hop, genergy):
    """The gradient of sum(genergy * energies_of(x)) with respect to x, float64: flip(K(flip(2 c y))), c = genergy held
    over its sub-block and 0 on the trailing samples."""
    y = k_filter(x.numpy(), fs)
    L = y.shape[-1]
    c = np.zeros_like(y)
    n_sub = L // hop
    c[..., :n_sub * hop] = np.repeat(genergy.numpy(), hop, axis=-1)
    return torch.from_numpy(k_filter((2.0 * c * y)[..., ::-1], fs)[..., ::-1].copy())


@functools.lru_cache(maxsize=None)
def energies(hop, L, C, fs, kind, rows=ROWS):
    return energies_of(signal(hop, L, C, fs, kind, rows), fs, hop)


@functools.lru_cache(maxsize=None)
def cotangent(hop, L, C, fs, pattern, rows=ROWS):
    """genergy (rows, C, L // hop) float64.  "ones"; "random": seeded normal doubles; "runs": 0 / 1 with runs of zeros."""
    n_sub = L // hop
    if pattern == "ones":
        return torch.ones(rows, C, n_sub, dtype=torch.float64)
    g = torch.Generator().manual_seed(hop + 3 * L + C)
    if pattern == "random":
        return torch.randn(rows, C, n_sub, generator=g, dtype=torch.float64)
    on = (torch.rand(rows, C, -(-n_sub // 3), generator=g) < 0.5).repeat_interleave(3, -1)[..., :n_sub]
    return on.double()


@functools.lru_cache(maxsize=None)
def energy_grad(hop, L, C, fs, kind, pattern, rows=ROWS):
    return energy_grad_of(signal(hop, L, C, fs, kind, rows), fs, hop, cotangent(hop, L, C, fs, pattern, rows))


# ------------------------------------------------------------------------------------------------------------- gating
def lufs(p):
    return -0.691 + 10.0 * torch.log10(p)


def block_power(mean_squares, block_hops, gains):
    """(C, n_sub) mean squares per sub-block -> (n_blocks,): sum_c G_c z_cj, z the mean over block_hops sub-blocks."""
    z = mean_squares.unfold(-1, block_hops, 1).mean(-1)
    return (torch.as_tensor(gains, dtype=torch.float64)[:, None] * z).sum(0)


def gated(mean_squares, block_hops, gains, absolute=-70.0, relative=-10.0):
    """One item's integrated loudness (a 0-d float64 tensor, differentiable in the energies) and the smallest distance in LU
    of a block from either threshold.  -inf and no margin for an item without a block above the absolute gate."""
    p = block_power(mean_squares, block_hops, gains)
    level = lufs(p.detach())
    first = level > absolute
    if not first.any():
        return torch.tensor(-math.inf, dtype=torch.float64), math.inf
    threshold = float(lufs(p.detach()[first].mean())) + relative
    second = first & (level > threshold)
    finite = level[torch.isfinite(level)]
    margin = float(torch.minimum((finite - absolute).abs(), (finite - threshold).abs()).min())
    return lufs(p[second].mean()), margin


@functools.lru_cache(maxsize=None)
def gating_signal(fs, seed=1):
    """(2, 3 fs + fs + 37) float32: per second 0.1 randn, then 30 dB below it, then 1e-5 randn (under the absolute gate),
    then 0.05 randn for a second and 37 samples."""
    rng = np.random.default_rng(seed)
    parts = [0.1 * rng.standard_normal((2, fs)), 0.1 * 10.0 ** (-30.0 / 20.0) * rng.standard_normal((2, fs)),
             1e-5 * rng.standard_normal((2, fs)), 0.05 * rng.standard_normal((2, fs + 37))]
    return torch.from_numpy(np.concatenate(parts, -1)).float()


@functools.lru_cache(maxsize=None)
def gating_case(fs, seed=1, block_hops=4):
    """For the gating signal at ``fs`` (hop = fs / 10): the sub-block sums (2, n_sub), the integrated loudness, its gradient
    with respect to the sums, the ungated block loudness, and the gradient with respect to the signal -- all float64.  The
    draw must keep every block MARGIN away from both thresholds: a comparison never hinges on a block at a threshold."""
    hop = fs // 10
    x = gating_signal(fs, seed)
    sums = energies_of(x, fs, hop).requires_grad_(True)
    loudness, margin = gated(sums / hop, block_hops, (1.0, 1.0))
    assert margin >= MARGIN, f"gating signal at {fs} Hz, seed {seed}: a block {margin:.3f} LU from a threshold"
    loudness.backward()
    blocks = lufs(block_power(sums.detach() / hop, block_hops, (1.0, 1.0)))
    return {"x": x, "hop": hop, "sums": sums.detach(), "loudness": loudness.detach(), "dsums": sums.grad,
            "blocks": blocks, "dx": energy_grad_of(x, fs, hop, sums.grad)}
