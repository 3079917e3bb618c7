"""The float64 yardstick of the STFT loss on a filterbank scale (not a test module): the definition of
include/grafx_amd.h's gfx_stft_band_loss_* and of MultiResolutionSTFTLoss with filterbanks -- torch.stft, a matmul and
autograd in float64 on the CPU -- on the shapes and inputs of stft_loss_float64; a restatement of the mel and A-weighting
formulas in numpy, independent of grafx_amd.losses; and the table of filterbanks the tests share.  Everything is computed
once per argument set and handed out unchanged."""
import functools

import numpy as np
import torch

import stft_loss_float64 as f64

SAMPLE_RATE = 44100
MEL_BANDS = {128: 8, 1024: 64, 2048: 128, 512: 40, 256: 24}       # Slaney mel bands per n_fft (16 are too many at 128)
ANY = ("aweight", "one", "boxes", "identity")                      # filterbanks defined for every n_fft
ANY_SHAPES = (f64.SHAPES[0], f64.SHAPES[1], f64.SHAPES[3])         # one frame per buffer (2048) and sixteen (128)
HTK_SHAPE = f64.SHAPES[4]
# Added to the seed of stft_loss_float64.draw for a (filterbank, n_fft, hop, L) whose draw comes too close to a jump of the
# gradient (the screening of tests/test_stft_band_loss_abi.py); the thresholds do not move.
RESEED = {}


# ------------------------------------------------------------------------------------------------ the formulas, in numpy
def hz_to_mel(f, htk=False):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + 27.0 * np.log(np.maximum(f, 1000.0) / 1000.0) / np.log(6.4))


def mel_to_hz(m, htk=False):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * 6.4 ** ((m - 15.0) / 27.0))


def mel_numpy(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None, htk=False, norm="slaney"):
    """(n_mels, n_fft / 2 + 1) float64, row by row."""
    f_max = sample_rate / 2.0 if f_max is None else f_max
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * sample_rate / n_fft
    pts = mel_to_hz(np.linspace(hz_to_mel(f_min, htk), hz_to_mel(f_max, htk), n_mels + 2), htk)
    W = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        left, centre, right = pts[m], pts[m + 1], pts[m + 2]
        W[m] = np.maximum(0.0, np.minimum((freqs - left) / (centre - left), (right - freqs) / (right - centre)))
        if norm == "slaney":
            W[m] *= 2.0 / (right - left)
    return W


def a_weighting_numpy(sample_rate, n_fft):
    def r_a(f):
        return (12194.0 ** 2 * f ** 4 / ((f ** 2 + 20.6 ** 2) * np.sqrt((f ** 2 + 107.7 ** 2) * (f ** 2 + 737.9 ** 2))
                                         * (f ** 2 + 12194.0 ** 2)))

    return r_a(np.arange(n_fft // 2 + 1, dtype=np.float64) * sample_rate / n_fft) / r_a(1000.0)


# ------------------------------------------------------------------------------------------------ the table
@functools.lru_cache(maxsize=None)
def filterbank(name, n_fft):
    """The float32 (n_bins, n_fft / 2 + 1) filterbank ``name`` of the table for a transform size, on the CPU."""
    bins = n_fft // 2 + 1
    if name == "mel":
        W = mel_numpy(SAMPLE_RATE, n_fft, MEL_BANDS[n_fft])
    elif name == "htk":
        W = mel_numpy(SAMPLE_RATE, n_fft, 40, htk=True, norm=None)
    elif name == "aweight":                                  # the diagonal without DC: rows of width 1, one uncovered bin
        W = np.diag(a_weighting_numpy(SAMPLE_RATE, n_fft))[1:]
    elif name == "one":                                      # the widest row
        W = np.ones((1, bins))
    elif name == "boxes":                                    # width 9 at stride 2: up to five rows per bin, a ramp in each
        rows = (bins - 9) // 2 + 1
        W = np.zeros((rows, bins))
        for m in range(rows):
            W[m, 2 * m:2 * m + 9] = (1.0 + np.arange(9)) / 9.0
    elif name == "identity":
        W = np.eye(bins)
    else:
        raise KeyError(name)
    return torch.from_numpy(W).float()


def bands_numpy(W):
    """(row_lo, row_hi, col_lo, col_hi) of a staircase filterbank by plain loops -- what losses.filterbank_bands must return."""
    W = np.asarray(W)
    row_lo = [int(np.flatnonzero(r)[0]) for r in W]
    row_hi = [int(np.flatnonzero(r)[-1]) + 1 for r in W]
    col_lo, col_hi = [], []
    for k in range(W.shape[1]):
        touching = [m for m in range(W.shape[0]) if row_lo[m] <= k < row_hi[m]]
        # an uncovered bin: the empty run at the first row that begins beyond it
        at = touching[0] if touching else sum(1 for m in range(W.shape[0]) if row_hi[m] <= k)
        col_lo.append(at)
        col_hi.append(at + len(touching))
    return tuple(np.asarray(a, dtype=np.int32) for a in (row_lo, row_hi, col_lo, col_hi))


# ------------------------------------------------------------------------------------------------ the inputs
def inputs(name, n_fft, hop, L, kind, rows=f64.ROWS):
    """(pred, target) float32 on the CPU: stft_loss_float64.inputs, from another seed where RESEED says so."""
    offset = RESEED.get((name, n_fft, hop, L), 0)
    if not offset:
        return f64.inputs(n_fft, hop, L, kind, rows)
    g = torch.Generator().manual_seed(1000 * n_fft + hop + L + f64.RESEED.get((n_fft, hop, L), 0) + offset)
    target, noise = torch.randn(rows, L, generator=g), torch.randn(rows, L, generator=g)
    if kind == "noise":
        return noise, target
    return {"half": 0.5, "double": 2.0}[kind] * target + 0.02 * noise, target


# ------------------------------------------------------------------------------------------------ the definition
def band_magnitudes(x, n_fft, hop, window, eps, W):
    """W @ |stft(x)|: (rows, n_bins, frames)."""
    return torch.matmul(W, f64.magnitude(f64.spectrum(x, n_fft, hop, window), eps))


def sums_of(pred, target, n_fft, hop, window, eps, W):
    """(rows, 4) = (A, B, E, D) over the bands, in the dtype of the inputs; differentiable.  W None: over the bins."""
    if W is None:
        return f64.sums_of(pred, target, n_fft, hop, window, eps)
    P, T = (band_magnitudes(x, n_fft, hop, window, eps, W) for x in (pred, target))
    d = T - P
    return torch.stack([d.square().sum((-2, -1)), T.square().sum((-2, -1)), d.abs().sum((-2, -1)),
                        (T.log() - P.log()).abs().sum((-2, -1))], -1)


def sums_and_grad(pred, target, n_fft, hop, eps, W, coef=None):
    p = pred.double().requires_grad_(coef is not None)
    s = sums_of(p, target.double(), n_fft, hop, f64.hann(n_fft), eps, W.double())
    if coef is None:
        return s.detach(), None
    (s[:, (0, 2, 3)] * coef.double()).sum().backward()
    return s.detach(), p.grad


@functools.lru_cache(maxsize=None)
def reference(name, n_fft, hop, L, eps, kind, coef_name=None):
    """The float64 sums and gradient for a table filterbank and shape, an input kind and a named coefficient set."""
    pred, target = inputs(name, n_fft, hop, L, kind)
    coef = None if coef_name is None else f64.coefficients(coef_name, n_fft + hop + L)
    return sums_and_grad(pred, target, n_fft, hop, eps, filterbank(name, n_fft), coef)


def loss_and_grad(pred, target, resolutions, filterbanks, w_sc, w_log, w_lin, eps, sum_and_difference=False):
    """The module's loss in float64 and its gradient with respect to pred.  resolutions: (n_fft, hop, win_length) each;
    filterbanks: a matrix or None for each."""
    p = pred.double().requires_grad_(True)
    rows_p, rows_t = (f64.add_sum_and_difference(x) if sum_and_difference else x for x in (p, target.double()))
    L = pred.shape[-1]
    rows_p, rows_t = rows_p.reshape(-1, L), rows_t.reshape(-1, L)
    total = 0.0
    for (n_fft, hop, win_length), W in zip(resolutions, filterbanks):
        A, B, E, D = sums_of(rows_p, rows_t, n_fft, hop, f64.hann(n_fft, win_length), eps,
                             None if W is None else W.double()).unbind(-1)
        M = (n_fft // 2 + 1 if W is None else W.shape[0]) * (1 + L // hop)
        total = total + (w_sc * torch.sqrt(A / B) + w_log * D / M + w_lin * E / M).mean()
    loss = total / len(resolutions)
    loss.backward()
    return loss.detach(), p.grad


def margins(pred, target, n_fft, hop, eps, W):
    """How far the float64 bands of an input stay from where the gradient jumps: (the smallest |Tm - Pm| / mean Tm over
    the bands that are not equal exactly, the number of bands that are)."""
    w = f64.hann(n_fft)
    P, T = (band_magnitudes(x.double(), n_fft, hop, w, eps, W.double()) for x in (pred, target))
    d = (T - P).abs()
    return float(d[d > 0].min() / T.mean()), int((d == 0).sum())


# what the GPU tests differentiate through E and D: (filterbank, shape, kind)
GRADIENT_CASES = ([(name, s, k) for name in ("mel", "boxes") for s in f64.SHAPES for k in ("half", "double")]
                  + [(name, f64.SHAPES[0], "noise") for name in ("mel", "boxes")])
