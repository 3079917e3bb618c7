"""Losses of a training step.  :class:`MultiResolutionSTFTLoss` is the multi-resolution STFT magnitude loss -- spectral
convergence, log-magnitude L1 and linear-magnitude L1 over several (n_fft, hop, window) resolutions -- on native kernels:
per resolution, pred and target are read once, four sums per row come back, and the backward recomputes the frames
instead of keeping spectrograms on autograd's tape (csrc/stft_loss.hip).  A resolution may compare
filterbank bands instead of bins -- a mel scale (:func:`mel_filterbank`), A-weighted bins (:func:`a_weighting`), any
staircase-banded matrix (:func:`filterbank_bands`) -- on the kernels of csrc/stft_band_loss.hip."""
import math

import torch
from torch import nn

from . import ops
from .autograd import StftBandLossSumsFn, StftLossSumsFn

NATIVE_MIN_FFT, NATIVE_MAX_FFT = 128, 2048      # the LDS frame transform of csrc/stft_loss.hip: powers of two in this range
BAND_NAMES = ("row_lo", "row_hi", "col_lo", "col_hi")


def padded_hann(win_length, n_fft):
    """The Hann window of ``win_length`` samples, zero-padded to ``n_fft`` and centred as torch.stft(win_length=) does."""
    if not 0 < win_length <= n_fft:
        raise ValueError(f"win_length={win_length} must be in 1..n_fft={n_fft}")
    left = (n_fft - win_length) // 2
    return nn.functional.pad(torch.hann_window(win_length), (left, n_fft - win_length - left))


def _hz_to_mel(f, htk):
    f = torch.as_tensor(f, dtype=torch.float64)
    if htk:
        return 2595.0 * torch.log10(1.0 + f / 700.0)
    # Slaney: linear below 1 kHz (200 / 3 Hz per mel), logarithmic from there on (27 mels per factor of 6.4)
    return torch.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + torch.log(torch.clamp(f, min=1000.0) / 1000.0) / (math.log(6.4) / 27.0))


def _mel_to_hz(m, htk):
    if htk:
        return 700.0 * (torch.pow(10.0, m / 2595.0) - 1.0)
    return torch.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * torch.exp((m - 15.0) * (math.log(6.4) / 27.0)))


def mel_filterbank(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None, htk=False, norm="slaney"):
    """(n_mels, n_fft / 2 + 1) float32 triangles between ``n_mels + 2`` points equally spaced in mel from ``f_min`` to
    ``f_max`` (default: sample_rate / 2), on the Slaney scale (mel = f / (200/3) below 1 kHz, 15 + ln(f / 1000) / (ln 6.4 / 27)
    from there on) or, with ``htk``, 2595 log10(1 + f / 700).  ``norm="slaney"`` scales row m by 2 / (f[m + 2] - f[m]);
    ``norm=None`` leaves unit peaks.  Computed in float64.  Too many bands for the transform leave rows without a bin:
    :func:`filterbank_bands` refuses those."""
    if norm not in (None, "slaney"):
        raise ValueError(f"mel_filterbank: norm={norm!r} must be None or 'slaney'")
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    if n_mels < 1 or not 0.0 <= f_min < f_max <= sample_rate / 2.0:
        raise ValueError(f"mel_filterbank: n_mels={n_mels} and 0 <= f_min={f_min} < f_max={f_max} <= sample_rate / 2 expected")
    freqs = torch.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1, dtype=torch.float64)
    lo, hi = _hz_to_mel(f_min, htk), _hz_to_mel(f_max, htk)
    points = _mel_to_hz(torch.linspace(float(lo), float(hi), n_mels + 2, dtype=torch.float64), htk)
    rise = (freqs[None, :] - points[:-2, None]) / (points[1:-1] - points[:-2])[:, None]
    fall = (points[2:, None] - freqs[None, :]) / (points[2:] - points[1:-1])[:, None]
    W = torch.clamp(torch.minimum(rise, fall), min=0.0)
    if norm == "slaney":
        W = W * (2.0 / (points[2:] - points[:-2]))[:, None]
    return W.float()


def a_weighting(sample_rate, n_fft):
    """The n_fft / 2 + 1 gains of IEC 61672's A curve at the bin frequencies, float32, 1 at 1 kHz and 0 at DC:
    R_A(f) = 12194^2 f^4 / ((f^2 + 20.6^2) sqrt((f^2 + 107.7^2)(f^2 + 737.9^2)) (f^2 + 12194^2)), divided by R_A(1000)."""
    def r_a(f):
        f2 = f * f
        return 12194.0 ** 2 * f2 * f2 / ((f2 + 20.6 ** 2) * torch.sqrt((f2 + 107.7 ** 2) * (f2 + 737.9 ** 2)) * (f2 + 12194.0 ** 2))

    freqs = torch.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1, dtype=torch.float64)
    return (r_a(freqs) / r_a(torch.tensor(1000.0, dtype=torch.float64))).float()


def filterbank_bands(W):
    """The band structure of an (n_bins, n_fft / 2 + 1) filterbank the native kernels take -> (row_lo, row_hi, col_lo,
    col_hi), int32 on W's device: the non-zeros of row m are the one run [row_lo[m], row_hi[m]) with both ends
    non-decreasing in m (a staircase), and the rows that touch bin k are [col_lo[k], col_hi[k]) -- empty for a bin no row
    covers.  None for a matrix that is not of this form (a gap inside a row, rows out of order): it is no error, such a
    loss runs as torch ops.  ValueError for a negative weight and for a row without any weight, whose band has no
    logarithm."""
    if W.ndim != 2:
        raise ValueError(f"filterbank_bands: an (n_bins, n_fft / 2 + 1) matrix expected, got {tuple(W.shape)}")
    M = W.detach().cpu()
    negative = (M < 0).any(1).nonzero()
    if negative.numel():
        raise ValueError(f"filterbank_bands: row {int(negative[0])} holds a negative weight")
    nz = M > 0
    count = nz.sum(1)
    empty = (count == 0).nonzero()
    if empty.numel():
        raise ValueError(f"filterbank_bands: row {int(empty[0])} has no weight on any of the {M.shape[1]} bins")
    bins = torch.arange(M.shape[1])
    row_lo = torch.where(nz, bins, M.shape[1]).amin(1)
    row_hi = torch.where(nz, bins, -1).amax(1) + 1
    if not torch.equal(row_hi - row_lo, count) or (row_lo.diff() < 0).any() or (row_hi.diff() < 0).any():
        return None
    # both ends are sorted: the rows that end at or before bin k are a prefix, and so are the rows that begin at or before it
    col_lo = torch.searchsorted(row_hi, bins, right=True)
    col_hi = torch.searchsorted(row_lo, bins, right=True)
    return tuple(t.to(torch.int32).to(W.device) for t in (row_lo, row_hi, col_lo, col_hi))


class MultiResolutionSTFTLoss(nn.Module):
    r"""mean over resolutions i and rows r of

        w_sc * sqrt(A / B)  +  w_log_mag * D / M_i  +  w_lin_mag * E / M_i,        M_i = (n_fft_i / 2 + 1) * frames_i,

    with, for P = torch.stft(pred row, n_fft, hop, window, center=True, pad_mode="reflect") and T likewise of the target,
    |.| = sqrt(clamp(re^2 + im^2, min=eps)):  A = sum (|T|-|P|)^2,  B = sum |T|^2,  E = sum ||T|-|P||,
    D = sum |log|T| - log|P||  over all bins and frames.

    ``forward(pred, target)``: (..., L) tensors of one shape; every leading index is a row.  ``sum_and_difference`` (the
    axis before the last must then hold two channels) appends the rows l + r and l - r.  The target gets no gradient.
    Resolutions whose n_fft is a power of two in [128, 2048] run on the native kernels; if any resolution is not,
    ``forward`` says so (ops.FftLibraryWarning) and returns ``torch_forward``, the same formula as torch ops.  The module
    has no parameters.

    Filterbank scales.  With an (n_bins_i, n_fft_i / 2 + 1) matrix W_i of non-negative weights for resolution i, the sums
    run over the bands Pm = W_i |P|, Tm = W_i |T| of every frame instead of the bins (the clamp stays on the bins, the
    logarithm moves to the bands) and M_i = n_bins_i * frames_i.  ``filterbanks``: one entry per resolution, a matrix or
    None (plain bins).  ``scale="mel"`` with ``n_bins`` and ``sample_rate`` builds :func:`mel_filterbank` for every
    resolution instead (not both).  ``perceptual_weighting`` (needs ``sample_rate``) multiplies the columns of each
    resolution's filterbank by :func:`a_weighting`, and where there is none uses the diagonal of those gains without the
    DC bin, whose gain is 0 (n_bins = n_fft / 2).  This weights magnitudes per bin: it is not a time-domain FIR prefilter
    in front of the transform, from which it differs by the window's leakage.  Staircase-banded filterbanks
    (:func:`filterbank_bands`) run on the native kernels, any other takes ``torch_forward`` under the same warning.  The
    filterbanks get no gradient; they and their bands are buffers that are not saved with the module."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(256, 512, 128), win_lengths=None, w_sc=1.0, w_log_mag=1.0,
                 w_lin_mag=0.0, eps=1e-8, sum_and_difference=False, filterbanks=None, scale=None, n_bins=None, sample_rate=None,
                 perceptual_weighting=False):
        super().__init__()
        win_lengths = tuple(fft_sizes) if win_lengths is None else tuple(win_lengths)
        if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths) > 0):
            raise ValueError("fft_sizes, hop_sizes and win_lengths must have one entry per resolution")
        if eps <= 0:
            raise ValueError(f"eps={eps} must be positive")
        self.fft_sizes, self.hop_sizes, self.win_lengths = tuple(fft_sizes), tuple(hop_sizes), win_lengths
        self.w_sc, self.w_log_mag, self.w_lin_mag, self.eps = float(w_sc), float(w_log_mag), float(w_lin_mag), float(eps)
        self.sum_and_difference = bool(sum_and_difference)
        for i, (n, wl) in enumerate(zip(self.fft_sizes, win_lengths)):
            self.register_buffer(f"window_{i}", padded_hann(wl, n), persistent=False)
        self.band_counts, self.staircase = [], True
        for i, W in enumerate(self._filterbanks(filterbanks, scale, n_bins, sample_rate, perceptual_weighting)):
            self.band_counts.append(self.fft_sizes[i] // 2 + 1 if W is None else W.shape[0])
            self.register_buffer(f"filterbank_{i}", W, persistent=False)
            try:
                bands = None if W is None else filterbank_bands(W)
            except ValueError as e:
                hint = f" (n_bins={n_bins} mel bands are too many for n_fft={self.fft_sizes[i]})" if scale == "mel" else ""
                raise ValueError(f"MultiResolutionSTFTLoss: resolution {i}: {e}{hint}") from None
            self.staircase = self.staircase and (W is None or bands is not None)
            for name, b in zip(BAND_NAMES, bands or (None,) * 4):
                self.register_buffer(f"{name}_{i}", b, persistent=False)

    def _filterbanks(self, filterbanks, scale, n_bins, sample_rate, perceptual_weighting):
        """One matrix or None per resolution from the constructor's keywords."""
        if scale not in (None, "mel"):
            raise ValueError(f"scale={scale!r} must be None or 'mel'")
        if scale is not None and filterbanks is not None:
            raise ValueError("give filterbanks or scale, not both")
        if (scale is not None or perceptual_weighting) and sample_rate is None:
            raise ValueError("scale and perceptual_weighting need sample_rate")
        if scale == "mel":
            if n_bins is None:
                raise ValueError("scale='mel' needs n_bins")
            banks = [mel_filterbank(sample_rate, n, n_bins) for n in self.fft_sizes]
        elif filterbanks is None:
            banks = [None] * len(self.fft_sizes)
        else:
            banks = list(filterbanks)
            if len(banks) != len(self.fft_sizes):
                raise ValueError("filterbanks must have one entry (a matrix or None) per resolution")
            for i, (W, n) in enumerate(zip(banks, self.fft_sizes)):
                if W is None:
                    continue
                if not isinstance(W, torch.Tensor) or W.ndim != 2 or W.shape[1] != n // 2 + 1 or W.shape[0] < 1:
                    raise ValueError(f"filterbank {i} must be (n_bins, n_fft / 2 + 1 = {n // 2 + 1}), got "
                                     f"{tuple(W.shape) if isinstance(W, torch.Tensor) else type(W).__name__}")
                if W.requires_grad:
                    raise ValueError(f"filterbank {i} requires grad: filterbanks are not learnable here (detach it)")
                banks[i] = W.detach().float().clone()
        if perceptual_weighting:
            for i, n in enumerate(self.fft_sizes):
                gains = a_weighting(sample_rate, n)
                banks[i] = torch.diag(gains)[1:] if banks[i] is None else banks[i] * gains.to(banks[i].device)
        return banks

    def filterbanks(self, like):
        """(W, bands) per resolution on ``like``'s device -- (None, None) for plain bins, bands None off the staircase."""
        out = []
        for i in range(len(self.fft_sizes)):
            W = getattr(self, f"filterbank_{i}")
            bands = tuple(getattr(self, f"{name}_{i}") for name in BAND_NAMES)
            if W is not None:
                W = W if (W.device, W.dtype) == (like.device, like.dtype) else W.to(like)
            out.append((W, None if bands[0] is None else tuple(b.to(like.device) for b in bands)))
        return out

    def windows(self, like):
        return [w if (w.device, w.dtype) == (like.device, like.dtype) else w.to(like)
                for w in (getattr(self, f"window_{i}") for i in range(len(self.fft_sizes)))]

    def rows(self, x):
        """(..., L) -> the signal whose leading indices are the rows of the loss: x itself, or with the sum and the difference
        of its two channels appended."""
        if not self.sum_and_difference:
            return x
        if x.ndim < 2 or x.shape[-2] != 2:
            raise ValueError(f"sum_and_difference needs two channels on the axis before the last, got {tuple(x.shape)}")
        left, right = x[..., 0:1, :], x[..., 1:2, :]
        return torch.cat([x, left + right, left - right], -2)

    def combine(self, sums, L):
        """The loss from the (R, n_res, 4) sums, in float64.  A = 0 (pred is target) gives no spectral-convergence term and
        no gradient through it instead of sqrt's infinite slope."""
        A, B, E, D = sums.double().unbind(-1)
        M = torch.tensor([bands * (1 + L // hop) for bands, hop in zip(self.band_counts, self.hop_sizes)],
                         dtype=torch.float64, device=sums.device)
        zero = A <= 0
        sc = torch.where(zero, torch.zeros_like(A), torch.sqrt(torch.where(zero, torch.ones_like(A), A) / B))
        return (self.w_sc * sc + self.w_log_mag * D / M + self.w_lin_mag * E / M).mean()

    def _check(self, pred, target):
        if target.requires_grad:
            raise ValueError("MultiResolutionSTFTLoss: the target gets no gradient (detach it)")
        if pred.shape != target.shape or pred.ndim < 2:
            raise ValueError(f"MultiResolutionSTFTLoss: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be "
                             f"(..., L) tensors of one shape")

    def torch_forward(self, pred, target):
        """The same loss as torch ops (torch.stft and autograd, in the inputs' dtype): the definition the kernels are held
        to, and the path of the resolutions they do not cover."""
        self._check(pred, target)
        p, t = self.rows(pred), self.rows(target)
        L = p.shape[-1]
        p, t = p.reshape(-1, L), t.reshape(-1, L)
        sums = []
        for n, hop, w, (W, _) in zip(self.fft_sizes, self.hop_sizes, self.windows(p), self.filterbanks(p)):
            mag = [torch.sqrt(torch.clamp(torch.view_as_real(torch.stft(x, n, hop, window=w, center=True, pad_mode="reflect",
                                                                        return_complex=True)).square().sum(-1), min=self.eps))
                   for x in (p, t)]
            if W is not None:
                mag = [torch.matmul(W, m) for m in mag]      # (n_bins, bins) @ (rows, bins, frames)
            diff = mag[1] - mag[0]
            sums.append(torch.stack([diff.square().sum((-2, -1)), mag[1].square().sum((-2, -1)), diff.abs().sum((-2, -1)),
                                     (mag[1].log() - mag[0].log()).abs().sum((-2, -1))], -1))
        return self.combine(torch.stack(sums, 1), L).to(pred.dtype)

    def native(self, L):
        return self.staircase and all(NATIVE_MIN_FFT <= n <= NATIVE_MAX_FFT and n & (n - 1) == 0 and 1 <= hop <= n and L > n // 2
                   for n, hop in zip(self.fft_sizes, self.hop_sizes))

    def forward(self, pred, target):
        self._check(pred, target)
        L = pred.shape[-1]
        if not self.native(L):
            ops.fft_library_reached("MultiResolutionSTFTLoss")
            return self.torch_forward(pred, target)
        ops._require_gpu(pred, target)
        banks = self.filterbanks(pred)
        if all(W is None for W, _ in banks):
            sums = StftLossSumsFn.apply(self.rows(pred), self.rows(target), self.eps, self.hop_sizes, *self.windows(pred))
        else:
            sums = StftBandLossSumsFn.apply(self.rows(pred), self.rows(target), self.eps, self.hop_sizes,
                                            tuple(W is not None for W, _ in banks), *self.windows(pred),
                                            *(t for W, bands in banks if W is not None for t in (W, *bands)))
        return self.combine(sums, L).to(pred.dtype)
