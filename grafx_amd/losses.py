"""Losses of a training step.  :class:`MultiResolutionSTFTLoss` is the multi-resolution STFT magnitude loss -- spectral
convergence, log-magnitude L1 and linear-magnitude L1 over several (n_fft, hop, window) resolutions -- on native kernels:
per resolution, pred and target are read once, four sums per row come back, and the backward recomputes the frames
instead of keeping spectrograms on autograd's tape (csrc/stft_loss.hip)."""
import torch
from torch import nn

from . import ops
from .autograd import StftLossSumsFn

NATIVE_MIN_FFT, NATIVE_MAX_FFT = 128, 2048      # the LDS frame transform of csrc/stft_loss.hip: powers of two in this range


def padded_hann(win_length, n_fft):
    """The Hann window of ``win_length`` samples, zero-padded to ``n_fft`` and centred as torch.stft(win_length=) does."""
    if not 0 < win_length <= n_fft:
        raise ValueError(f"win_length={win_length} must be in 1..n_fft={n_fft}")
    left = (n_fft - win_length) // 2
    return nn.functional.pad(torch.hann_window(win_length), (left, n_fft - win_length - left))


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
    has no parameters."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(256, 512, 128), win_lengths=None, w_sc=1.0, w_log_mag=1.0,
                 w_lin_mag=0.0, eps=1e-8, sum_and_difference=False):
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
        M = torch.tensor([(n // 2 + 1) * (1 + L // hop) for n, hop in zip(self.fft_sizes, self.hop_sizes)],
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
        for n, hop, w in zip(self.fft_sizes, self.hop_sizes, self.windows(p)):
            mag = [torch.sqrt(torch.clamp(torch.view_as_real(torch.stft(x, n, hop, window=w, center=True, pad_mode="reflect",
                                                                        return_complex=True)).square().sum(-1), min=self.eps))
                   for x in (p, t)]
            diff = mag[1] - mag[0]
            sums.append(torch.stack([diff.square().sum((-2, -1)), mag[1].square().sum((-2, -1)), diff.abs().sum((-2, -1)),
                                     (mag[1].log() - mag[0].log()).abs().sum((-2, -1))], -1))
        return self.combine(torch.stack(sums, 1), L).to(pred.dtype)

    def native(self, L):
        return all(NATIVE_MIN_FFT <= n <= NATIVE_MAX_FFT and n & (n - 1) == 0 and 1 <= hop <= n and L > n // 2
                   for n, hop in zip(self.fft_sizes, self.hop_sizes))

    def forward(self, pred, target):
        self._check(pred, target)
        L = pred.shape[-1]
        if not self.native(L):
            ops.fft_library_reached("MultiResolutionSTFTLoss")
            return self.torch_forward(pred, target)
        ops._require_gpu(pred, target)
        sums = StftLossSumsFn.apply(self.rows(pred), self.rows(target), self.eps, self.hop_sizes, *self.windows(pred))
        return self.combine(sums, L).to(pred.dtype)
