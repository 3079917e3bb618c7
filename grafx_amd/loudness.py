"""Programme loudness after ITU-R BS.1770: K-weighting, mean squares over overlapping blocks, the two gates, LUFS.
:class:`IntegratedLoudness` meters a batch of signals on the GPU and is differentiable in them; :func:`loudness_normalize`
brings them to a target; :class:`TruePeak` and :func:`true_peak_normalize` are the other half of the recommendation, the
oversampled peak in dBTP.  The K-weighting filter and the sums of squares run in double on the native kernels of
csrc/loudness.hip (autograd.KWeightEnergyFn: the tape holds the signal alone); the gating is a handful of float64 torch ops
on the small (rows, channels, sub-blocks) tensor."""
import math

import torch
from torch import nn

from . import ops
from .autograd import KWeightEnergyFn, UpfirdnAbsmaxFn

# the analogue prototypes whose bilinear transform at 48 kHz is the standard's coefficient table
SHELF_F0, SHELF_GAIN_DB, SHELF_Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
SHELF_VB_EXPONENT = 0.4996667741545416
HIGHPASS_F0, HIGHPASS_Q = 38.13547087602444, 0.5003270373238773
LUFS_OFFSET = -0.691
MAX_BLOCK_HOPS = 16


def k_weighting(sample_rate):
    """The K-weighting of BS.1770 at ``sample_rate`` -> (Bs, As), two (2, 3) float64 tensors with a0 = 1: a high shelf
    (+4 dB above 1.68 kHz) and a 38 Hz high-pass, the standard's 48 kHz filters re-derived by the bilinear transform (at
    48 kHz they are the standard's table to 1e-15).  The shelf must lie below the Nyquist frequency."""
    fs = float(sample_rate)
    if not fs > 2.0 * SHELF_F0:
        raise ValueError(f"k_weighting: sample_rate={sample_rate} must be above {2.0 * SHELF_F0:.1f} Hz")
    K = math.tan(math.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXPONENT
    a0 = 1.0 + K / SHELF_Q + K * K
    b1 = [(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0]
    a1 = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0]
    K = math.tan(math.pi * HIGHPASS_F0 / fs)
    a0 = 1.0 + K / HIGHPASS_Q + K * K
    b2 = [1.0, -2.0, 1.0]
    a2 = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HIGHPASS_Q + K * K) / a0]
    return torch.tensor([b1, b2], dtype=torch.float64), torch.tensor([a1, a2], dtype=torch.float64)


def _lufs(p):
    """-0.691 + 10 log10 p where p > 0, -inf elsewhere, with a zero gradient there (no NaN either way)."""
    positive = p > 0
    safe = torch.where(positive, p, torch.ones_like(p))
    return torch.where(positive, LUFS_OFFSET + 10.0 * torch.log10(safe), torch.full_like(p, -math.inf))


def _block_power(energy, block_hops, channel_gains):
    """p[..., j] = sum_c G_c z_cj, z_cj the mean of sub-blocks j .. j + block_hops - 1 of channel c."""
    if energy.ndim < 2:
        raise ValueError(f"energy must be (..., C, n_sub), got {tuple(energy.shape)}")
    n_sub = energy.shape[-1]
    if not 1 <= block_hops <= n_sub:
        raise ValueError(f"block_hops={block_hops} must be in 1..n_sub={n_sub}")
    e = energy.double()
    G = torch.as_tensor(channel_gains, dtype=torch.float64, device=e.device)
    if G.shape != (e.shape[-2],):
        raise ValueError(f"channel_gains {tuple(G.shape)} must hold one gain per channel ({e.shape[-2]})")
    n_blocks = n_sub - block_hops + 1
    z = e[..., 0:n_blocks]
    for i in range(1, block_hops):          # (at most MAX_BLOCK_HOPS shifted views: no cumulative sum to cancel in)
        z = z + e[..., i:i + n_blocks]
    return (z * G[:, None]).sum(-2) / block_hops


def gated_loudness(energy, block_hops, channel_gains, absolute_gate=-70.0, relative_gate=-10.0):
    """Integrated loudness in LUFS from sub-block energies -> (...) float64.

    ``energy``: (..., C, n_sub), the MEAN square of the K-weighted signal over consecutive sub-blocks of ``hop`` samples
    (ops.kweight_energy divided by ``hop``).  Gating block j is sub-blocks j .. j + block_hops - 1, z_cj their mean,
    l_j = -0.691 + 10 log10 sum_c G_c z_cj.  The absolute gate keeps the blocks with l_j > ``absolute_gate``; the relative
    threshold is the loudness of their mean plus ``relative_gate``; the result is -0.691 + 10 log10 of the mean over the
    blocks above both.  Which blocks pass is computed without gradient -- a constant of the derivative.  An item without
    a surviving block gives -inf and a zero gradient; no NaN is produced.  Plain torch ops in float64 on the device of
    ``energy``, masks and sums only: nothing synchronises with the host."""
    p = _block_power(energy, block_hops, channel_gains)
    with torch.no_grad():
        level = _lufs(p)
        above = level > absolute_gate
        count = above.sum(-1, keepdim=True)
        mean = torch.where(above, p, torch.zeros_like(p)).sum(-1, keepdim=True) / count.clamp(min=1)
        keep = above & (level > _lufs(mean) + relative_gate)
        kept = keep.sum(-1)
    gated = torch.where(keep, p, torch.zeros_like(p)).sum(-1) / kept.clamp(min=1)
    return _lufs(gated)


class IntegratedLoudness(nn.Module):
    """Integrated loudness (BS.1770-4) of ``x`` (..., C, L) in LUFS -> (...), in ``x.dtype``, differentiable in ``x``.

    Gating blocks of ``block`` seconds overlapping by ``overlap``: ``sample_rate * block * (1 - overlap)`` must be a whole
    number of samples (the hop) and the block a whole number of hops, at most 16; a signal shorter than one block is
    refused.  ``channel_gains``: G_c per channel (default ones; 1.41 for surround channels).  ``block_loudness`` gives the
    ungated l_j -- with the defaults the momentary loudness every 100 ms.  The signal must be float32 on the GPU: the
    filter and the sums of squares are one native call (ops.kweight_energy), and autograd keeps ``x`` alone."""

    def __init__(self, sample_rate, block=0.4, overlap=0.75, channel_gains=None, absolute_gate=-70.0, relative_gate=-10.0):
        super().__init__()
        if not 0.0 <= overlap < 1.0 or not block > 0:
            raise ValueError(f"block={block} must be positive and overlap={overlap} in [0, 1)")
        hop = sample_rate * block * (1.0 - overlap)
        self.hop = int(round(hop))
        if self.hop < 1 or abs(hop - self.hop) > 1e-9 * max(hop, 1.0):
            raise ValueError(f"sample_rate * block * (1 - overlap) = {hop!r} is not a whole number of samples")
        hops = sample_rate * block / self.hop
        self.block_hops = int(round(hops))
        if abs(hops - self.block_hops) > 1e-9 * hops or not 1 <= self.block_hops <= MAX_BLOCK_HOPS:
            raise ValueError(f"a block of {sample_rate * block!r} samples is {hops!r} hops of {self.hop}: a whole number "
                             f"in 1..{MAX_BLOCK_HOPS} expected")
        Bs, As = k_weighting(sample_rate)
        self.sample_rate, self.absolute_gate, self.relative_gate = sample_rate, float(absolute_gate), float(relative_gate)
        self.coef = torch.cat([Bs, As[:, 1:]], 1)          # (2, 5) float64 on the host: what the kernels read at the call
        self.channel_gains = None if channel_gains is None else tuple(float(g) for g in channel_gains)

    def energies(self, x):
        """(..., C, L) -> (..., C, n_sub) float64: the mean squares of the K-weighted signal per sub-block of ``hop``."""
        if x.ndim < 2:
            raise ValueError(f"IntegratedLoudness: x must be (..., C, L), got {tuple(x.shape)}")
        if x.shape[-1] < self.block_hops * self.hop:
            raise ValueError(f"IntegratedLoudness: {x.shape[-1]} samples are less than one block of "
                             f"{self.block_hops * self.hop}")
        ops._require_gpu(x)
        if x.ndim == 2:
            rows = x.unsqueeze(0)
        elif x.ndim > 4 or x.stride(-1) != 1:
            rows = x.reshape(-1, *x.shape[-2:])
        else:
            rows = x                                       # (R,C,L) or a strided (B,n,C,L) view, read in place
        sums = KWeightEnergyFn.apply(rows, self.coef, self.hop)
        return sums.view(*x.shape[:-1], -1) / self.hop

    def _gains(self, x):
        return (1.0,) * x.shape[-2] if self.channel_gains is None else self.channel_gains

    def block_loudness(self, x):
        """The ungated loudness l_j of every gating block -> (..., n_blocks) in ``x.dtype``; -inf for a silent block."""
        return _lufs(_block_power(self.energies(x), self.block_hops, self._gains(x))).to(x.dtype)

    def forward(self, x):
        return gated_loudness(self.energies(x), self.block_hops, self._gains(x), self.absolute_gate,
                              self.relative_gate).to(x.dtype)


def loudness_normalize(x, target_lufs, meter, detach_gain=False):
    """``x`` (..., C, L) scaled per item to ``target_lufs`` as ``meter`` (an :class:`IntegratedLoudness`) measures it:
    x * 10^((target - L) / 20).  An item at -inf (nothing above the gates) is returned unchanged.  ``detach_gain``: the gain
    is a constant of the gradient (the usual choice for a target signal); otherwise the gradient flows through the meter
    as well."""
    level = meter(x)
    if detach_gain:
        level = level.detach()
    finite = torch.isfinite(level)
    level = torch.where(finite, level, torch.full_like(level, float(target_lufs)))
    gain = torch.pow(10.0, (float(target_lufs) - level) / 20.0)
    return x * gain[..., None, None]


def _dbtp(p):
    """20 log10 p where p > 0, -inf elsewhere, with a zero gradient there (no NaN either way)."""
    positive = p > 0
    safe = torch.where(positive, p, torch.ones_like(p))
    return torch.where(positive, 20.0 * torch.log10(safe), torch.full_like(p, -math.inf))


class TruePeak(nn.Module):
    """True-peak level (BS.1770 Annex 2) of ``x`` (..., C, L) in dBTP -> (...), in ``x.dtype``, differentiable in ``x``:
    20 log10 of the largest |y| over the item's channels, y being ``x`` oversampled by ``oversample`` (``oversample * L``
    samples per channel); -inf for a silent item, with a zero gradient there and no NaN.  ``channel_peaks`` gives the linear
    peak per channel, (..., C).

    The default taps are ``resample.sinc_kernel(1, oversample)``: 49 taps at 4x, about 12 per phase, which is the structure
    of BS.1770 Annex 2.  The standard's own 48-coefficient table is not reproduced here, so it is not the default;
    ``taps=`` takes any 1-D prototype at the oversampled rate (the table, for whoever has it), and ``offset`` is then
    (N - 1) // 2.  The signal must be float32 on the GPU: the meter is one native call (ops.upfirdn_absmax) and the
    oversampled signal never reaches memory.  The gradient of a channel's peak lands on the at most ceil(N / oversample)
    input samples under the tap window of the output that attains it (autograd.UpfirdnAbsmaxFn)."""

    def __init__(self, oversample=4, taps=None):
        super().__init__()
        if isinstance(oversample, bool) or not isinstance(oversample, int) or not 1 <= oversample <= ops.UPFIRDN_MAX_RATIO:
            raise ValueError(f"TruePeak: oversample={oversample!r} must be an integer in 1..{ops.UPFIRDN_MAX_RATIO}")
        if taps is None:
            from .resample import sinc_kernel

            h, _, _, self.offset = sinc_kernel(1, oversample)
        else:
            h = torch.as_tensor(taps).detach().cpu()
            if h.ndim != 1 or not 1 <= h.numel() <= ops.UPFIRDN_MAX_TAPS:
                raise ValueError(f"TruePeak: taps must hold 1..{ops.UPFIRDN_MAX_TAPS} values in one dimension, got "
                                 f"{tuple(h.shape)}")
            self.offset = (h.numel() - 1) // 2
        self.oversample = oversample
        self.register_buffer("taps", h.float(), persistent=False)

    def channel_peaks(self, x):
        """(..., C, L) -> (..., C) float32: the largest magnitude of every channel's oversampled signal."""
        if x.ndim < 2:
            raise ValueError(f"TruePeak: x must be (..., C, L), got {tuple(x.shape)}")
        ops._require_gpu(x)
        if x.ndim == 2:
            rows = x.unsqueeze(0)
        elif x.ndim > 4 or x.stride(-1) != 1:
            rows = x.reshape(-1, *x.shape[-2:])
        else:
            rows = x                                       # (R,C,L) or a strided (B,n,C,L) view, read in place
        peak, _ = UpfirdnAbsmaxFn.apply(rows, self.taps, self.oversample, 1, self.offset, self.oversample * x.shape[-1])
        return peak.view(x.shape[:-1])

    def forward(self, x):
        return _dbtp(self.channel_peaks(x).amax(-1)).to(x.dtype)


def true_peak_normalize(x, target_dbtp, meter, detach_gain=False):
    """``x`` (..., C, L) scaled per item to a true peak of ``target_dbtp`` as ``meter`` (a :class:`TruePeak`) measures it:
    x * 10^((target - level) / 20).  A silent item (-inf) is returned unchanged.  ``detach_gain``: the gain is a constant of
    the gradient; otherwise the gradient flows through the meter as well."""
    level = meter(x)
    if detach_gain:
        level = level.detach()
    finite = torch.isfinite(level)
    level = torch.where(finite, level, torch.full_like(level, float(target_dbtp)))
    gain = torch.pow(10.0, (float(target_dbtp) - level) / 20.0)
    return x * gain[..., None, None]
