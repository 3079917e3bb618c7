"""Sample-rate conversion by a rational polyphase FIR on the GPU: :func:`sinc_kernel` designs the prototype filter on the
host, :class:`Resample` applies it through the native kernel of csrc/upfirdn.hip (autograd.UpfirdnFn: one call forward, one
backward, the tape holds the taps and the signal's shape), :func:`resample` is the functional form."""
import math

import torch
from torch import nn

from . import ops
from .autograd import UpfirdnFn


def _geometry(orig_freq, new_freq, lowpass_filter_width, rolloff):
    """The arguments of a design, checked -> the reduced rates, the cutoff ``base`` and the filter's half length."""
    for name, f in (("orig_freq", orig_freq), ("new_freq", new_freq)):
        if isinstance(f, bool) or not isinstance(f, int) or f < 1:
            raise ValueError(f"sinc_kernel: {name}={f!r} must be a positive integer")
    if isinstance(lowpass_filter_width, bool) or not isinstance(lowpass_filter_width, int) or lowpass_filter_width < 1:
        raise ValueError(f"sinc_kernel: lowpass_filter_width={lowpass_filter_width!r} must be a positive integer")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"sinc_kernel: rolloff={rolloff!r} must be in (0, 1]")
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    return orig, new, base, int(math.floor(lowpass_filter_width * orig * new / base))


def sinc_kernel(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The Hann-windowed sinc of the widely used torch audio resampler, restated as ONE prototype filter at the rate
    orig * new (both reduced by their gcd) -> (h, up, down, offset): ``h`` float64 on the host, 2 half + 1 taps,
    ``up = new``, ``down = orig``, ``offset = half``.  With base = min(orig, new) rolloff, half = floor(width orig new / base)
    and t = q base / (orig new) for q = -half .. half:
        h[q + half] = (base / orig) sinc(t) cos^2(pi t / (2 width))   where |t| < width, else 0.
    y[m] = sum_k x[k] h[m down + offset - k up] is then the signal at the new rate."""
    orig, new, base, half = _geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    t = torch.arange(-half, half + 1, dtype=torch.float64) * (base / (orig * new))
    window = torch.cos(t * (math.pi / (2.0 * lowpass_filter_width))) ** 2
    h = (base / orig) * torch.sinc(t) * window
    h = torch.where(t.abs() < lowpass_filter_width, h, torch.zeros_like(h))
    return h, new, orig, half


class Resample(nn.Module):
    """``x`` (..., C, L) float32 on the GPU at ``orig_freq`` -> (..., C, ceil(L new / orig)) at ``new_freq``, differentiable in
    ``x``.  The filter is :func:`sinc_kernel`; the work is one native polyphase call (ops.upfirdn) each way, and autograd keeps
    the taps and the shape of ``x``, no signal.  A (R, C, L) tensor or a strided (B, n, C, L) view is read in place.  Equal
    rates return ``x`` itself.  A ratio whose reduced form or tap count is beyond the kernel (up, down <= 1024, 16384 taps)
    is refused at construction: there is no other route.  The taps are a float32 buffer that follows ``.to(device)``."""

    def __init__(self, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
        super().__init__()
        orig, new, _, half = _geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
        if max(orig, new) > ops.UPFIRDN_MAX_RATIO or 2 * half + 1 > ops.UPFIRDN_MAX_TAPS:      # (before the taps are built)
            raise ValueError(f"Resample: {orig_freq} -> {new_freq} reduces to {orig}/{new} with {2 * half + 1} taps; the "
                             f"kernel takes ratios up to {ops.UPFIRDN_MAX_RATIO} and {ops.UPFIRDN_MAX_TAPS} taps")
        h, self.up, self.down, self.offset = sinc_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.orig_freq, self.new_freq = orig_freq, new_freq
        self.register_buffer("taps", h.float(), persistent=False)

    def forward(self, x):
        if x.ndim < 2:
            raise ValueError(f"Resample: x must be (..., C, L), got {tuple(x.shape)}")
        ops._require_gpu(x)
        if self.up == self.down:
            return x
        if x.ndim == 2:
            rows = x.unsqueeze(0)
        elif x.ndim > 4 or x.stride(-1) != 1:
            rows = x.reshape(-1, *x.shape[-2:])
        else:
            rows = x                                       # (R,C,L) or a strided (B,n,C,L) view, read in place
        n_out = -(-x.shape[-1] * self.up // self.down)
        y = UpfirdnFn.apply(rows, self.taps, self.up, self.down, self.offset, n_out)
        return y.view(*x.shape[:-1], n_out)


_MODULES = {}


def resample(x, orig_freq, new_freq, **design):
    """:class:`Resample` as a function; the modules are cached by their arguments and the device of ``x``."""
    key = (orig_freq, new_freq, tuple(sorted(design.items())), x.device)
    module = _MODULES.get(key)
    if module is None:
        module = _MODULES[key] = Resample(orig_freq, new_freq, **design).to(x.device)
    return module(x)
