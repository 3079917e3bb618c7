"""Float64 yardstick of the polyphase FIR (tests/test_gpu_upfirdn.py, tests/test_gpu_true_peak.py, tests/test_upfirdn_abi.py):
its own statement of the resampling filter, the formula

    y[m] = sum_k x[k] h[m down + offset - k up],   0 <= m < M,   x zero outside [0, L), h zero outside [0, N)

as a direct float64 sum and through scipy.signal.upfirdn, the adjoint, the peak with its first index, and seeded inputs.
Everything is evaluated on the float32-rounded taps and inputs the GPU gets.  Not a test module."""
import math

import numpy as np
import torch
from scipy import signal as sps

ROWS = 2


def sinc_kernel(orig_freq, new_freq, width=6, rolloff=0.99):
    """-> (h float64, up, down, offset): the Hann-windowed sinc at the rate orig * new, rates reduced by their gcd."""
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    half = int(math.floor(width * orig * new / base))
    h = np.zeros(2 * half + 1)
    for q in range(-half, half + 1):
        t = q * base / (orig * new)
        if abs(t) < width:
            s = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            h[q + half] = (base / orig) * s * math.cos(math.pi * t / (2.0 * width)) ** 2
    return h, new, orig, half


def taps32(h):
    """The taps as the GPU gets them: rounded to float32 -> (float64 array of the rounded values, float32 tensor)."""
    t = torch.as_tensor(np.asarray(h, dtype=np.float64)).float()
    return t.double().numpy(), t


def default_n_out(L, N, up, down, offset):
    return -(-(L * up + N - 1 - offset) // down)


def upfirdn_direct(x, h, up, down, offset, ms):
    """The formula as a direct float64 sum for the outputs ``ms`` (any integers >= 0) of rows x (..., L)."""
    x = np.asarray(x, dtype=np.float64)
    L, N = x.shape[-1], len(h)
    out = np.zeros(x.shape[:-1] + (len(ms),))
    for i, m in enumerate(ms):
        p = int(m) * down + offset
        k_hi = min(p // up, L - 1)
        k_lo = max(-((N - 1 - p) // up), 0)              # ceil((p - (N - 1)) / up)
        if k_hi < k_lo:
            continue
        k = np.arange(k_lo, k_hi + 1)
        out[..., i] = x[..., k] @ h[p - k * up]
    return out


def upfirdn(x, h, up, down, offset=0, n_out=None):
    """The formula for rows x (..., L) -> (..., M) float64 through scipy.signal.upfirdn: zeros in front of the taps move
    ``offset`` onto the next multiple of ``down``, and outputs beyond the last non-empty tap window are 0."""
    x = np.asarray(x, dtype=np.float64)
    L, N = x.shape[-1], len(h)
    M = default_n_out(L, N, up, down, offset) if n_out is None else n_out
    z = (-offset) % down
    full = sps.upfirdn(np.concatenate([np.zeros(z), h]), x, up, down, axis=-1)   # full[j] = w[j down - z], w = the zero-stuffed x * h
    first = (offset + z) // down
    out = np.zeros(x.shape[:-1] + (M,))
    n = max(0, min(M, full.shape[-1] - first))
    out[..., :n] = full[..., first:first + n]
    return out


def adjoint(g, h, up, down, offset, L):
    """The adjoint of x -> upfirdn(x, h, up, down, offset, M) applied to g (..., M) -> (..., L): up and down exchanged, the
    taps reversed, offset' = N - 1 - offset."""
    return upfirdn(g, h[::-1].copy(), down, up, len(h) - 1 - offset, n_out=L)


def peak(x, h, up, down, offset, n_out):
    """-> (max_m |y[m]|, the lowest m that attains it, y) per row, float64."""
    y = upfirdn(x, h, up, down, offset, n_out)
    a = np.abs(y)
    return a.max(-1), a.argmax(-1), y                     # (argmax returns the first of equal maxima)


def noise(shape, seed):
    """Unit noise, float32 -> (float64 array of the float32 values, float32 tensor)."""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    return t.double().numpy(), t


def noise_and_tone(shape, seed, cycles_per_sample=0.05, level=2.0):
    """Noise at 0.1 plus a passband tone of amplitude ``level`` (phase and amplitude differ per row)."""
    gen = torch.Generator().manual_seed(seed)
    n = torch.arange(shape[-1], dtype=torch.float64)
    lead = shape[:-1]
    phase = torch.rand(*lead, 1, generator=gen, dtype=torch.float64) * 2.0 * math.pi
    amp = level * (0.5 + torch.rand(*lead, 1, generator=gen, dtype=torch.float64))
    t = (amp * torch.sin(2.0 * math.pi * cycles_per_sample * n + phase)
         + 0.1 * torch.randn(*shape, generator=gen, dtype=torch.float64)).float()
    return t.double().numpy(), t


KINDS = {"noise": noise, "tone": noise_and_tone}
