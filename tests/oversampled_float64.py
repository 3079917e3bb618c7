"""Float64 yardstick of the oversampled waveshapers (tests/test_oversampled_abi.py, tests/test_gpu_oversampled.py): the
definition

    xc[k] = x[k] - dc                            0 <= k < L, zero outside      (dc = mean of x over time under remove_dc)
    u[p]  = sum_k xc[k] h_up[p + o_up - k F]     0 <= p < F L
    v[p]  = post s(pre u[p])                     0 <= p < F L, and zero outside
    y[m]  = sum_p v[p] h_dn[m F + o_dn - p]      0 <= m < L

as torch ops in float64, so that autograd gives every gradient; its own statement of the four shapes; the filters (the
yardstick design of upfirdn_float64, rounded to float32 as the GPU gets them); and the alias share of the issue's tone.
Not a test module."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import upfirdn_float64 as f64

TANH, PIECEWISE, POWER, CHEBYSHEV = 0, 1, 2, 3


def filters(factor, width=6, rolloff=0.99):
    """-> (h_up float32 tensor, o_up, h_dn float32 tensor, o_dn): sinc_kernel(1, factor) and sinc_kernel(factor, 1)."""
    h_up, _, _, o_up = f64.sinc_kernel(1, factor, width, rolloff)
    h_dn, _, _, o_dn = f64.sinc_kernel(factor, 1, width, rolloff)
    return f64.taps32(h_up)[1], o_up, f64.taps32(h_dn)[1], o_dn


def interpolate(x, h, factor, offset):
    """u[..., p] = sum_k x[..., k] h[p + offset - k factor], 0 <= p < factor L."""
    L, N = x.shape[-1], h.numel()
    full = F.conv_transpose1d(x.reshape(-1, 1, L), h.to(x.dtype).view(1, 1, N), stride=factor)   # full[n] = sum_k x[k] h[n - k F]
    full = F.pad(full, (0, max(0, offset + factor * L - full.shape[-1])))
    return full[..., offset:offset + factor * L].reshape(*x.shape[:-1], factor * L)


def decimate(v, h, factor, offset):
    """y[..., m] = sum_p v[..., p] h[m factor + offset - p], 0 <= m < len(v) / factor; v zero outside."""
    FL, N = v.shape[-1], h.numel()
    padded = F.pad(v.reshape(-1, 1, FL), (N - 1 - offset, max(0, offset + 1 - factor)))
    y = F.conv1d(padded, h.to(v.dtype).flip(0).view(1, 1, N), stride=factor)[..., :FL // factor]
    return y.reshape(*v.shape[:-1], FL // factor)


def shape(u, mode, p0=None, p1=None, use_tanh=False):
    """s(u) of the four modes for u (R, C, n); p0, p1 (R, k) as the C entry takes them."""
    if mode == TANH:
        return torch.tanh(u) if p0 is None else torch.tanh(u + p0[:, :, None]) - torch.tanh(p0[:, :, None])
    if mode == PIECEWISE:
        gp, gn = torch.exp(p0[:, 0])[:, None, None], torch.exp(p0[:, 1])[:, None, None]
        kn, kp = torch.sigmoid(p1[:, 0])[:, None, None], torch.sigmoid(p1[:, 1])[:, None, None]
        bp, bn = torch.tanh(kp), -torch.tanh(kn)
        hi = (1 - bp) / gp * torch.tanh(gp * (u - kp)) + bp
        lo = (1 + bn) / gn * torch.tanh(gn * (u + kn)) + bn
        return torch.where(u > kp, hi, torch.where(u < -kn, lo, torch.tanh(u)))
    K = p0.shape[1]
    if mode == POWER:
        terms = [u ** k for k in range(K)]
    else:
        terms = [torch.ones_like(u), u]
        for _ in range(2, K):
            terms.append(2 * u * terms[-1] - terms[-2])
    f = torch.tanh if use_tanh else (lambda t: t)
    return sum(torch.tanh(p0[:, k])[:, None, None] * f(terms[k]) for k in range(K))


def forward(x, mode, factor, h_up, o_up, h_dn, o_dn, log_pre_gain=None, log_post_gain=None, p0=None, p1=None, use_tanh=False,
            inverse_post_gain=False, remove_dc=False):
    """The definition for x (R, C, L) in x's dtype; parameters (R, k)."""
    xc = x - x.mean(-1, keepdim=True) if remove_dc else x
    pre = torch.exp(log_pre_gain.reshape(-1))[:, None, None] if log_pre_gain is not None else 1.0
    post = 1.0 / pre if inverse_post_gain else (torch.exp(log_post_gain.reshape(-1))[:, None, None] if log_post_gain is not None else 1.0)
    u = interpolate(xc, h_up, factor, o_up)
    v = post * shape(pre * u, mode, p0, p1, use_tanh)
    return decimate(v, h_dn, factor, o_dn)


def reference(x, gy, params, **cfg):
    """y and every gradient in float64 -> {"y", "x", parameter names}; x, gy float32 (R, C, L), params {name: float32 (R, k)}."""
    x64 = x.double().requires_grad_()
    ps64 = {k: v.double().requires_grad_() for k, v in params.items()}
    y = forward(x64, **cfg, **ps64)
    leaves = [x64, *ps64.values()]
    grads = torch.autograd.grad(y, leaves, gy.double(), allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, grads)]
    return {"y": y.detach(), "x": grads[0], **dict(zip(ps64, grads[1:]))}


# ---------------------------------------------------------------------------------------------------------------- the purpose
TONE_BIN, TONE_N, TONE_LEN = 437, 2048, 4096


def tone():
    """The issue's tone: amplitude 0.5 at 437 / 2048 of the sample rate, 4096 samples -> float32 (1, 1, 4096)."""
    n = torch.arange(TONE_LEN, dtype=torch.float64)
    return (0.5 * torch.sin(2.0 * math.pi * TONE_BIN / TONE_N * n)).float().view(1, 1, -1)


def alias_share(y):
    """The share of the energy of the middle 2048 of 4096 output samples that is not in the fundamental's bin: the tone's
    harmonics are all odd and all above Nyquist, so everything else is aliasing."""
    mid = np.asarray(y.detach().double().cpu()).reshape(-1)[TONE_LEN // 4: TONE_LEN // 4 + TONE_N]
    e = np.abs(np.fft.rfft(mid)) ** 2
    e[1:-1] *= 2.0
    return float(1.0 - e[TONE_BIN] / e.sum())


def tone_share(factor):
    """The alias share of tanh(e^3 x) / e^3 on the tone in float64, at ``factor`` times the rate (1: the plain shaper)."""
    x = tone().double()
    pre = torch.full((1, 1), 3.0, dtype=torch.float64)
    if factor == 1:
        return alias_share(torch.tanh(math.exp(3.0) * x) / math.exp(3.0))
    return alias_share(forward(x, TANH, factor, *filters(factor), log_pre_gain=pre, inverse_post_gain=True))
