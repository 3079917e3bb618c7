"""Memoryless distortions (mirrors grafx.processors.nonlinear — reference nonlinear.py:6-309).

Inference runs one streaming HIP pass per processor (`gfx_waveshaper_f32`, plus `gfx_row_mean_f32` when
`remove_dc` is set).  When a gradient is requested the same pass runs as the forward of one autograd node
(`autograd.WaveshaperFn`) whose backward is one more streaming pass (`gfx_waveshaper_bwd_f32`): nothing full-size is kept
but the input.  Every class keeps its formula as torch ops in `torch_forward` (any device, any dtype): the float64
reference of the tests, and what the native backward is measured against.

``oversample=F`` (2..16) runs the shaper at F times the rate against aliasing: the centred signal is interpolated by
``sinc_kernel(1, F)``, shaped, and decimated by ``sinc_kernel(F, 1)`` (:func:`oversampling_filters`), in one fused tile
kernel each way (`gfx_oversampled_waveshaper_f32`, `autograd.OversampledWaveshaperFn`); the signal at the high rate
exists in LDS only.  ``oversample=1`` is the plain shaper, on the code paths above."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..autograd import OversampledWaveshaperFn, WaveshaperFn, needs_grad
from ..resample import sinc_kernel
from .core._buffer_io import FusedIO


def _center(x, remove_dc):
    return x - x.mean(-1, keepdim=True) if remove_dc else x


def oversampling_filters(factor, lowpass_filter_width=6, rolloff=0.99):
    """The filters of an oversampled distortion -> (h_up, offset_up, h_dn, offset_dn), the taps float64 on the host: the
    interpolator ``sinc_kernel(1, factor)`` and the decimator ``sinc_kernel(factor, 1)``, each centred (offset = half its
    length), each of unit gain in the passband.  With them
        u[p] = sum_k x[k] h_up[p + offset_up - k factor],    y[m] = sum_p v[p] h_dn[m factor + offset_dn - p]."""
    if isinstance(factor, bool) or not isinstance(factor, int) or not 1 <= factor <= ops.OVERSAMPLE_MAX_FACTOR:
        raise ValueError(f"oversampling_filters: factor={factor!r} must be an integer in 1..{ops.OVERSAMPLE_MAX_FACTOR}")
    h_up, _, _, offset_up = sinc_kernel(1, factor, lowpass_filter_width, rolloff)
    h_dn, _, _, offset_dn = sinc_kernel(factor, 1, lowpass_filter_width, rolloff)
    return h_up, offset_up, h_dn, offset_dn


def _interpolate(x, h, factor, offset):
    """u[..., p] = sum_k x[..., k] h[p + offset - k factor], 0 <= p < factor L, as torch ops."""
    L, N = x.shape[-1], h.numel()
    full = F.conv_transpose1d(x.reshape(-1, 1, L), h.view(1, 1, N), stride=factor)      # full[n] = sum_k x[k] h[n - k factor]
    full = F.pad(full, (0, max(0, offset + factor * L - full.shape[-1])))
    return full[..., offset:offset + factor * L].reshape(*x.shape[:-1], factor * L)


def _decimate(v, h, factor, offset):
    """y[..., m] = sum_p v[..., p] h[m factor + offset - p], 0 <= m < L = len(v) / factor, v zero outside, as torch ops."""
    FL, N = v.shape[-1], h.numel()
    L = FL // factor
    padded = F.pad(v.reshape(-1, 1, FL), (N - 1 - offset, max(0, offset + 1 - factor)))
    return F.conv1d(padded, h.flip(0).view(1, 1, N), stride=factor)[..., :L].reshape(*v.shape[:-1], L)


class _Waveshaper(FusedIO, nn.Module):
    accepts_strided_rows = True   # forward() also takes a strided (B, n, C, L) view (under grad it then returns (B, n, C, L))

    def _set_oversample(self, oversample):
        """``oversample`` = 1: nothing changes and nothing is registered; F > 1: the two filters as float32 buffers."""
        if isinstance(oversample, bool) or not isinstance(oversample, int) or not 1 <= oversample <= ops.OVERSAMPLE_MAX_FACTOR:
            raise ValueError(f"{type(self).__name__}: oversample={oversample!r} must be an integer in "
                             f"1..{ops.OVERSAMPLE_MAX_FACTOR}")
        self.oversample = oversample
        if oversample > 1:
            h_up, self.os_offset_up, h_dn, self.os_offset_dn = oversampling_filters(oversample)
            self.register_buffer("os_h_up", h_up.float(), persistent=False)
            self.register_buffer("os_h_dn", h_dn.float(), persistent=False)

    def _oversampled(self, x, pre, post, p0, p1, mode, use_tanh, inverse, out):
        """forward() of an oversampled module: the fused op, or its autograd node when a gradient is asked for."""
        filters = (self.os_h_up, self.os_offset_up, self.os_h_dn, self.os_offset_dn)
        if needs_grad(x, pre, post, p0, p1):
            return OversampledWaveshaperFn.apply(x, pre, post, p0, p1, mode, use_tanh, inverse, self.remove_dc,
                                                 self.oversample, filters)
        return ops.oversampled_waveshaper(x, mode, self.oversample, *filters, pre, post, p0=p0, p1=p1, use_tanh=use_tanh,
                                          inverse_post_gain=inverse, remove_dc=self.remove_dc, out=out)

    def _at_rate(self, u, shape):
        """``shape`` of the centred signal ``u`` at the module's rate, as torch ops: as it is, or between the interpolator
        and the decimator (the shaped signal is zero outside its factor L samples; the taps are the float32 buffers' values
        in the signal's dtype)."""
        if self.oversample == 1:
            return shape(u)
        h_up, h_dn = self.os_h_up.to(u.device, u.dtype), self.os_h_dn.to(u.device, u.dtype)
        v = shape(_interpolate(u, h_up, self.oversample, self.os_offset_up))
        return _decimate(v, h_dn, self.oversample, self.os_offset_dn)

    def stream_check(self):
        if self.oversample > 1:
            raise ValueError(f"{type(self).__name__}: oversample={self.oversample} runs an interpolator and a decimator whose "
                             "taps reach across the block's ends, and carrying their history from block to block is not "
                             "built; a chain of blocks is not a stream")
        if self.remove_dc:
            raise ValueError(f"{type(self).__name__}: remove_dc=True subtracts the mean of the whole signal, which a block "
                             "does not know; a chain of blocks is not a stream")


class TanhDistortion(_Waveshaper):
    def __init__(self, pre_post_gain=True, inverse_post_gain=True, remove_dc=False, use_bias=False, oversample=1):
        super().__init__()
        self.pre_post_gain = pre_post_gain
        self.inverse_post_gain = inverse_post_gain
        self.remove_dc = remove_dc
        self.use_bias = use_bias
        self._set_oversample(oversample)

    def forward(self, input_signals, log_pre_gain=None, log_post_gain=None, bias=None, _out=None):
        pre = log_pre_gain if self.pre_post_gain else None
        inverse = self.pre_post_gain and self.inverse_post_gain
        post = log_post_gain if (self.pre_post_gain and not self.inverse_post_gain) else None
        b = bias if self.use_bias else None
        if self.oversample > 1:
            return self._oversampled(input_signals, pre, post, b, None, ops.WS_TANH, False, inverse, _out)
        if needs_grad(input_signals, pre, post, b):
            return WaveshaperFn.apply(input_signals, pre, post, b, None, ops.WS_TANH, False, inverse, self.remove_dc)
        return ops.waveshaper(input_signals, ops.WS_TANH, pre, post, p0=b, inverse_post_gain=inverse,
                              remove_dc=self.remove_dc, out=_out)

    def torch_forward(self, input_signals, log_pre_gain=None, log_post_gain=None, bias=None):
        """forward() as torch ops."""
        pre = log_pre_gain if self.pre_post_gain else None
        inverse = self.pre_post_gain and self.inverse_post_gain
        post = log_post_gain if (self.pre_post_gain and not self.inverse_post_gain) else None
        b = bias if self.use_bias else None
        g = torch.exp(pre).unsqueeze(-1) if pre is not None else None

        def shape(u):
            u = u * g if g is not None else u
            y = torch.tanh(u + b.unsqueeze(-1)) - torch.tanh(b.unsqueeze(-1)) if b is not None else torch.tanh(u)
            if inverse:
                return y / g
            return y * torch.exp(post).unsqueeze(-1) if post is not None else y

        return self._at_rate(_center(input_signals, self.remove_dc), shape)

    def parameter_size(self):
        size = {}
        if self.pre_post_gain:
            size["log_pre_gain"] = 1
            if not self.inverse_post_gain:
                size["log_post_gain"] = 1
        if self.use_bias:
            size["bias"] = 1
        return size


class PiecewiseTanhDistortion(_Waveshaper):
    def __init__(self, pre_post_gain=True, inverse_post_gain=True, remove_dc=False, oversample=1):
        super().__init__()
        self.pre_post_gain = pre_post_gain
        self.inverse_post_gain = inverse_post_gain
        self.remove_dc = remove_dc
        self._set_oversample(oversample)

    def forward(self, input_signals, log_hardness, z_threshold, log_pre_gain=None, log_post_gain=None, _out=None):
        pre = log_pre_gain if self.pre_post_gain else None
        inverse = self.pre_post_gain and self.inverse_post_gain
        post = log_post_gain if (self.pre_post_gain and not self.inverse_post_gain) else None
        if self.oversample > 1:
            return self._oversampled(input_signals, pre, post, log_hardness, z_threshold, ops.WS_PIECEWISE, False, inverse, _out)
        if needs_grad(input_signals, log_hardness, z_threshold, pre, post):
            return WaveshaperFn.apply(input_signals, pre, post, log_hardness, z_threshold, ops.WS_PIECEWISE, False, inverse,
                                      self.remove_dc)
        return ops.waveshaper(input_signals, ops.WS_PIECEWISE, pre, post, p0=log_hardness, p1=z_threshold,
                              inverse_post_gain=inverse, remove_dc=self.remove_dc, out=_out)

    def torch_forward(self, input_signals, log_hardness, z_threshold, log_pre_gain=None, log_post_gain=None):
        """forward() as torch ops."""
        pre = log_pre_gain if self.pre_post_gain else None
        inverse = self.pre_post_gain and self.inverse_post_gain
        post = log_post_gain if (self.pre_post_gain and not self.inverse_post_gain) else None
        g = torch.exp(pre).unsqueeze(-1) if pre is not None else None

        def shape(u):
            u = u * g if g is not None else u
            y = self.apply_distortion(u, torch.exp(log_hardness), torch.sigmoid(z_threshold))
            if inverse:
                return y / g
            return y * torch.exp(post).unsqueeze(-1) if post is not None else y

        return self._at_rate(_center(input_signals, self.remove_dc), shape)

    @staticmethod
    def apply_distortion(u, hardness, threshold):
        # the (kn, kp) / (gp, gn) ordering follows upstream (nonlinear.py:163-164)
        kn, kp = threshold[..., None, 0:1], threshold[..., None, 1:2]
        gp, gn = hardness[..., None, 0:1], hardness[..., None, 1:2]
        bp, bn = torch.tanh(kp), -torch.tanh(kn)
        above, below = u > kp, u < -kn
        hi = (1 - bp) / gp * torch.tanh(gp * (u - kp)) + bp
        lo = (1 + bn) / gn * torch.tanh(gn * (u + kn)) + bn
        return torch.where(above, hi, torch.where(below, lo, torch.tanh(u)))

    def parameter_size(self):
        size = {"log_hardness": 2, "z_threshold": 2}
        if self.pre_post_gain:
            size["log_pre_gain"] = 1
            if not self.inverse_post_gain:
                size["log_post_gain"] = 1
        return size


class _PolynomialDistortion(_Waveshaper):
    mode = None

    def __init__(self, max_order=10, pre_gain=True, remove_dc=False, use_tanh=False, oversample=1):
        super().__init__()
        if not 1 <= max_order <= 32:
            raise ValueError("max_order must be in [1, 32]")
        self.pre_gain = pre_gain
        self.max_order = max_order
        self.remove_dc = remove_dc
        self.use_tanh = use_tanh
        self._set_oversample(oversample)

    def basis(self, u):
        raise NotImplementedError

    def forward(self, input_signals, basis_weights, log_pre_gain=None, _out=None):
        pre = log_pre_gain if self.pre_gain else None
        if self.oversample > 1:
            return self._oversampled(input_signals, pre, None, basis_weights, None, self.mode, self.use_tanh, False, _out)
        if needs_grad(input_signals, basis_weights, pre):
            return WaveshaperFn.apply(input_signals, pre, None, basis_weights, None, self.mode, self.use_tanh, False,
                                      self.remove_dc)
        return ops.waveshaper(input_signals, self.mode, pre, None, p0=basis_weights, use_tanh=self.use_tanh,
                              remove_dc=self.remove_dc, out=_out)

    def torch_forward(self, input_signals, basis_weights, log_pre_gain=None):
        """forward() as torch ops (materialises the K basis terms, as upstream does)."""
        pre = log_pre_gain if self.pre_gain else None

        def shape(u):
            u = u * torch.exp(pre).unsqueeze(-1) if pre is not None else u
            terms = self.basis(u)                                   # (K, R, C, L)
            terms = torch.tanh(terms) if self.use_tanh else terms
            return (terms * torch.tanh(basis_weights).T[:, :, None, None]).sum(0)

        return self._at_rate(_center(input_signals, self.remove_dc), shape)

    def parameter_size(self):
        size = {"basis_weights": self.max_order}
        if self.pre_gain:
            size["log_pre_gain"] = 1
        return size


class PowerDistortion(_PolynomialDistortion):
    mode = ops.WS_POWER

    def basis(self, u):
        k = torch.arange(self.max_order, device=u.device)[:, None, None, None]
        return torch.pow(u.unsqueeze(0), k)


class ChebyshevDistortion(_PolynomialDistortion):
    mode = ops.WS_CHEBYSHEV

    @staticmethod
    def apply_distortion(input_signals, basis_weights, use_tanh=False):
        """sum_k basis_weights[:, k] * T_k(x) (optionally tanh(T_k)) on (R, C, L) signals, weights (R, K) taken as
        they are (reference nonlinear.py:385-403), as torch ops."""
        K = basis_weights.shape[-1]
        terms = [torch.ones_like(input_signals), input_signals]
        for _ in range(2, K):
            terms.append(2 * input_signals * terms[-1] - terms[-2])
        terms = torch.stack(terms[:K], 0)
        terms = torch.tanh(terms) if use_tanh else terms
        return (terms * basis_weights.T[:, :, None, None]).sum(0)

    def basis(self, u):
        terms = [torch.ones_like(u), u]
        for _ in range(2, self.max_order):
            terms.append(2 * u * terms[-1] - terms[-2])
        return torch.stack(terms[: self.max_order], 0)
