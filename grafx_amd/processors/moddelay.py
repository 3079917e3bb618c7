"""A modulated delay line: chorus, vibrato, doubling, a flanger without feedback (an extension of this project: upstream
grafx has none).

Per row r, channel c and voice v, at the absolute position p of sample n:

    theta = rate[r,v] p + phase[r,v,c]                                  cycles; in double, reduced mod 1
    d     = clamp(delay[r,v] + depth[r,v] sin(2 pi theta), 1, max_delay)     samples; in double
    i = floor(d), f = d - i
    u[v,c,n] = sum_j l_j(f) x[c, n - i - j]                             linear (j = 0, 1) or third-order Lagrange (j = -1 .. 2)
    y[c,n]   = dry[r] x[c,n] + sum_v gain[r,v,c] u[v,c,n]

One fused HIP tile kernel forward (`gfx_moddelay_f32`) and one backward call (`gfx_moddelay_bwd_f32`) behind
`autograd.ModulatedDelayFn`; the tape is ``x`` and the parameters.  The formula stays available as torch ops in
``torch_forward`` (any device, any dtype; the delay always in float64)."""
import math

import torch
import torch.nn as nn

from .. import ops
from ..autograd import ModulatedDelayFn, needs_grad
from .core._buffer_io import FusedStateIO, history_after, refuse_state_under_grad, write_rows

# the part of the kernel's slope contract 2 pi rate depth <= 1/2 that the mapping uses: float32 rounding stays inside it
_SLOPE = 0.45


def _lagrange(f, interp):
    """[(j, l_j(f))] of the interpolation."""
    if interp == "linear":
        return [(0, 1 - f), (1, f)]
    return [(-1, -f * (f - 1) * (f - 2) / 6), (0, (f + 1) * (f - 1) * (f - 2) / 2), (1, -(f + 1) * f * (f - 2) / 2),
            (2, (f + 1) * f * (f - 1) / 6)]


def moddelay_torch(x, delay, depth, rate, phase, gain, dry, max_delay, interp="cubic", state=None):
    """ops.moddelay as torch ops on any device and dtype, differentiable in x and the six physical parameters; the delay is
    always evaluated in float64 (a delay of 4000 samples has a float32 ulp of 2.4e-4 samples) -> (y, (history, position))."""
    Dmax, S = max_delay, max_delay + 2
    C, L = x.shape[-2:]
    shape, x = x.shape, x.reshape(-1, C, L)
    R, V = x.shape[0], delay.shape[-1]
    if state is None:
        zi, pos = x.new_zeros(R, C, S), torch.zeros(R, dtype=torch.int64, device=x.device)
    else:
        zi, pos = state[0].reshape(R, C, S).to(x.dtype), state[1].reshape(R)
    n = torch.arange(L, device=x.device)
    p = (pos[:, None] + n).double()[:, None, None, :]
    theta = rate.reshape(R, V).double()[:, :, None, None] * p + phase.reshape(R, V, C).double()[..., None]     # (R, V, C, L)
    theta = theta - theta.detach().floor()
    swing = depth.reshape(R, V).double()[:, :, None, None] * torch.sin(2 * math.pi * theta)
    d = (delay.reshape(R, V).double()[:, :, None, None] + swing).clamp(1, Dmax)
    i = d.detach().floor()
    f = (d - i).to(x.dtype)
    xx = torch.cat([zi, x], -1)                                                             # sample k sits at k + S
    lines = xx[:, None].expand(R, V, C, S + L)
    base = S + n - i.long()
    u = sum(w * lines.gather(-1, base - j) for j, w in _lagrange(f, interp))
    y = dry.reshape(R, 1, 1).to(x.dtype) * x + (gain.reshape(R, V, C, 1).to(x.dtype) * u).sum(1)
    return y.reshape(shape), (xx[..., L:L + S].detach().contiguous(), pos + L)


class ModulatedDelay(FusedStateIO, nn.Module):
    """``num_voices`` = V (1 .. 8) delay taps per channel, each swinging under its own sine oscillator between
    ``min_delay`` and ``max_delay`` samples (max_delay <= 8192) at up to ``max_rate`` Hz; ``interpolation``: "linear" or
    "cubic"; ``processor_channel``: "mono" (C = 1) or "stereo" (C = 2, every voice with its own phase and gain per channel).
    Parameters per row: ``z_delay``, ``z_depth``, ``z_rate`` (V), ``phase`` (V, C) in cycles, ``log_gain`` (V, C),
    ``log_dry`` (1); :meth:`physical` maps them so that the modulation's slope stays within +-45 % of a sample per sample.
    ``z_depth -> -inf`` is a static fractional delay, ``log_dry -> -inf`` a pure vibrato."""

    accepts_strided_rows = True   # forward() also takes a strided (B, n, C, L) view (under grad it then returns (B, n, C, L))
    latency = 0

    def __init__(self, num_voices=2, min_delay=16, max_delay=1764, max_rate=8.0, sample_rate=44100, interpolation="cubic",
                 processor_channel="stereo"):
        super().__init__()
        for name, v, lo in (("num_voices", num_voices, 1), ("min_delay", min_delay, 0), ("max_delay", max_delay, 2)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"ModulatedDelay: {name}={v!r} must be an integer >= {lo}")
        if num_voices > ops.MODDELAY_MAX_VOICES:
            raise ValueError(f"ModulatedDelay: num_voices={num_voices}, the kernels take {ops.MODDELAY_MAX_VOICES} at most")
        if max_delay > ops.MODDELAY_MAX_DELAY:
            raise ValueError(f"ModulatedDelay: max_delay={max_delay} samples, the delay line holds {ops.MODDELAY_MAX_DELAY} at most")
        if max(1, min_delay) >= max_delay:
            raise ValueError(f"ModulatedDelay: min_delay={min_delay} must lie below max_delay={max_delay} (the delay is at "
                             "least one sample)")
        if interpolation not in ("linear", "cubic"):
            raise ValueError(f"ModulatedDelay: interpolation={interpolation!r} must be 'linear' or 'cubic'")
        if processor_channel not in ("mono", "stereo"):
            raise ValueError(f"ModulatedDelay: processor_channel={processor_channel!r} must be 'mono' or 'stereo'")
        for name, v in (("max_rate", max_rate), ("sample_rate", sample_rate)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
                raise ValueError(f"ModulatedDelay: {name}={v!r} must be a positive number")
        self.num_voices, self.min_delay, self.max_delay = num_voices, min_delay, max_delay
        self.max_rate, self.sample_rate = float(max_rate), float(sample_rate)
        self.interpolation, self.processor_channel = interpolation, processor_channel
        self.num_channels = 1 if processor_channel == "mono" else 2

    @property
    def state_samples(self):
        """Input samples a state carries: max_delay + 2."""
        return self.max_delay + 2

    def stream_check(self):
        """Every configuration renders in blocks."""

    def parameter_size(self):
        V, C = self.num_voices, self.num_channels
        return {"z_delay": V, "z_depth": V, "z_rate": V, "phase": (V, C), "log_gain": (V, C), "log_dry": 1}

    def physical(self, z_delay, z_depth, z_rate, phase, log_gain, log_dry):
        """The kernel's parameters from the module's, in torch ops (autograd carries the chain) -> (delay, depth, rate
        (R, V), phase, gain (R, V, C), dry (R,)): the delay in [max(1, min_delay), max_delay], the rate in
        (0, max_rate / sample_rate) cycles per sample, the depth a share of what keeps delay +- depth inside the range and
        2 pi rate depth <= 0.45."""
        V, C = self.num_voices, self.num_channels
        R = z_delay.numel() // V
        lo, hi = float(max(1, self.min_delay)), float(self.max_delay)
        delay = lo + (hi - lo) * torch.sigmoid(z_delay.reshape(R, V))
        rate = (self.max_rate / self.sample_rate) * torch.sigmoid(z_rate.reshape(R, V))
        room = torch.minimum(torch.minimum(delay - lo, hi - delay), _SLOPE / (2 * math.pi * rate))
        depth = torch.sigmoid(z_depth.reshape(R, V)) * room
        return delay, depth, rate, phase.reshape(R, V, C), torch.exp(log_gain.reshape(R, V, C)), torch.exp(log_dry.reshape(R))

    def forward(self, input_signals, z_delay, z_depth, z_rate, phase, log_gain, log_dry, state=None, return_state=False,
                _out=None):
        """(B, C, L) / (R, C, L) signals, or a strided (B, n, C, L) view, and the parameters of ``parameter_size()`` per row.
        ``state`` / ``return_state``: block-wise processing: the pair (the last max_delay + 2 input samples, contiguous
        (R, C, .), oldest first; the samples rendered so far, int64 (R,) on the device) (None: silence at position 0);
        treat it as opaque.  Blocks cut anywhere concatenate to the one-call output bit for bit; ``(y, state)`` comes back
        when a state is asked for."""
        if input_signals.shape[-2] != self.num_channels:
            raise ValueError(f"ModulatedDelay: {input_signals.shape[-2]} channels for processor_channel="
                             f"{self.processor_channel!r}")
        z = (z_delay, z_depth, z_rate, phase, log_gain, log_dry)
        cfg = (self.max_delay, self.interpolation)
        if needs_grad(input_signals, *z):
            refuse_state_under_grad("ModulatedDelay", state)
            y = ModulatedDelayFn.apply(input_signals, *self.physical(*z), *cfg)
            y = y if _out is None else write_rows(_out, y)
            return (y, self._state_after(input_signals)) if return_state else y
        with torch.no_grad():
            params = self.physical(*z)
        if state is None and not return_state:
            return ops.moddelay(input_signals, *params, *cfg, out=_out)
        return ops.moddelay(input_signals, *params, *cfg, out=_out, state=state, return_state=True)

    def _state_after(self, x):
        """The state a first block leaves: its last samples behind zeros, and its length."""
        history = history_after(x, self.state_samples)
        return history, torch.full((history.shape[0],), x.shape[-1], dtype=torch.int64, device=x.device)

    def torch_forward(self, input_signals, z_delay, z_depth, z_rate, phase, log_gain, log_dry, state=None, return_state=False):
        """forward() as torch ops: the same definition on any device and dtype, the delay evaluated in float64."""
        params = self.physical(z_delay, z_depth, z_rate, phase, log_gain, log_dry)
        y, after = moddelay_torch(input_signals, *params, self.max_delay, self.interpolation, state)
        return (y, after) if return_state or state is not None else y
