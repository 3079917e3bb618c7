"""A look-ahead peak limiter (an extension of this project: upstream grafx has none).

With T = exp(log_ceiling) per row, look-ahead D, hold H, window M = D + 1 + H and N <= D + 1 smoothing taps w:

    p[k]  = max_c |x[c, k]|                      the detector, linked over the channels
    pk[q] = max_{0 <= j < M} p[q - j]            the peak ahead of the delayed signal, held for H samples
    m[q]  = T / pk[q] where pk[q] > T, else 1
    s[n]  = sum_j w[j] m[n - j]                  the gain, smoothed: attack and release ramps of N samples
    y[c, n] = x[c, n - D] s[n]                   or, with ``compensate_delay``, x[c, n] s[n + D]

Every gain under the sum was computed from a window that holds the sample it multiplies, and the taps are a convex
combination: |y| <= T up to rounding.  One fused HIP tile kernel each way (`gfx_limiter_f32`, `autograd.LimiterFn`): the
detector, the windows' maxima and the gains exist in LDS only.  The formula stays available as torch ops in
``torch_forward`` (any device, any dtype)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..autograd import LimiterFn, needs_grad
from .core._buffer_io import FusedIO, history_after, refuse_state_under_grad, write_rows


def limiter_window(lookahead):
    """The default smoothing taps of a limiter with ``lookahead`` = D samples: the N = D + 1 Hann taps
    sin^2(pi (k + 1) / (N + 1)), normalised to sum to one -> float64 on the host."""
    if isinstance(lookahead, bool) or not isinstance(lookahead, int) or not 0 <= lookahead < ops.LIMITER_MAX_TAPS:
        raise ValueError(f"limiter_window: lookahead={lookahead!r} must be an integer in 0..{ops.LIMITER_MAX_TAPS - 1} "
                         f"(the window has lookahead + 1 taps, {ops.LIMITER_MAX_TAPS} at most)")
    n = lookahead + 1
    w = torch.sin(math.pi * torch.arange(1, n + 1, dtype=torch.float64) / (n + 1)).square()
    return w / w.sum()


class Limiter(FusedIO, nn.Module):
    """``lookahead`` = D >= 0 and ``hold`` = H >= 0 samples with D + 1 + H <= 4096; ``window``: 1 .. min(D + 1, 1024)
    non-negative taps that sum to one within 1e-6 (None: ``limiter_window(lookahead)``), kept as a float32 buffer;
    ``compensate_delay``: the output is aligned with the input (x taken as zero beyond its end) instead of D samples
    late.  The only parameter is ``log_ceiling``, one value per row."""

    accepts_strided_rows = True   # forward() also takes a strided (B, n, C, L) view (under grad it then returns (B, n, C, L))

    def __init__(self, lookahead=240, hold=0, window=None, compensate_delay=True):
        super().__init__()
        for name, v in (("lookahead", lookahead), ("hold", hold)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"Limiter: {name}={v!r} must be a non-negative integer")
        if lookahead + 1 + hold > ops.LIMITER_MAX_WINDOW:
            raise ValueError(f"Limiter: lookahead + 1 + hold = {lookahead + 1 + hold} samples, the window holds "
                             f"{ops.LIMITER_MAX_WINDOW} at most")
        if window is None:
            window = limiter_window(lookahead)
        window = torch.as_tensor(window, dtype=torch.float64).detach().cpu()
        if window.ndim != 1 or not 1 <= window.numel() <= min(lookahead + 1, ops.LIMITER_MAX_TAPS):
            raise ValueError(f"Limiter: window must hold 1..{min(lookahead + 1, ops.LIMITER_MAX_TAPS)} taps in one dimension "
                             f"(lookahead + 1, {ops.LIMITER_MAX_TAPS} at most: with more the ceiling is not guaranteed), "
                             f"got {tuple(window.shape)}")
        if not bool(torch.isfinite(window).all()) or bool((window < 0).any()) or abs(float(window.sum()) - 1.0) > 1e-6:
            raise ValueError("Limiter: the window's taps must be non-negative and sum to one (a convex combination of gains "
                             "keeps the ceiling)")
        self.lookahead, self.hold, self.compensate_delay = lookahead, hold, bool(compensate_delay)
        self.register_buffer("window", window.float(), persistent=False)

    @property
    def state_samples(self):
        """Input samples a state carries: M + N - 2."""
        return self.lookahead + self.hold + self.window.numel() - 1

    @property
    def latency(self):
        """Samples the output lags the input by."""
        return 0 if self.compensate_delay else self.lookahead

    def stream_check(self):
        if self.compensate_delay:
            raise ValueError(f"Limiter: compensate_delay=True aligns the output with the input, so the last {self.lookahead} "
                             "outputs of a block would need samples the next block brings; build the module with "
                             "compensate_delay=False to render in blocks")

    def forward(self, input_signals, log_ceiling, state=None, return_state=False, _out=None):
        """(B, C, L) / (R, C, L) signals, or a strided (B, n, C, L) view, and ``log_ceiling`` (R, 1) or (R,).
        ``state`` / ``return_state``: block-wise processing (``compensate_delay=False`` only): the last
        lookahead + hold + taps - 1 input samples, contiguous (R, C, .), oldest first (None: silence); treat it as opaque.
        Blocks cut anywhere concatenate to the one-call output bit for bit; ``(y, state)`` comes back when a state is asked
        for -- ``None`` for a module without memory (lookahead = hold = 0)."""
        stateful = state is not None or return_state
        cfg = (self.lookahead, self.hold, self.compensate_delay)
        if stateful:
            self.stream_check()
            if self.state_samples == 0 and state is not None:
                raise ValueError("Limiter: lookahead = hold = 0 has no memory: there is no state to carry")
        if needs_grad(input_signals, log_ceiling):
            refuse_state_under_grad("Limiter", state)
            y = LimiterFn.apply(input_signals, log_ceiling, self.window, *cfg)
            y = y if _out is None else write_rows(_out, y)
            return (y, self._state_after(input_signals)) if return_state else y
        if not stateful or self.state_samples == 0:
            y = ops.limiter(input_signals, log_ceiling, self.window, *cfg, out=_out)
            return (y, None) if return_state else y
        return ops.limiter(input_signals, log_ceiling, self.window, *cfg, out=_out, state=state, return_state=True)

    def _state_after(self, x):
        """The state a first block leaves: its last samples behind zeros."""
        return history_after(x, self.state_samples) if self.state_samples else None

    def torch_forward(self, input_signals, log_ceiling, state=None, return_state=False):
        """forward() as torch ops."""
        D, H, N = self.lookahead, self.hold, self.window.numel()
        M, S, sigma = D + 1 + H, D + H + N - 1, D if self.compensate_delay else 0
        if state is not None or return_state:
            self.stream_check()
        C, L = input_signals.shape[-2:]
        x = input_signals.reshape(-1, C, L)
        R = x.shape[0]
        T = torch.exp(log_ceiling).reshape(R, 1)
        zi = x.new_zeros(R, C, S) if state is None else state.reshape(R, C, S).to(x.dtype)
        xx = torch.cat([zi, x, x.new_zeros(R, C, sigma)], -1)                 # sample k sits at k + S
        p = xx.abs().amax(1)
        pk = F.max_pool1d(p.unsqueeze(1), M, 1).squeeze(1) if M > 1 else p     # q from -(N - 1) on
        over = pk > T
        m = torch.where(over, T / torch.where(over, pk, torch.ones_like(pk)), torch.ones_like(pk))
        w = self.window.to(x.device, x.dtype).flip(0).view(1, 1, N)
        s = F.conv1d(m.unsqueeze(1), w).squeeze(1)                            # s[n'], 0 <= n' < L + sigma
        y = xx[..., S + sigma - D:S + sigma - D + L] * s[:, None, sigma:sigma + L]
        y = y.reshape(input_signals.shape)
        if return_state:
            return y, (xx[..., L:L + S].contiguous() if S else None)
        return y

    def stream_block(self, x4, out4, carry, **params):
        """The carry is the state of forward(state=): the input's last samples; None for a module without memory."""
        self.stream_check()
        if self.state_samples == 0:
            self.render_into(x4, out4, **params)
            return None
        return self.forward(x4, _out=out4, state=carry, return_state=True, **params)[1]

    def parameter_size(self):
        return {"log_ceiling": 1}
