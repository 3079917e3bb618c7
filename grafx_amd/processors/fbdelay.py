"""A feedback delay: an echo that repeats and decays, with damping in the loop, straight or ping-pong between the channels
(an extension of this project: upstream grafx has none).

Per row r and channels c, c':

    i_c = floor(delay[r,c]), f_c = delay[r,c] - i_c                      samples, 64 <= delay <= max_delay
    s_c[n] = (1 - f_c) w_c[n - i_c] + f_c w_c[n - i_c - 1]               the line's output, linear interpolation
    q_c[n] = (1 - a[r,c]) s_c[n] + a[r,c] q_c[n - 1]                     the loop's one-pole damping
    w_c[n] = x_c[n] + sum_c' F[r,c,c'] q_c'[n]                           what enters the line
    y_c[n] = dry[r] x_c[n] + wet[r] q_c[n]

One recursive HIP chunk walk forward (`gfx_fbdelay_f32`) and one backward call (`gfx_fbdelay_bwd_f32`) behind
`autograd.FeedbackDelayFn`; the tape is ``x``, the parameters and the two signals q and w.  The formula stays available as
torch ops in ``torch_forward`` (any device, any dtype)."""
import torch
import torch.nn as nn

from .. import ops
from ..autograd import FeedbackDelayFn, needs_grad
from .core._buffer_io import FusedStateIO, refuse_state_under_grad, write_rows


def _onepole_matrix(a, K):
    """(R, C, K, K): the lower-triangular Toeplitz matrix of the one-pole (1 - a) / (1 - a z^-1) over K samples, and
    (R, C, K): a^(k + 1), what the value before the chunk contributes."""
    k = torch.arange(K, device=a.device)
    # a^0 .. a^K as a running product: its derivative is finite at a = 0, where pow's is not
    pw = torch.cumprod(torch.cat([torch.ones_like(a)[..., None], a[..., None].expand(*a.shape, K)], -1), -1)
    tri = (k[:, None] >= k[None, :]).to(a.dtype)
    T = (1 - a)[..., None, None] * pw[..., (k[:, None] - k[None, :]).clamp_min(0)] * tri
    return T, pw[..., 1:]


def fbdelay_torch(x, delay, damping, feedback, dry, wet, max_delay, state=None, chunk=None):
    """ops.fbdelay as torch ops on any device and dtype, differentiable in x and the five physical parameters: the row is
    walked in chunks of min(floor(delay)) samples (at most ``chunk``, by default ops.FBDELAY_CHUNK, of them), inside which the line's output depends on
    earlier chunks only and the one-pole is a lower-triangular Toeplitz product -> (y, (history, q_last))."""
    S = max_delay + 1
    C, L = x.shape[-2:]
    shape, x = x.shape, x.reshape(-1, C, L)
    R = x.shape[0]
    delay, a = delay.reshape(R, C).to(x.dtype), damping.reshape(R, C).to(x.dtype)
    F = feedback.reshape(R, C, C).to(x.dtype)
    if state is None:
        hist, q_last = x.new_zeros(R, C, S), x.new_zeros(R, C)
    else:
        hist, q_last = state[0].reshape(R, C, S).to(x.dtype), state[1].reshape(R, C).to(x.dtype)
    i = delay.detach().floor()
    f = (delay - i)[..., None]
    i = i.long()
    imin, imax = int(i.min()), int(i.max())
    K = max(1, min(imin, chunk or ops.FBDELAY_CHUNK, L))       # (the Toeplitz matrix is quadratic in K)
    T, apow = _onepole_matrix(a, K)
    ws, qs = [], []                                            # the chunks of w; sample k sits at position k + S behind hist
    for n0 in range(0, L, K):
        Kc = min(K, L - n0)
        lo, hi = S + n0 - imax - 1, S + n0 + Kc - imin         # the positions this chunk can read: earlier chunks only
        first, last = max(0, (lo - S) // K), max(-1, (hi - 1 - S) // K)
        start = 0 if lo < S else S + first * K
        window = torch.cat(([hist] if lo < S else []) + ws[first:last + 1], -1)[..., lo - start:hi - start]
        base = (S + n0 - lo + torch.arange(Kc, device=x.device)) - i[..., None]         # (R, C, Kc): where w[n - i] sits
        s = (1 - f) * window.gather(-1, base) + f * window.gather(-1, base - 1)
        q = (T[..., :Kc, :Kc] @ s[..., None])[..., 0] + apow[..., :Kc] * q_last[..., None]
        q_last = q[..., -1]
        ws.append(x[..., n0:n0 + Kc] + (F @ q))
        qs.append(q)
    w, q = torch.cat(ws, -1), torch.cat(qs, -1)
    y = dry.reshape(R, 1, 1).to(x.dtype) * x + wet.reshape(R, 1, 1).to(x.dtype) * q
    after = torch.cat([hist, w], -1)[..., L:L + S].detach().contiguous()
    return y.reshape(shape), (after, q_last.detach().contiguous())


class FeedbackDelay(FusedStateIO, nn.Module):
    """A delay of ``min_delay`` .. ``max_delay`` samples per channel (64 <= min_delay < max_delay <= 65536) inside a
    feedback loop of gain up to ``max_feedback`` with a one-pole low-pass of coefficient up to ``max_damping``;
    ``processor_channel``: "mono" (C = 1) or "stereo" (C = 2: each channel its own delay and damping, and ``z_cross``
    moves the feedback from straight to ping-pong).  Parameters per row: ``z_delay`` (C), ``z_feedback`` (1), ``z_cross``
    (1, stereo only), ``z_damping`` (C), ``log_wet`` (1), ``log_dry`` (1); :meth:`physical` maps them so that the loop
    gain stays below ``max_feedback`` < 1."""

    accepts_strided_rows = True   # forward() also takes a strided (B, n, C, L) view (under grad it then returns (B, n, C, L))
    latency = 0

    def __init__(self, min_delay=64, max_delay=22050, max_feedback=0.95, max_damping=0.95, processor_channel="stereo"):
        super().__init__()
        for name, v, lo in (("min_delay", min_delay, ops.FBDELAY_MIN_DELAY), ("max_delay", max_delay, ops.FBDELAY_MIN_DELAY + 1)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"FeedbackDelay: {name}={v!r} must be an integer >= {lo}")
        if max_delay > ops.FBDELAY_MAX_DELAY:
            raise ValueError(f"FeedbackDelay: max_delay={max_delay} samples, the delay line holds {ops.FBDELAY_MAX_DELAY} at most")
        if min_delay >= max_delay:
            raise ValueError(f"FeedbackDelay: min_delay={min_delay} must lie below max_delay={max_delay}")
        if processor_channel not in ("mono", "stereo"):
            raise ValueError(f"FeedbackDelay: processor_channel={processor_channel!r} must be 'mono' or 'stereo'")
        for name, v in (("max_feedback", max_feedback), ("max_damping", max_damping)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < v < 1:
                raise ValueError(f"FeedbackDelay: {name}={v!r} must be a number inside (0, 1)")
        self.min_delay, self.max_delay = min_delay, max_delay
        self.max_feedback, self.max_damping = float(max_feedback), float(max_damping)
        self.processor_channel = processor_channel
        self.num_channels = 1 if processor_channel == "mono" else 2

    @property
    def state_samples(self):
        """Samples of the line a state carries: max_delay + 1."""
        return self.max_delay + 1

    def stream_check(self):
        """Every configuration renders in blocks."""

    def parameter_size(self):
        C = self.num_channels
        size = {"z_delay": C, "z_feedback": 1, "z_cross": 1, "z_damping": C, "log_wet": 1, "log_dry": 1}
        if C == 1:
            del size["z_cross"]
        return size

    def physical(self, z_delay, z_feedback, z_cross=None, z_damping=None, log_wet=None, log_dry=None):
        """The kernel's parameters from the module's, in torch ops (autograd carries the chain) -> (delay, damping (R, C),
        feedback (R, C, C), dry, wet (R,)): the delay in [min_delay, max_delay], fb = max_feedback sigmoid(z_feedback),
        F = fb [[1 - cross, cross], [cross, 1 - cross]] with cross = sigmoid(z_cross) (mono: F = fb), so that every row sum
        of |F| is fb <= max_feedback < 1; the damping in [0, max_damping]."""
        C = self.num_channels
        R = z_delay.numel() // C
        lo, hi = float(self.min_delay), float(self.max_delay)
        delay = lo + (hi - lo) * torch.sigmoid(z_delay.reshape(R, C))
        fb = self.max_feedback * torch.sigmoid(z_feedback.reshape(R, 1, 1))
        if C == 1:
            feedback = fb
        else:
            cross = torch.sigmoid(z_cross.reshape(R, 1, 1))
            eye = torch.eye(2, dtype=fb.dtype, device=fb.device)
            feedback = fb * ((1 - cross) * eye + cross * (1 - eye))
        damping = self.max_damping * torch.sigmoid(z_damping.reshape(R, C))
        return delay, damping, feedback, torch.exp(log_dry.reshape(R)), torch.exp(log_wet.reshape(R))

    def _z(self, z_delay, z_feedback, z_cross, z_damping, log_wet, log_dry):
        if (z_cross is None) != (self.num_channels == 1) or z_damping is None or log_wet is None or log_dry is None:
            raise ValueError(f"FeedbackDelay: processor_channel={self.processor_channel!r} takes the parameters "
                             f"{list(self.parameter_size())}")
        return z_delay, z_feedback, z_cross, z_damping, log_wet, log_dry

    def forward(self, input_signals, z_delay, z_feedback, z_cross=None, z_damping=None, log_wet=None, log_dry=None, state=None,
                return_state=False, _out=None):
        """(B, C, L) / (R, C, L) signals, or a strided (B, n, C, L) view, and the parameters of ``parameter_size()`` per row
        (by keyword: "mono" has no ``z_cross``).
        ``state`` / ``return_state``: block-wise processing: the pair (the last max_delay + 1 samples that entered the line,
        contiguous (R, C, .), oldest first; the loop filter's last value (R, C)) (None: silence); treat it as opaque.
        Blocks cut anywhere concatenate to the one-call output to rounding (the walk restarts at each block); ``(y, state)``
        comes back when a state is asked for."""
        if input_signals.shape[-2] != self.num_channels:
            raise ValueError(f"FeedbackDelay: {input_signals.shape[-2]} channels for processor_channel="
                             f"{self.processor_channel!r}")
        z = self._z(z_delay, z_feedback, z_cross, z_damping, log_wet, log_dry)
        if needs_grad(input_signals, *z):
            refuse_state_under_grad("FeedbackDelay", state)
            params = self.physical(*z)
            y = FeedbackDelayFn.apply(input_signals, *params, self.max_delay)
            y = y if _out is None else write_rows(_out, y)
            if not return_state:
                return y
            with torch.no_grad():                  # (the state a first block leaves: a second walk, outside the tape)
                return y, ops.fbdelay(input_signals.detach(), *(p.detach() for p in params), self.max_delay, return_state=True)[1]
        with torch.no_grad():
            params = self.physical(*z)
        if state is None and not return_state:
            return ops.fbdelay(input_signals, *params, self.max_delay, out=_out)
        return ops.fbdelay(input_signals, *params, self.max_delay, out=_out, state=state, return_state=True)

    def torch_forward(self, input_signals, z_delay, z_feedback, z_cross=None, z_damping=None, log_wet=None, log_dry=None,
                      state=None, return_state=False):
        """forward() as torch ops: the same definition on any device and dtype, differentiable."""
        params = self.physical(*self._z(z_delay, z_feedback, z_cross, z_damping, log_wet, log_dry))
        y, after = fbdelay_torch(input_signals, *params, self.max_delay, state, chunk=ops.FBDELAY_CHUNK)
        return (y, after) if return_state or state is not None else y
