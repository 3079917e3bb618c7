"""Reverbs (mirrors grafx.processors.reverb.STFTMaskedNoiseReverb — reference reverb.py:15-228)."""
import numpy as np
import torch
import torch.nn as nn

import torch.nn.functional as F

from .. import autograd as diff
from .. import ops
from ..autograd import needs_grad
from .core._buffer_io import BufferIO, Prepared, StreamIO, expand_shared, shared_reps, write_rows
from .core.utils import normalize_impulse
from .core.convolution import check_state, convolve_taps, resolve_flashfftconv
from .core.midside import lr_to_ms, ms_to_lr


class STFTMaskedNoiseReverb(BufferIO, nn.Module):
    def __init__(self, ir_len=60000, processor_channel="pseudo_midside", n_fft=384, hop_length=192,
                 fixed_noise=True, gain_envelope=False, flashfftconv=True, max_input_len=2**17):
        super().__init__()
        self.ir_len, self.n_fft, self.hop_length = ir_len, n_fft, hop_length
        # upstream builds a FIRConvolution here (reverb.py:86-90), which without FlashFFTConv warns and goes native
        self.flashfftconv = resolve_flashfftconv(flashfftconv)
        self.num_frames = 1 + (ir_len // hop_length)
        self.num_bins = 1 + n_fft // 2
        self.register_buffer("window", torch.hann_window(n_fft))
        self.register_buffer("arange", torch.arange(self.num_frames).view(1, 1, 1, -1))
        self.fixed_noise = fixed_noise
        if fixed_noise:
            self.get_fixed_noise()
        self.gain_envelope = gain_envelope
        self.processor_channel = processor_channel
        if processor_channel not in ("mono", "stereo", "midside", "pseudo_midside"):
            raise ValueError(f"Invalid processor_channel: {processor_channel}")
        self._basis = {}
        self._envelope = {}  # overlap-added squared window per (device, frames), for _istft

    def get_fixed_noise(self):
        """One-time constant, built exactly like upstream (reverb.py:101-114): RandomState(0) uniform
        noise in [-1,1) -> float32 -> centred STFT.  Init-time only; the buffer then lives on the GPU."""
        noise = np.random.RandomState(0).uniform(size=(2, self.ir_len)) * 2 - 1
        noise = torch.tensor(noise).float()
        spec = torch.stft(noise, n_fft=self.n_fft, hop_length=self.hop_length, window=self.window.cpu(),
                          return_complex=True)
        self.register_buffer("noise_stft", spec[None].contiguous())

    def sample_noise(self, num_noises, device):
        """Fresh uniform noise per row and its STFT (reverb.py:116-128), drawn with the device generator."""
        noise = torch.rand(num_noises * 2, self.ir_len, device=device) * 2 - 1
        # (round 6: the frames on the direct-sum kernel gfx_stft_f32 -- this was the last FFT-library call of the reverb)
        spec = ops.stft(noise, self.window, self.hop_length)
        return spec.view(num_noises, 2, self.num_bins, self.num_frames)

    def _istft_basis(self, device):
        return ops.built_once(self._basis, (device.type, device.index), lambda: ops.istft_basis(self.window), device,
                              "STFTMaskedNoiseReverb: the inverse-STFT bases")

    def _noise(self, rows, device):
        """The noise spectra the mask shapes: the fixed one, or with fixed_noise=False (reverb.py:63, 80-82, 165) fresh
        noise for every row, its STFT on gfx_stft_f32 -- the kernels behind it are the same."""
        return self.noise_stft if self.fixed_noise else self.sample_noise(rows, device)

    def _ir_and_gain(self, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, ms_lr):
        genv = gain_env_log_magnitude if self.gain_envelope else None
        noise = self._noise(init_log_magnitude.shape[0], init_log_magnitude.device)
        return ops.stft_reverb_ir(noise, init_log_magnitude, delta_log_magnitude, genv, self.window,
                                  self._istft_basis(init_log_magnitude.device), self.ir_len, self.hop_length, ms_lr)

    def _tap_spectra(self, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, pseudo):
        """(Hs, R): the tile spectra of the R impulse responses.  normalize_impulse (core/utils.py:14-18) is folded into
        the tap -> spectrum step."""
        ir, gain = self._ir_and_gain(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, pseudo)
        R = ir.shape[0]
        return ops.fir_spectrum(ir.view(R * 2, self.ir_len), gain=gain, gain_div=2), R

    def compute_ir(self, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude=None):
        """Un-normalised mid/side impulse responses (R,2,ir_len) (reverb.py:161-187)."""
        if needs_grad(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude):
            if self._native_backward():
                return self._native_taps(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, False, False)
            return self._compute_ir_differentiable(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude)
        return self._ir_and_gain(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, False)[0]

    def compute_stft_mask(self, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude=None):
        """(R, 2, bins, frames) magnitude mask exp((H0 - softplus(Hd) m [+ G_m]) / 8) (reverb.py:189-200), torch ops."""
        logmag = init_log_magnitude[..., None] - F.softplus(delta_log_magnitude)[..., None] * self.arange
        if self.gain_envelope:
            logmag = logmag + gain_env_log_magnitude[:, :, None, :]
        return torch.exp(logmag / 8)

    def _native_backward(self):
        """Whether the taps train on the native node (autograd.StftReverbIrFn: the FFT form, n_fft = 384 with hop = 192, the
        reference's defaults).  Any other transform size keeps the torch chain of _compute_ir_differentiable under
        gradients: there is no backward kernel for the matrix-core ("gemm") schedule."""
        return self.n_fft == 384 and self.hop_length == 192

    def _native_taps(self, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, ms_lr, normalise):
        """The taps under autograd, one node: the inference kernel forward, gfx_stft_reverb_ir_bwd_f32 backward."""
        genv = gain_env_log_magnitude if self.gain_envelope else None
        noise = self._noise(init_log_magnitude.shape[0], init_log_magnitude.device)
        return diff.StftReverbIrFn.apply(init_log_magnitude, delta_log_magnitude, genv, noise, self.window,
                                         self._istft_basis(init_log_magnitude.device), self.ir_len, self.hop_length,
                                         ms_lr, normalise)

    def _training_taps(self, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, pseudo):
        """Normalised taps (R, 2, ir_len) with a gradient path to the parameters; left/right when ``pseudo``."""
        if self._native_backward():
            return self._native_taps(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, pseudo, True)
        ir = self._compute_ir_differentiable(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude)
        return normalize_impulse(ms_to_lr(ir)) if pseudo else normalize_impulse(ir)

    def _compute_ir_differentiable(self, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude=None):
        """reverb.py:161-200 with torch ops (mask, istft): the formula, and the training path of every transform size
        but the default one (see _native_backward)."""
        mask = self.compute_stft_mask(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude)
        spec = self._noise(mask.shape[0], mask.device) * mask
        R = spec.shape[0]
        return self._istft(spec.reshape(R * 2, self.num_bins, self.num_frames)).view(R, 2, self.ir_len)

    def _istft(self, spec):
        """torch.istft(center=True, length=ir_len) spelled out (windowed inverse frames, overlap-add, division by the
        overlap-added squared window, trim): same arithmetic, but without istft's host-side envelope check, so that a
        training step can be captured into a HIP graph."""
        n_fft, hop, T = self.n_fft, self.hop_length, spec.shape[-1]
        total = n_fft + hop * (T - 1)
        # the frames' inverse real DFT on the direct-sum kernels (autograd.IrdftFn; n_fft <= 8192), not the FFT library
        from .. import autograd as diff

        frames = diff.irfft_small(spec.transpose(-1, -2), n_fft) * self.window
        y = self._overlap_add(frames)
        envelope = ops.built_once(self._envelope, (spec.device.type, spec.device.index, T),
                                  lambda: self._overlap_add((self.window * self.window).expand(1, T, n_fft))[0], spec.device,
                                  "STFTMaskedNoiseReverb: the overlap-added squared window")
        a = n_fft // 2
        return y[:, a : a + self.ir_len] / envelope[a : a + self.ir_len]

    def _overlap_add(self, frames):
        """(R, T, n_fft) frames -> (R, n_fft + hop (T - 1)) with n_fft a multiple of hop: the q-th hop-sized piece of
        frame m lands in output block m + q, i.e. n_fft / hop shifted slice additions over the whole batch (F.fold
        would do the same, but its backward runs one im2col kernel per row)."""
        R, T, n_fft = frames.shape
        hop = self.hop_length
        pieces = n_fft // hop
        assert pieces * hop == n_fft
        out = frames.new_zeros(R, T + pieces - 1, hop)
        for q in range(pieces):
            out[:, q : q + T] = out[:, q : q + T] + frames[:, :, q * hop : (q + 1) * hop]
        return out.reshape(R, (T + pieces - 1) * hop)

    accepts_shared_params = True  # render_into(..., _shared_rows=n): parameters hold n rows shared by the batch
    accepts_strided_rows = True   # forward() also takes a strided (B, n, C, L) view and then returns (B, n, C, L)

    def render_into(self, x4, out4, _shared_rows=None, **params):
        if self.processor_channel == "midside":
            if _shared_rows is not None:
                params = {k: expand_shared(v, shared_reps(x4, _shared_rows)) for k, v in params.items()}
            return super().render_into(x4, out4, **params)
        return self.forward(x4, _out=out4, _shared_rows=_shared_rows, **params)

    def prepare(self, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude=None, _shared_rows=None):
        """Impulse-response synthesis + tile spectra (everything before the convolution), for the render's side stream."""
        if (not self.fixed_noise or self.processor_channel == "midside"
                or needs_grad(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude)):
            return None
        return Prepared(self._tap_spectra(init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude,
                                          self.processor_channel == "pseudo_midside")[0])

    def forward(self, input_signals, init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude=None, _out=None,
                _shared_rows=None, _prepared=None, state=None, return_state=False):
        """``state`` / ``return_state``: block-wise processing (core.convolution.convolve).  The state is the history of
        what the convolution reads, (R, 2, ir_len - 1), oldest first -- in "midside" mode the mid/side signal; treat it
        as opaque, its layout is stable.  With a state the result is the causal linear convolution, so blocks cut
        anywhere concatenate to the linear convolution of the whole: the one-call output exactly when that call does
        not alias (L_total + ir_len - 1 even) or under set_exact_convolution(True) -- the reference's odd-length
        aliasing is a property of one whole-signal transform and has no block form.  ``fixed_noise=False`` raises with
        a state: a fresh impulse response per block is not a stream.  ``(y, state)`` comes back when a state is asked
        for; the in-place ``_out`` and ``_prepared`` paths take both arguments too."""
        x, N = input_signals, self.ir_len
        block = state is not None or return_state
        if block:
            self.stream_check()  # (one call may draw its noise afresh, a chain of blocks may not)
        # what convolve_taps is told: one call follows the module's flashfftconv flag, a block is the linear convolution
        conv = {"state": state, "return_state": return_state} if block else {"exact": self.flashfftconv}
        if _prepared is not None:
            return convolve_taps(x, _prepared.tensors[0], N, 2, "causal", out=_out, h_rows=_shared_rows, **conv)
        pseudo = self.processor_channel == "pseudo_midside"
        midside = self.processor_channel == "midside"
        params = (init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude)
        if _shared_rows is not None and not self.fixed_noise:  # a noise per row: one parameter row per signal row
            # (one call only: with fixed_noise=False a block has raised above)
            params = tuple(expand_shared(t, shared_reps(x, _shared_rows)) for t in params)
            _shared_rows = None
        training = needs_grad(x, *params, state)
        if training:
            # the taps on one native node (autograd.StftReverbIrFn; other transform sizes: mask + istft as torch ops), the
            # convolution below is native either way.  The impulse responses are synthesised once per parameter row (per
            # node when the batch shares them) and the native convolution lets every batch row read them; a strided
            # (B, n, C, L) view is read in place
            h = self._training_taps(*params, pseudo)
        else:
            Hs, R = self._tap_spectra(*params, pseudo)
            if not midside:
                return convolve_taps(x, Hs, N, 2, "causal", out=_out, h_rows=_shared_rows, **conv)
        if midside:  # reverb.py:219-223; the history is the mid/side signal the convolution reads
            # one-call inference hands its input over as it comes; training and blocks flatten the rows first
            x = lr_to_ms(x.reshape(-1, *x.shape[-2:]) if training or block else x)
            if training and h.shape[0] != x.shape[0]:
                h = expand_shared(h, x.shape[0] // h.shape[0])
        zf = None
        if training and block:  # neither exact= nor final=: the stateful convolution is the linear one
            y, zf = diff.convolve(x, h, "causal", state=check_state(state, x, N, "STFTMaskedNoiseReverb"), return_state=True)
        elif training:
            y = diff.convolve(x, h, "causal", exact=self.flashfftconv, final=True)
        elif block:  # mid/side inference from here on
            y, zf = convolve_taps(x, Hs, N, 2, "causal", h_rows=_shared_rows or R, state=state, return_state=True)
        else:  # neither out= nor h_rows=: render_into routes mid/side around this path
            y = convolve_taps(x, Hs, N, 2, "causal", exact=self.flashfftconv)
        if midside:
            y = ms_to_lr(y)
        if _out is not None and (training or block):  # (one-call mid/side inference returns a new tensor even with _out)
            _out.copy_(y.view(_out.shape))
            y = _out
        return (y, zf) if return_state else y

    def stream_check(self):
        if not self.fixed_noise:
            raise ValueError("STFTMaskedNoiseReverb: fixed_noise=False draws a fresh impulse response per call, so a chain "
                             "of blocks is not a stream; state / return_state need fixed_noise=True")

    def stream_block(self, x4, out4, carry, _shared_rows=None, _prepared=None, **params):
        """The carry is the input history of the convolution (forward(state=))."""
        return self.forward(x4, _out=out4, _shared_rows=_shared_rows, _prepared=_prepared, state=carry, return_state=True,
                            **params)[1]

    def parameter_size(self):
        size = {"init_log_magnitude": (2, self.num_bins), "delta_log_magnitude": (2, self.num_bins)}
        if self.gain_envelope:
            size["gain_env_log_magnitude"] = (2, self.num_frames)
        return size


class FilteredNoiseShapingReverb(StreamIO, nn.Module):
    """Band-wise exponentially decaying filtered noise (mirrors reference reverb.py:231-401).

    Init: uniform noise split into `num_bands` bands by a Linkwitz-Riley crossover (host side, scipy).
    Forward: `gfx_noise_shaping_ir_f32` sums the K decaying bands into the impulse response (the reference
    materialises a (B, C, K, ir_len) envelope tensor for this), the response is energy-normalised and the
    HIP overlap-save convolution applies it (uniformly partitioned for the default 60 000 taps).
    Under gradients the same kernel is the forward of one autograd node whose backward is `gfx_noise_shaping_ir_bwd_f32`
    (`_taps`); `torch_compute_ir` keeps the formula as torch ops."""

    def __init__(self, ir_len=60000, num_bands=12, processor_channel="midside", f_min=31.5, f_max=15000, scale="log",
                 sr=30000, zerophase=True, order=2, noise_randomness="pseudo-random", use_fade_in=False,
                 min_decay_ms=50, max_decay_ms=2000, flashfftconv=True, max_input_len=2**17):
        super().__init__()
        from .core.convolution import FIRConvolution
        from .core.noise import get_filtered_noise

        if processor_channel not in ("midside", "stereo", "mono"):
            raise ValueError(f"Unknown channel type: {processor_channel}")
        if noise_randomness not in ("pseudo-random", "fixed"):
            if noise_randomness == "random":
                raise NotImplementedError('noise_randomness="random" is an unfinished option upstream (assert False)')
            raise ValueError(f"Invalid filtered_noise argument: {noise_randomness}")
        self.num_bands = num_bands
        self.processor_channel = processor_channel
        self.num_channels = 1 if processor_channel == "mono" else 2
        self.ir_len = ir_len
        self.noise_randomness = noise_randomness
        noise_len = ir_len if noise_randomness == "fixed" else 5 * ir_len
        noise = get_filtered_noise(noise_len, num_channels=self.num_channels, num_bands=num_bands, f_min=f_min,
                                   f_max=f_max, scale=scale, sr=sr, zerophase=zerophase, order=order)
        self.register_buffer("filtered_noise", noise.unsqueeze(0))      # (1, C, K, noise_len)
        self.conv = FIRConvolution(mode="causal", flashfftconv=flashfftconv, max_input_len=max_input_len)
        ln10_20 = np.log(10) / 20
        self.min_decay = -60 / (min_decay_ms * sr / 1000) * ln10_20      # log-amplitude slope per sample
        self.max_decay = -60 / (max_decay_ms * sr / 1000) * ln10_20
        self.use_fade_in = use_fade_in
        self.register_buffer("arange", torch.arange(ir_len)[None, None, None, :])

    def get_filtered_noise(self):
        if self.noise_randomness == "fixed":
            return self.filtered_noise
        start = int(torch.randint(0, self.filtered_noise.shape[-1] - self.ir_len, (1,)))
        return self.filtered_noise[..., start : start + self.ir_len]

    def compute_ir(self, log_decay, log_gain, log_fade_in=None, z_fade_in_gain=None):
        """Un-normalised impulse responses (R, C, ir_len) (reverb.py:343-366)."""
        return self._taps(log_decay, log_gain, log_fade_in, z_fade_in_gain, False)

    def _taps(self, log_decay, log_gain, log_fade_in, z_fade_in_gain, normalise):
        """The impulse responses on the native kernels, normalised or not.  Under gradients one node
        (autograd.NoiseShapingIrFn: the inference kernel forward, gfx_noise_shaping_ir_bwd_f32 backward, on the noise
        window this call cut); without, the inference kernel and normalize_impulse."""
        noise = self.get_filtered_noise()
        fade = (log_fade_in, z_fade_in_gain) if self.use_fade_in else (None, None)
        if needs_grad(log_decay, log_gain, *fade):
            return diff.NoiseShapingIrFn.apply(log_decay, log_gain, fade[0], fade[1], noise[0], self.ir_len,
                                               self.min_decay, self.max_decay, normalise)
        ir = ops.noise_shaping_ir(noise[0], log_decay, log_gain, fade[0], fade[1], self.ir_len, self.min_decay,
                                  self.max_decay)
        return normalize_impulse(ir) if normalise else ir

    def torch_compute_ir(self, log_decay, log_gain, log_fade_in=None, z_fade_in_gain=None):
        """reverb.py:343-366 with torch ops, the (R, C, K, ir_len) envelope tensor materialised: the formula, and the
        baseline of tools/noise_shaping_ir_bwd_bench.py.  No call of the module runs it."""
        noise = self.get_filtered_noise()
        d = torch.sigmoid(log_decay) * (self.max_decay - self.min_decay) + self.min_decay
        env = torch.exp(self.arange * d.unsqueeze(-1))
        if self.use_fade_in:
            f = torch.sigmoid(log_fade_in) * (d - self.min_decay) + self.min_decay
            env = env - torch.exp(self.arange * f.unsqueeze(-1)) * torch.sigmoid(z_fade_in_gain).unsqueeze(-1)
        return (noise * (env * log_gain.unsqueeze(-1))).sum(2)

    def forward(self, input_signals, log_decay, log_gain, log_fade_in=None, z_fade_in_gain=None, state=None,
                return_state=False):
        """``state`` / ``return_state``: block-wise processing (core.convolution.convolve).  The state is the history of
        what the convolution reads, (R, C, ir_len - 1), oldest first -- in "midside" mode the mid/side signal; treat it
        as opaque, its layout is stable.  With a state the result is the causal linear convolution, so blocks cut
        anywhere concatenate to the linear convolution of the whole (the one-call output when L_total + ir_len - 1 is
        even, or under set_exact_convolution(True)).  ``noise_randomness="pseudo-random"`` raises with a state: it cuts
        a fresh impulse response per call, and a chain of blocks is then not a stream.  ``(y, state)`` comes back when
        a state is asked for."""
        block = {} if state is None and not return_state else {"state": state, "return_state": True}
        if block:
            self.stream_check()
        ir = self._taps(log_decay, log_gain, log_fade_in, z_fade_in_gain, True)
        x = lr_to_ms(input_signals) if self.processor_channel == "midside" else input_signals
        y = self.conv(x, ir, **block)
        y, zf = y if block else (y, None)
        if self.processor_channel == "midside":
            y = ms_to_lr(y)
        return (y, zf) if return_state else y

    def stream_check(self):
        if self.noise_randomness != "fixed":
            raise ValueError('FilteredNoiseShapingReverb: noise_randomness="pseudo-random" cuts a fresh impulse response '
                             'per call, so a chain of blocks is not a stream; state / return_state need '
                             'noise_randomness="fixed"')

    def stream_block(self, x4, out4, carry, **params):
        y, carry = self.forward(x4.reshape(-1, *x4.shape[2:]), state=carry, return_state=True, **params)
        write_rows(out4, y)
        return carry

    def parameter_size(self):
        shape = (self.num_channels, self.num_bands)
        size = {"log_decay": shape, "log_gain": shape}
        if self.use_fade_in:
            size["log_fade_in"] = shape
            size["z_fade_in_gain"] = shape
        return size
