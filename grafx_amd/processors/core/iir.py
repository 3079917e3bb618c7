"""Biquad-cascade IIR filter (mirrors grafx.processors.core.iir.IIRFilter —
reference core/iir.py:25-276): the frequency-sampling ("fsm") backend and the exact recursive backends
("lfilter", "ssm") on HIP."""
import torch
import torch.nn as nn

from ... import autograd as diff
from ... import ops
from ...autograd import needs_grad
from ._buffer_io import StreamIO, write_rows
from .convolution import FIRConvolution, check_state, convolve_taps


def map_signal(fn, result):
    """``fn`` on the signal of a result that is ``y`` or, from a block-wise call, ``(y, carry)``."""
    return (fn(result[0]), *result[1:]) if isinstance(result, tuple) else fn(result)


class BiquadStream(StreamIO):
    """The block protocol of a processor whose ``forward(x, **params, **block)`` hands the block-wise keywords on to its
    ``self.biquad``: the carry is the input history on the "fsm" backend, the recursion's state on "lfilter" / "ssm"."""

    def stream_block(self, x4, out4, carry, **params):
        key = "history" if self.biquad.backend == "fsm" else "state"
        y, carry = self.forward(x4.reshape(-1, *x4.shape[2:]), **params, **{key: carry, "return_" + key: True})
        write_rows(out4, y)
        return carry


class IIRFilter(nn.Module):
    def __init__(self, order=2, backend="fsm", flashfftconv=True, fsm_fir_len=4000,
                 fsm_max_input_len=2**17, fsm_regularization=False):
        super().__init__()
        self.backend = backend
        self.fsm_fir_len = fsm_fir_len
        self.fsm_regularization = fsm_regularization
        self.flashfftconv = False  # resolved as upstream resolves it without FlashFFTConv (FIRConvolution below warns)
        if flashfftconv:  # same precondition as upstream (iir.py:110-112)
            assert fsm_fir_len % 2 == 0
            assert fsm_max_input_len % 2 == 0
        self.order = order
        if backend == "fsm":
            # order != 2 (no processor of the package uses it): the sampled response is formed by torch ops on the GPU, as
            # upstream (iir.py:147-150 with delays = arange(order + 1)); the taps then take the native convolution
            if fsm_regularization:
                assert False  # upstream: iir.py:122-123
            self.conv = FIRConvolution(mode="causal", flashfftconv=flashfftconv, max_input_len=fsm_max_input_len)
            self.flashfftconv = self.conv.flashfftconv
            self._plans = {}
        elif backend in ("lfilter", "ssm"):
            # upstream: torchaudio.functional.lfilter per section / a state-space form on torchlpc (iir.py:154-261).
            # Here both are the exact recursive cascade as one parallel-scan HIP kernel (gfx_biquad_cascade_f32; with the
            # filter state carried across calls: gfx_biquad_cascade_state_f32).
            # (first-order sections ride on it with a zero third coefficient; upstream's "ssm" asserts order 2, iir.py:226)
            if order not in (1, 2) or (order == 1 and backend == "ssm"):
                raise NotImplementedError("the HIP recursive kernel runs first- and second-order sections (order 1 or 2; "
                                          "backend='ssm': 2, as upstream); use backend='fsm' for higher orders")
        else:
            raise ValueError(f"Unsupported backend: {backend}")

    def _plan(self, device):
        return ops.built_once(self._plans, (device.type, device.index), lambda: ops.iir_fsm_plan(self.fsm_fir_len, device),
                              device, f"IIRFilter(fsm_fir_len={self.fsm_fir_len}): the taps' plan")

    FSM_NATIVE_MAX = 4096  # the Bluestein inverse DFT runs on one 8192-point LDS tile: 2N - 1 <= 8192

    def _taps(self, Bs, As):
        """(R,Cf,K,3) coefficients -> (R*Cf, N) frequency-sampled taps (iir.py:148-150): the native response +
        Bluestein kernel up to 4096 taps and the tile's own inverse transform at 8192 / 16384; other lengths: the same
        response formula as torch ops on the GPU (complex64 as upstream), inverted by the direct-sum kernel up to 8192
        taps and by the FFT library in float64 beyond."""
        N = self.fsm_fir_len
        if Bs.shape[-1] == 3 and ops.iir_fsm_native(N):  # 1..4096 (Bluestein on the LDS tile), 8192 and 16384 (tile inverse)
            return ops.iir_fsm_fir(Bs, As, N, self._plan(Bs.device))
        k = torch.arange(N // 2 + 1, device=Bs.device)
        d = torch.arange(Bs.shape[-1], device=Bs.device)
        delays = torch.exp(-1j * ((d[:, None] * k[None, :]).to(Bs.dtype) / N * 2 * torch.pi))
        resp = ((Bs.unsqueeze(-1) * delays).sum(-2) / (As.unsqueeze(-1) * delays).sum(-2)).prod(-2)
        if N <= ops.IRDFT_MAX_N and resp.dtype == torch.complex64:   # any length up to 8192: direct-sum kernel, no FFT library
            return ops.irdft(resp.contiguous(), N).reshape(-1, N)
        if resp.is_cuda:
            ops.fft_library_reached(f"IIRFilter(fsm_fir_len={N}): the taps' inverse real DFT")
        return torch.fft.irfft(resp.to(torch.complex128), dim=-1, n=N).float().reshape(-1, N)

    def fsm_fir(self, Bs, As):
        """(R,Cf,K,3) coefficients -> (R,Cf,N) FIR the FSM backend convolves with (iir.py:148-150)."""
        R, Cf = Bs.shape[0], Bs.shape[1]
        return self._taps(Bs, As).view(R, Cf, self.fsm_fir_len)

    # the two static helpers of the reference class (core/iir.py:263-276), for code that builds responses by hand
    @staticmethod
    def delay(delay_length, fir_length):
        """exp(-j 2 pi d k / N) for every delay d in ``delay_length`` and k = 0..N//2 (a trailing frequency axis)."""
        k = torch.arange(fir_length // 2 + 1, device=delay_length.device)
        k = k.reshape((1,) * delay_length.ndim + (-1,))
        return torch.exp(-1j * (delay_length.unsqueeze(-1) * k / fir_length * 2 * torch.pi))

    @staticmethod
    def iir_fsm(Bs, As, delays, eps=1e-10):
        """Sampled response of every section: sum_d B_d D_d / sum_d A_d D_d (``eps`` is accepted and unused upstream)."""
        return (Bs.unsqueeze(-1) * delays).sum(-2) / (As.unsqueeze(-1) * delays).sum(-2)

    def _process_recursive(self, input_signal, Bs, As, out=None, state=None, return_state=False):
        first_order = Bs.shape[-1] == 2 and As.shape[-1] == 2
        if first_order:     # first-order sections: b2 = a2 = 0 (differentiable: a zero pad)
            Bs, As = torch.nn.functional.pad(Bs, (0, 1)), torch.nn.functional.pad(As, (0, 1))
        stateful = state is not None or return_state
        lead = input_signal.shape[:2] if input_signal.ndim == 4 else None     # a (B, n, C, L) view: rows are B * n
        if state is not None and lead is not None and state.ndim == 5:
            state = state.reshape(-1, *state.shape[2:])
        if needs_grad(input_signal, Bs, As, state):
            x3 = input_signal.reshape(-1, *input_signal.shape[-2:]) if lead is not None else input_signal
            if stateful:
                y, zf = self._stateful_differentiable(x3, Bs, As, state)
            elif self.backend == "ssm" and Bs.shape[2] > 1:
                y = self._ssm_quirk_differentiable(x3, Bs, As)
            else:
                y = diff.BiquadCascadeFn.apply(x3, Bs, As)   # native recursion both ways (autograd.BiquadCascadeFn)
            if lead is not None:
                y = y.view(*lead, *y.shape[1:])
            if out is not None:
                out.copy_(y.view(out.shape))
                y = out
        else:
            if self.backend == "ssm":
                assert Bs.shape[-1] == As.shape[-1] == 3, "The filter order must be 2."
            # "ssm" with K > 1: upstream drives every section's recursion with the original input (iir.py:226-246)
            if not stateful:
                return ops.biquad_cascade(input_signal, Bs, As, ssm_quirk=self.backend == "ssm", out=out)
            y, zf = ops.biquad_cascade(input_signal, Bs, As, ssm_quirk=self.backend == "ssm", out=out, zi=state,
                                       return_state=True)
        if not return_state:
            return y
        if first_order:     # a first-order section has one state value: w[n-2] is read by nothing (a2 = b2 = 0)
            zf = zf * torch.arange(1, -1, -1, dtype=zf.dtype, device=zf.device)   # (1, 0), made on the device
        return y, (zf.view(*lead, *zf.shape[1:]) if lead is not None else zf)

    def _stateful_differentiable(self, x, Bs, As, state):
        """(y, zf) with gradients (autograd.BiquadCascadeStateFn); "ssm" with K > 1 as in _ssm_quirk_differentiable below,
        every section's recursion (and so its state) driven by the original input."""
        R, Cout, K = x.shape[0], max(x.shape[1], Bs.shape[1]), Bs.shape[2]
        if state is None:
            state = torch.zeros((R, Cout, K, 2), dtype=x.dtype, device=x.device)
        elif tuple(state.shape) != (R, Cout, K, 2) or state.dtype != torch.float32:
            raise ValueError(f"state: expected a float32 tensor of shape {(R, Cout, K, 2)}, got {state.dtype} "
                             f"{tuple(state.shape)}")
        if self.backend != "ssm" or K == 1:
            return diff.BiquadCascadeStateFn.apply(x, Bs, As, state)
        a0 = As[..., :1]
        Bn, a12 = Bs / a0, As[..., 1:] / a0
        b0 = Bn[..., :1]
        b12 = Bn[..., 1:] - b0 * a12
        one, zero = torch.ones_like(b0[:, :, 0]), torch.zeros_like(b0[:, :, 0])
        y, zfs = x, []
        for k in range(K):
            Bk = torch.cat([zero, b12[:, :, k]], -1).unsqueeze(2)
            Ak = torch.cat([one, a12[:, :, k]], -1).unsqueeze(2)
            d, zf = diff.BiquadCascadeStateFn.apply(x, Bk, Ak, state[:, :, k : k + 1])
            y = b0[:, :, k] * y + d
            zfs.append(zf)
        return y, torch.cat(zfs, 2)

    @staticmethod
    def _ssm_quirk_differentiable(x, Bs, As):
        """Upstream's "ssm" with K > 1 sections (core/iir.py:186-260) is not a cascade: every section's RECURSION is driven by
        the ORIGINAL input and only its direct term b0 by the previous section's output,
            y_k = b0_k y_{k-1} + z^-1 (b12_k / A_k) x,      b12 = b[1:] / a0 - b0 a[1:] / a0,  b0 = b[0] / a0,
        i.e. K parallel one-section filters of the input folded with the direct gains.  Spelled out like that it is K native
        single-section recursions (autograd.BiquadCascadeFn: native backward) and a few products -- the same values as the
        forward-only kernel path (gfx_biquad_cascade_f32 with ssm_quirk), with gradients (round 6: this used to raise)."""
        a0 = As[..., :1]
        Bn, a12 = Bs / a0, As[..., 1:] / a0
        b0 = Bn[..., :1]                                   # (R, Cf, K, 1)
        b12 = Bn[..., 1:] - b0 * a12                       # (R, Cf, K, 2)
        one, zero = torch.ones_like(b0[:, :, 0]), torch.zeros_like(b0[:, :, 0])
        y = x
        for k in range(Bs.shape[2]):
            Bk = torch.cat([zero, b12[:, :, k]], -1).unsqueeze(2)          # z^-1 (b12_0 + b12_1 z^-1)
            Ak = torch.cat([one, a12[:, :, k]], -1).unsqueeze(2)
            y = b0[:, :, k] * y + diff.BiquadCascadeFn.apply(x, Bk, Ak)
        return y

    def _process_fsm_block(self, x, Bs, As, out, tee, shared_rows, final, history, return_history):
        """One block of a stream on the frequency-sampled backend: the same taps, the stateful causal convolution."""
        N = self.fsm_fir_len
        if tee is not None:
            tee.copy_(x)
        if needs_grad(x, Bs, As, history):
            if N <= self.FSM_NATIVE_MAX and Bs.shape[-1] == 3:
                h = diff.FsmFirFn.apply(Bs, As, N, self._plan(Bs.device))
            else:
                h = diff.fsm_fir(Bs, As, N)
            y, zf = diff.convolve(x, h, "causal", final=final, state=check_state(history, x, N, "IIRFilter(backend='fsm')"),
                                  return_state=True)
            if out is not None:
                out.copy_(y.view(out.shape))
                y = out
        else:
            y, zf = convolve_taps(x, ops.fir_spectrum(self._taps(Bs, As)), N, Bs.shape[1], "causal", out=out,
                                  h_rows=shared_rows, state=history, return_state=True)
        return (y, zf) if return_history else y

    def forward(self, input_signal, Bs, As, out=None, tee=None, shared_rows=None, final=False, state=None,
                return_state=False, history=None, return_history=False):
        """``shared_rows``: Bs/As hold that many rows, shared by the batch (signal row r uses r % shared_rows).
        ``final``: the caller returns this output as its own up to linear operations (autograd.TAPE_ONLY).
        ``state`` / ``return_state`` (recursive backends): block-wise processing of a long signal.  ``state`` is the filter
        state entering this block, float32 (R, Cout, K, 2) -- (B, n, Cout, K, 2) for a (B, n, C, L) input -- with
        (w[n-1], w[n-2]) of every section's a0-normalised direct form II (first-order sections: a zero second entry); None
        is silence.  With ``return_state`` the result is ``(y, state)``, the state after the block's last sample: pass it
        to the next block's call and the blocks' outputs are the one-call output, gradients included.
        ``history`` / ``return_history`` (backend "fsm"): block-wise processing of the frequency-sampled FIR.  ``history`` is
        the last fsm_fir_len - 1 input samples before this block, float32 (R, C_in, fsm_fir_len - 1), oldest first (None:
        silence) -- the state of core.convolution.convolve, read in place; with ``return_history`` the result is
        ``(y, history)``.  A call with a history is always the causal linear convolution with the sampled taps: blocks cut
        anywhere concatenate to the linear convolution of the whole, which equals the one-call output exactly when that
        call does not alias (L_total + fsm_fir_len - 1 even) or under set_exact_convolution(True) -- the reference's
        odd-length aliasing is a property of one whole-signal transform and has no block form."""
        if self.backend == "fsm" and (state is not None or return_state):
            raise ValueError("IIRFilter(backend='fsm'): the frequency-sampled FIR carries no recursive state; use the "
                             "recursive backends (backend='lfilter' or 'ssm') for block-wise processing")
        if history is not None or return_history:
            if self.backend != "fsm":
                raise ValueError(f"IIRFilter(backend={self.backend!r}): history / return_history carry the input history of the "
                                 "frequency-sampled FIR (backend='fsm'); a recursive backend carries state / return_state")
            return self._process_fsm_block(input_signal, Bs, As, out, tee, shared_rows, final, history, return_history)
        if shared_rows is not None and self.backend != "fsm":
            rows = input_signal.shape[0] * input_signal.shape[1] if input_signal.ndim == 4 else input_signal.shape[0]
            Bs, As = Bs.repeat(rows // shared_rows, 1, 1, 1), As.repeat(rows // shared_rows, 1, 1, 1)  # no row sharing
            shared_rows = None
        if self.backend != "fsm":
            if tee is not None:
                tee.copy_(input_signal)
            return self._process_recursive(input_signal, Bs, As, out=out, state=state, return_state=return_state)
        if tee is not None and needs_grad(input_signal, Bs, As):
            tee.copy_(input_signal)
            tee = None
        if needs_grad(input_signal, Bs, As):  # training path: torch front-end + native conv fwd/bwd
            # a strided (B,n,C,L) view goes through as it is (the native convolution reads it in place)
            if self.fsm_fir_len <= self.FSM_NATIVE_MAX and Bs.shape[-1] == 3:  # native taps, written-out backward
                h = diff.FsmFirFn.apply(Bs, As, self.fsm_fir_len, self._plan(Bs.device))
            else:
                h = diff.fsm_fir(Bs, As, self.fsm_fir_len)
            y = diff.convolve(input_signal, h, "causal", exact=self.flashfftconv, final=final)
            if out is None:
                return y
            out.copy_(y.view(out.shape))
            return out
        R, Cf = Bs.shape[0], Bs.shape[1]
        N = self.fsm_fir_len
        h = self._taps(Bs, As)
        return convolve_taps(input_signal, ops.fir_spectrum(h), N, Cf, "causal", out=out, tee=tee, exact=self.flashfftconv,
                             h_rows=shared_rows)
