"""Float64 reference of the STFT-masked-noise taps on the CPU, shared by the tests of the native impulse-response backward:
the formula of reverb.py:161-200 spelled with torch.istft(..., length=ir_len) on the module's float32 noise spectrum and
window, then ms_to_lr and normalize_impulse, differentiated by autograd."""
import torch
import torch.nn.functional as F

N_FFT, HOP = 384, 192


def taps64(noise_stft, window, init, delta, genv, ir_len, ms_to_lr, normalise, n_fft=N_FFT, hop=HOP):
    """noise_stft: (1 or R, 2, K, T) complex64; init / delta (R, 2, K), genv (R, 2, T) or None: float64 -> (R, 2, ir_len)."""
    T = 1 + ir_len // hop
    m = torch.arange(T, dtype=torch.float64).view(1, 1, 1, -1)
    logmag = init[..., None] - F.softplus(delta)[..., None] * m
    if genv is not None:
        logmag = logmag + genv[:, :, None, :]
    spec = noise_stft.cpu().to(torch.complex128) * torch.exp(logmag / 8)
    R = spec.shape[0]
    ir = torch.istft(spec.reshape(R * 2, n_fft // 2 + 1, T), n_fft=n_fft, hop_length=hop, window=window.cpu().double(),
                     length=ir_len).view(R, 2, ir_len)
    if ms_to_lr:
        ir = torch.stack([ir[:, 0] + ir[:, 1], ir[:, 0] - ir[:, 1]], 1)
    if normalise:
        ir = ir * torch.rsqrt(ir.square().sum(-1, keepdim=True).mean(-2, keepdim=True) + 1e-12)
    return ir


def tap_gradients64(noise_stft, window, init, delta, genv, gh, ir_len, ms_to_lr, normalise):
    """Gradients of sum(gh * taps) with respect to init, delta and (when given) genv, all float64 on the CPU."""
    leaves = [t.detach().cpu().double().requires_grad_() for t in (init, delta, genv) if t is not None]
    h = taps64(noise_stft, window, leaves[0], leaves[1], leaves[2] if genv is not None else None, ir_len, ms_to_lr,
               normalise)
    return torch.autograd.grad((h * gh.detach().cpu().double()).sum(), leaves)
