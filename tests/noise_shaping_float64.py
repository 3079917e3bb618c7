"""Float64 reference of the filtered-noise-shaping taps on the CPU, shared by the tests of the native impulse-response
backward: the formula of reverb.py:343-366 on the module's float32 band-split noise,

    ir[r,c,t] = sum_k noise[c,k,t] gain[r,c,k] (exp(t d) - fg exp(t f)),
    d = sigmoid(log_decay) (max - min) + min,  f = sigmoid(log_fade_in) (d - min) + min,  fg = sigmoid(z_fade_in_gain)

(the gain is the raw parameter), then normalize_impulse, mid/side and the reference's FFT convolution, differentiated by
autograd."""
import torch


def taps64(noise, log_decay, log_gain, log_fade_in, z_fade_in_gain, min_decay, max_decay, normalise):
    """noise: (C, K, T) float32 (a window of the buffer); parameters (R, C, K) float64 (fade pair: both or None) -> (R, C, T)."""
    t = torch.arange(noise.shape[-1], dtype=torch.float64)
    d = torch.sigmoid(log_decay) * (max_decay - min_decay) + min_decay
    env = torch.exp(t * d[..., None])
    if log_fade_in is not None:
        f = torch.sigmoid(log_fade_in) * (d - min_decay) + min_decay
        env = env - torch.sigmoid(z_fade_in_gain)[..., None] * torch.exp(t * f[..., None])
    ir = (noise.detach().cpu().double()[None] * (log_gain[..., None] * env)).sum(2)
    if normalise:
        ir = ir * torch.rsqrt(ir.square().sum(-1, keepdim=True).mean(-2, keepdim=True) + 1e-12)
    return ir


def tap_gradients64(noise, params, gh, min_decay, max_decay, normalise):
    """params: {name: (R, C, K) tensor} in the order log_decay, log_gain[, log_fade_in, z_fade_in_gain]; -> {name: gradient
    of sum(gh * taps)}, float64 on the CPU."""
    leaves = {k: v.detach().cpu().double().requires_grad_() for k, v in params.items()}
    h = taps64(noise, leaves["log_decay"], leaves["log_gain"], leaves.get("log_fade_in"), leaves.get("z_fade_in_gain"),
               min_decay, max_decay, normalise)
    return dict(zip(leaves, torch.autograd.grad((h * gh.detach().cpu().double()).sum(), list(leaves.values()))))


def _sum_difference(x):
    return torch.stack([x[..., 0, :] + x[..., 1, :], x[..., 0, :] - x[..., 1, :]], -2)


def causal_convolve64(x, h, exact):
    """The reference's convolve(mode="causal"): real FFTs of P = L + N - 1 points, the inverse at its default length (P - 1
    samples when P is odd: the aliasing), the first L samples.  ``exact``: the linear convolution whatever the parity."""
    L, P = x.shape[-1], x.shape[-1] + h.shape[-1] - 1
    spec = torch.fft.rfft(x, n=P) * torch.fft.rfft(h, n=P)
    return (torch.fft.irfft(spec, n=P) if exact or P % 2 == 0 else torch.fft.irfft(spec))[..., :L]


def reverb64(x, noise, log_decay, log_gain, log_fade_in, z_fade_in_gain, min_decay, max_decay, channel, exact=False):
    """FilteredNoiseShapingReverb.forward in float64: normalised taps, mid/side around the convolution in "midside" mode."""
    h = taps64(noise, log_decay, log_gain, log_fade_in, z_fade_in_gain, min_decay, max_decay, True)
    if channel == "midside":
        return _sum_difference(causal_convolve64(0.5 * _sum_difference(x), h, exact))
    return causal_convolve64(x, h, exact)
