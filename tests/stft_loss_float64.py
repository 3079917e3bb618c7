"""The float64 yardstick of the STFT loss (not a test module): the definition of include/grafx_amd.h's gfx_stft_loss_* and
of grafx_amd.losses.MultiResolutionSTFTLoss, written with torch.stft and autograd in float64 on the CPU, and the inputs the
tests share.  Everything is computed once per argument set and handed out unchanged."""
import functools

import torch

# n_fft, hop, L, eps: the smallest shapes at which the kernels can still go wrong
SHAPES = (
    (128, 32, 65, 0.25),        # smallest transform, L = n_fft / 2 + 1: 3 frames, every sample hit by reflections from both ends
    (128, 32, 1000, 0.25),      # L no multiple of hop, several frames per run
    (1024, 256, 1025, 2.0),     # a reflection longer than a segment may be
    (2048, 512, 6000, 4.0),     # largest transform, 12 frames
    (512, 50, 20001, 1.0),      # hop does not divide n_fft, 401 frames: several workgroups per row
    (256, 64, 4099, 1e-8),      # default eps: the sums and the gradient of A only
)
FLOORED = SHAPES[:5]
DEFAULT_EPS = SHAPES[5]
SMALL = (SHAPES[0], SHAPES[2])  # the two shapes whose independent-noise inputs are also differentiated through E and D
KINDS = ("noise", "half", "double")
# Added to a shape's seed where the draw of the plain seed comes too close to a jump of the gradient (the screening of
# tests/test_stft_loss_abi.py: at 1024/256/1025 the independent noise leaves ||T|-|P|| / mean|T| at 2.4e-5 with +0 and the
# doubled input at 8.6e-6 with +1; +2 clears every condition).
RESEED = {(1024, 256, 1025): 2}
ROWS = 3


def hann(n_fft, win_length=None, dtype=torch.float64):
    win_length = n_fft if win_length is None else win_length
    left = (n_fft - win_length) // 2
    return torch.nn.functional.pad(torch.hann_window(win_length, dtype=torch.float64),
                                   (left, n_fft - win_length - left)).to(dtype)


@functools.lru_cache(maxsize=None)
def draw(n_fft, hop, L, rows=ROWS):
    """(target, noise), float32 (rows, L), from a CPU generator seeded by the shape: the target first, then the noise."""
    g = torch.Generator().manual_seed(1000 * n_fft + hop + L + RESEED.get((n_fft, hop, L), 0))
    return torch.randn(rows, L, generator=g), torch.randn(rows, L, generator=g)


def inputs(n_fft, hop, L, kind, rows=ROWS):
    """(pred, target) float32 on the CPU.  "noise": pred independent of the target; "half" / "double":
    pred = s * target + 0.02 * noise with s = 0.5 / 2, which keeps |P| and |T| apart in every bin, with either sign."""
    target, noise = draw(n_fft, hop, L, rows)
    if kind == "noise":
        return noise.clone(), target.clone()
    return {"half": 0.5, "double": 2.0}[kind] * target + 0.02 * noise, target.clone()


def spectrum(x, n_fft, hop, window):
    return torch.stft(x, n_fft, hop, window=window, center=True, pad_mode="reflect", return_complex=True)


def magnitude(X, eps):
    return torch.sqrt(torch.clamp(X.real.square() + X.imag.square(), min=eps))


def sums_of(pred, target, n_fft, hop, window, eps):
    """(rows, 4) = (A, B, E, D) in the dtype of the inputs; differentiable."""
    P, T = magnitude(spectrum(pred, n_fft, hop, window), eps), magnitude(spectrum(target, n_fft, hop, window), eps)
    d = T - P
    return torch.stack([d.square().sum((-2, -1)), T.square().sum((-2, -1)), d.abs().sum((-2, -1)),
                        (T.log() - P.log()).abs().sum((-2, -1))], -1)


def sums_and_grad(pred, target, n_fft, hop, eps, coef=None, window=None):
    """float64 sums (rows, 4) and, with ``coef`` (rows, 3) = (cA, cE, cD), the gradient of sum_r (cA A + cE E + cD D)[r] with
    respect to pred."""
    window = hann(n_fft) if window is None else window.double()
    p = pred.double().requires_grad_(coef is not None)
    s = sums_of(p, target.double(), n_fft, hop, window, eps)
    if coef is None:
        return s.detach(), None
    (s[:, (0, 2, 3)] * coef.double()).sum().backward()
    return s.detach(), p.grad


@functools.lru_cache(maxsize=None)
def reference(n_fft, hop, L, eps, kind, coef_name=None):
    """The float64 sums and gradient for a table shape, an input kind and one of the named coefficient sets."""
    pred, target = inputs(n_fft, hop, L, kind)
    return sums_and_grad(pred, target, n_fft, hop, eps, None if coef_name is None else coefficients(coef_name, n_fft + hop + L))


def coefficients(name, seed=0, rows=ROWS):
    """(rows, 3) float32: the unit coefficients "A", "E", "D", or "random": positive, different per row."""
    if name == "random":
        return 0.25 + torch.rand(rows, 3, generator=torch.Generator().manual_seed(seed))
    return torch.tensor([[float(name == c) for c in "AED"]]).repeat(rows, 1)


def add_sum_and_difference(x):
    left, right = x[..., 0:1, :], x[..., 1:2, :]
    return torch.cat([x, left + right, left - right], -2)


def loss_and_grad(pred, target, resolutions, w_sc, w_log, w_lin, eps, sum_and_difference=False):
    """The module's loss in float64 and its gradient with respect to pred.  resolutions: (n_fft, hop, win_length) each."""
    p = pred.double().requires_grad_(True)
    rows_p, rows_t = (add_sum_and_difference(x) if sum_and_difference else x for x in (p, target.double()))
    L = pred.shape[-1]
    rows_p, rows_t = rows_p.reshape(-1, L), rows_t.reshape(-1, L)
    total = 0.0
    for n_fft, hop, win_length in resolutions:
        A, B, E, D = sums_of(rows_p, rows_t, n_fft, hop, hann(n_fft, win_length), eps).unbind(-1)
        M = (n_fft // 2 + 1) * (1 + L // hop)
        total = total + (w_sc * torch.sqrt(A / B) + w_log * D / M + w_lin * E / M).mean()
    loss = total / len(resolutions)
    loss.backward()
    return loss.detach(), p.grad


def margins(pred, target, n_fft, hop, eps):
    """How far the float64 spectra of an input stay from where the loss's gradient jumps: (the smallest
    |P.re^2 + P.im^2 - eps| / eps, the smallest ||T| - |P|| / mean |T| over the bins whose pred is live)."""
    w = hann(n_fft)
    P, T = spectrum(pred.double(), n_fft, hop, w), spectrum(target.double(), n_fft, hop, w)
    p2 = P.real.square() + P.imag.square()
    band = float(((p2 - eps).abs() / eps).min())
    mP, mT = magnitude(P, eps), magnitude(T, eps)
    gap = float(((mT - mP).abs()[p2 > eps]).min() / mT.mean())
    return band, gap
