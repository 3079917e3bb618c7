"""Float64 yardstick of the look-ahead limiter (tests/test_limiter_abi.py, tests/test_gpu_limiter.py): the definition

    p[k]  = max_c |x[c, k]|                          zero outside [0, L), or the state below 0
    pk[q] = max_{0 <= j < M} p[q - j]                M = D + 1 + H; ties take the earliest index a(q)
    m[q]  = T / pk[q] if pk[q] > T else 1            T = exp(log_ceiling)
    s[n]  = sum_{0 <= j < N} w[j] m[n - j]
    y[c, n] = x[c, n + sigma - D] s[n + sigma]       0 <= n < L, sigma in {0, D}

as torch ops in float64 on the CPU, so that autograd gives both gradients; the same as a brute-force loop; the written
adjoint as a loop; and the test whether an input has a tie that a gradient would see.  Not a test module."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def window(D, N=None):
    """The N (default D + 1) Hann taps sin^2(pi (k + 1) / (N + 1)) normalised in float64, rounded to float32."""
    N = D + 1 if N is None else N
    w = torch.sin(math.pi * torch.arange(1, N + 1, dtype=torch.float64) / (N + 1)).square()
    return (w / w.sum()).float()


def _padded(x, state, M, N, sigma):
    """x (R, C, L) behind its state (zeros without one) and before sigma zeros: sample k at index k + S."""
    R, C, _ = x.shape
    S = M + N - 2
    zi = x.new_zeros(R, C, S) if state is None else state.to(x.dtype)
    assert tuple(zi.shape) == (R, C, S)
    return torch.cat([zi, x, x.new_zeros(R, C, sigma)], -1), S


def forward(x, log_ceiling, w, D, H, sigma=0, state=None):
    """-> (y (R, C, L), gain (R, L), zf (R, C, M + N - 2)) in float64, differentiable in x and log_ceiling."""
    assert sigma in (0, D) and (state is None or sigma == 0)
    x, w = x.double(), w.double()
    R, C, L = x.shape
    M, N = D + 1 + H, w.numel()
    T = torch.exp(log_ceiling.double()).reshape(R, 1)
    xx, S = _padded(x, state, M, N, sigma)
    p = xx.abs().amax(1)
    pk = F.max_pool1d(p.unsqueeze(1), M, 1).squeeze(1)                       # q = -(N - 1) .. L + sigma - 1
    over = pk > T
    m = torch.where(over, T / torch.where(over, pk, torch.ones_like(pk)), torch.ones_like(pk))
    s = F.conv1d(m.unsqueeze(1), w.flip(0).view(1, 1, N)).squeeze(1)         # s[n'], 0 <= n' < L + sigma
    gain = s[:, sigma:sigma + L]
    y = xx[..., S + sigma - D:S + sigma - D + L] * gain.unsqueeze(1)
    return y, gain, xx[..., L:L + S].detach().clone()


def check_ties(x, log_ceiling, w, D, H, sigma=0, state=None):
    """Raises ValueError when a gradient would see a tie: a window whose maximum exceeds T and is reached twice, or two
    channels with equal |x| at a sample above T (only such a sample can be the peak of a limiting window)."""
    x = x.double()
    R, C, L = x.shape
    M, N = D + 1 + H, w.numel()
    T = torch.exp(log_ceiling.double()).reshape(R, 1)
    xx, _ = _padded(x, state, M, N, sigma)
    mag = xx.abs()
    p = mag.amax(1)
    if C > 1:
        top = mag.topk(2, dim=1).values
        if bool(((top[:, 0] == top[:, 1]) & (p > T)).any()):
            raise ValueError("two channels hold the same peak above the ceiling")
    n = p.shape[-1]
    pk, first = F.max_pool1d(p.unsqueeze(1), M, 1, return_indices=True)
    _, back = F.max_pool1d(p.flip(-1).unsqueeze(1), M, 1, return_indices=True)
    other = (n - 1 - back).flip(-1)                    # the same windows' maxima found from the other end
    if bool(((first != other) & (pk > T.unsqueeze(1))).any()):
        raise ValueError("a window above the ceiling reaches its maximum twice")


def gradients(x, g, log_ceiling, w, D, H, sigma=0):
    """-> (gx, g_log_ceiling) of sum(g y) by torch autograd in float64; the input must pass check_ties."""
    check_ties(x, log_ceiling, w, D, H, sigma)
    x = x.double().clone().requires_grad_(True)
    lc = log_ceiling.double().clone().requires_grad_(True)
    y, _, _ = forward(x, lc, w, D, H, sigma)
    (y * g.double()).sum().backward()
    return x.grad, lc.grad


def brute(x, log_ceiling, w, D, H, sigma=0, state=None):
    """The definition as loops over numpy doubles -> (y, gain, a): a[r][q'] = a(q) for q = q' - (N - 1) as a sample index."""
    x, w = x.double().numpy(), w.double().numpy()
    R, C, L = x.shape
    M, N = D + 1 + H, len(w)
    S = M + N - 2
    zi = np.zeros((R, C, S)) if state is None else state.double().numpy()
    T = np.exp(log_ceiling.double().numpy().reshape(R))

    def sample(r, c, k):
        if 0 <= k < L:
            return x[r, c, k]
        return zi[r, c, S + k] if -S <= k < 0 else 0.0

    y, gain = np.zeros((R, C, L)), np.zeros((R, L))
    arg = np.zeros((R, L + sigma + N - 1), dtype=np.int64)
    for r in range(R):
        m = {}
        for q in range(-(N - 1), L + sigma):
            best, at = -1.0, None
            for k in range(q - M + 1, q + 1):
                v = max(abs(sample(r, c, k)) for c in range(C))
                if v > best:
                    best, at = v, k
            arg[r, q + N - 1] = at
            m[q] = T[r] / best if best > T[r] else 1.0
        for n in range(L):
            s = 0.0
            for j in range(N):
                s += w[j] * m[n + sigma - j]
            gain[r, n] = s
            for c in range(C):
                y[r, c, n] = sample(r, c, n + sigma - D) * s
    return y, gain, arg


def adjoint(x, g, log_ceiling, w, D, H, sigma=0):
    """The written adjoint (no state) as loops over numpy doubles -> (gx, g_log_ceiling)."""
    x, g, w = x.double().numpy(), g.double().numpy(), w.double().numpy()
    R, C, L = x.shape
    M, N = D + 1 + H, len(w)
    T = np.exp(log_ceiling.double().numpy().reshape(R))
    gx, gc = np.zeros((R, C, L)), np.zeros(R)

    def xs(r, c, k):
        return x[r, c, k] if 0 <= k < L else 0.0

    def G(r, c, q):
        return g[r, c, q - sigma] if 0 <= q - sigma < L else 0.0

    for r in range(R):
        p = lambda k: max(abs(xs(r, c, k)) for c in range(C))   # noqa: E731
        lo, hi = -(N - 1), L + sigma + M                         # every q that can matter
        pk, a = {}, {}
        for q in range(lo, hi):
            best, at = -1.0, None
            for k in range(q - M + 1, q + 1):
                if p(k) > best:
                    best, at = p(k), k
            pk[q], a[q] = best, at
        m = {q: T[r] / pk[q] if pk[q] > T[r] else 1.0 for q in pk}
        gs = {q: sum(G(r, c, q) * xs(r, c, q - D) for c in range(C)) for q in range(lo, hi + N)}
        gm = {q: sum(w[j] * gs[q + j] for j in range(N)) for q in range(lo, hi)}
        for q in range(lo, hi):
            if pk[q] > T[r]:
                gc[r] += T[r] * gm[q] / pk[q]
        for k in range(L):
            s = sum(w[j] * m[k + D - j] for j in range(N))
            cstar = min(c for c in range(C) if abs(x[r, c, k]) == p(k))
            routed = sum(gm[q] * (-T[r] / pk[q] ** 2) for q in range(lo, hi) if a[q] == k and pk[q] > T[r])
            for c in range(C):
                gx[r, c, k] = G(r, c, k + D) * s + (np.sign(x[r, c, k]) * routed if c == cstar else 0.0)
    return gx, gc


def burst_rows(R, C, L, seed, scale=0.1, burst=5.0):
    """float32 (R, C, L): normal rows of standard deviation ``scale`` with a stretch ``burst`` times louder in the middle --
    well above a ceiling of about 2.5 ``scale``, with quiet stretches under it."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(R, C, L, generator=gen, dtype=torch.float32) * scale
    lo, hi = L // 3, max(L // 3 + 1, L // 2)
    x[..., lo:hi] *= burst
    return x
