"""Float64 yardstick of the feedback delay (tests/test_fbdelay_abi.py, tests/test_gpu_fbdelay.py): the definition

    i_c = floor(delay[r,c]),  f_c = delay[r,c] - i_c
    s_c[n] = (1 - f_c) w_c[n - i_c] + f_c w_c[n - i_c - 1]              w, q zero, or the carried state, below the row's start
    q_c[n] = (1 - a[r,c]) s_c[n] + a[r,c] q_c[n - 1]
    w_c[n] = x_c[n] + sum_c' F[r,c,c'] q_c'[n]
    y_c[n] = dry[r] x_c[n] + wet[r] q_c[n]

as torch ops in float64 on float32 inputs on the CPU, so that autograd gives all six gradients; the same as a brute-force
loop over single samples; the written adjoint; parameters drawn inside the contract; and bright test signals.  The
torch version walks each row by itself in chunks of min_c i_c samples: inside a chunk s is two slices of what earlier
chunks wrote, and the one-pole is a lower-triangular Toeplitz product.  Not a test module."""
import numpy as np
import torch

MIN_DELAY = 64
MAX_CHUNK = 1024          # the Toeplitz matrix of a chunk is quadratic in its length: longer delays are walked in pieces
NAMES = ("x", "delay", "damping", "feedback", "dry", "wet")


def _onepole(a, K):
    """(C, K, K) lower-triangular Toeplitz matrix of q[n] = (1 - a) s[n] + a q[n - 1] and (C, K) a^(k + 1); the powers are
    a running product, whose derivative is finite at a = 0."""
    k = torch.arange(K)
    pw = torch.cumprod(torch.cat([torch.ones_like(a)[:, None], a[:, None].expand(-1, K)], -1), -1)
    tri = (k[:, None] >= k[None, :]).to(a.dtype)
    return (1 - a)[:, None, None] * pw[:, (k[:, None] - k[None, :]).clamp_min(0)] * tri, pw[:, 1:]


class _Line:
    """What has entered one channel's line so far, as the pieces it arrived in; ``take(p0, p1)`` is a slice of their
    concatenation (differentiable, and touching only the pieces it meets)."""

    def __init__(self, first):
        self.pieces, self.starts, self.end = [first], [0], first.shape[-1]

    def append(self, piece):
        self.pieces.append(piece)
        self.starts.append(self.end)
        self.end += piece.shape[-1]

    def take(self, p0, p1):
        assert 0 <= p0 <= p1 <= self.end
        out = []
        # pieces after the first have one length: jump to the first that can meet [p0, p1)
        j = 0
        if len(self.pieces) > 1 and p0 >= self.starts[1]:
            j = 1 + (p0 - self.starts[1]) // self.pieces[1].shape[-1]
        while j < len(self.pieces) and self.starts[j] < p1:
            s = self.starts[j]
            out.append(self.pieces[j][max(p0 - s, 0):p1 - s])
            j += 1
        return torch.cat(out) if len(out) != 1 else out[0]


def _row(x, delay, a, F, hist, q_last):
    """One row: x (C, L), delay, a (C), F (C, C), hist (C, S), q_last (C) -> q, w (C, L), the new q_last (C)."""
    C, L = x.shape
    S = hist.shape[-1]
    i = [int(v) for v in delay.detach().floor()]
    f = delay - delay.detach().floor()
    K = min(min(i), L, MAX_CHUNK)
    T, apow = _onepole(a, K)
    lines = [_Line(hist[c]) for c in range(C)]
    qs, wchunks = [], []
    for n0 in range(0, L, K):
        Kc = min(K, L - n0)
        s = []
        for c in range(C):
            run = lines[c].take(S + n0 - i[c] - 1, S + n0 - i[c] + Kc)      # w[n0 - i - 1 .. n0 - i + Kc - 1]
            s.append((1 - f[c]) * run[1:] + f[c] * run[:-1])
        s = torch.stack(s)
        q = (T[:, :Kc, :Kc] @ s[..., None])[..., 0] + apow[:, :Kc] * q_last[:, None]
        q_last = q[:, -1]
        w = x[:, n0:n0 + Kc] + F @ q
        for c in range(C):
            lines[c].append(w[c])
        qs.append(q)
        wchunks.append(w)
    return torch.cat(qs, -1), torch.cat(wchunks, -1), q_last


def forward(x, delay, damping, feedback, dry, wet, Dmax, state=None, signals=False):
    """-> (y (R, C, L) float64, (history (R, C, Dmax + 1) float64, q_last (R, C) float64)); differentiable in x and the five
    parameters.  ``state``: the pair an earlier block returned.  ``signals``: also (q, w)."""
    x = x.double()
    R, C, L = x.shape
    S = Dmax + 1
    delay, a, F = delay.double().reshape(R, C), damping.double().reshape(R, C), feedback.double().reshape(R, C, C)
    assert float(delay.detach().min()) >= MIN_DELAY and float(delay.detach().max()) <= Dmax
    hist, q_last = (x.new_zeros(R, C, S), x.new_zeros(R, C)) if state is None else (state[0].double(), state[1].double())
    assert tuple(hist.shape) == (R, C, S) and tuple(q_last.shape) == (R, C)
    rows = [_row(x[r], delay[r], a[r], F[r], hist[r], q_last[r]) for r in range(R)]
    q, w, last = (torch.stack([row[k] for row in rows]) for k in range(3))
    y = dry.double().reshape(R, 1, 1) * x + wet.double().reshape(R, 1, 1) * q
    after = (torch.cat([hist, w], -1)[..., L:L + S].detach().clone(), last.detach().clone())
    return (y, after, (q, w)) if signals else (y, after)


def gradients(x, g, delay, damping, feedback, dry, wet, Dmax):
    """-> (gx, g_delay, g_damping, g_feedback, g_dry, g_wet) of sum(g y) by torch autograd in float64."""
    leaves = [t.double().clone().requires_grad_(True) for t in (x, delay, damping, feedback, dry, wet)]
    y, _ = forward(*leaves, Dmax)
    (y * g.double()).sum().backward()
    return leaf_gradients(leaves)


def leaf_gradients(leaves):
    """The leaves' gradients after a backward; zeros for a leaf nothing reached (the feedback matrix of a signal shorter
    than its delays: what enters the line never comes out)."""
    return tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in leaves)


def _np(*ts):
    return [t.detach().double().numpy() for t in ts]


def brute(x, delay, damping, feedback, dry, wet, Dmax, state=None, signals=False):
    """The definition as a loop over single samples in numpy doubles -> y (R, C, L) (``signals``: y, q, w, s)."""
    R, C, L = x.shape
    S = Dmax + 1
    xs, dl, a, F, dr, we = _np(x, delay.reshape(R, C), damping.reshape(R, C), feedback.reshape(R, C, C), dry.reshape(R),
                               wet.reshape(R))
    hist = np.zeros((R, C, S)) if state is None else _np(state[0])[0]
    qprev = np.zeros((R, C)) if state is None else _np(state[1])[0].copy()
    i = np.floor(dl).astype(np.int64)
    f = dl - i
    w = np.concatenate([hist, np.zeros((R, C, L))], -1)            # sample k at index k + S
    q, s = np.zeros((R, C, L)), np.zeros((R, C, L))
    for r in range(R):
        for n in range(L):
            for c in range(C):
                s[r, c, n] = (1 - f[r, c]) * w[r, c, S + n - i[r, c]] + f[r, c] * w[r, c, S + n - i[r, c] - 1]
                q[r, c, n] = (1 - a[r, c]) * s[r, c, n] + a[r, c] * qprev[r, c]
            qprev[r] = q[r, :, n]
            for c in range(C):
                w[r, c, S + n] = xs[r, c, n] + sum(F[r, c, d] * q[r, d, n] for d in range(C))
    y = dr[:, None, None] * xs + we[:, None, None] * q
    return (y, q, w[..., S:], s) if signals else y


def adjoint(x, g, delay, damping, feedback, dry, wet, Dmax):
    """The written adjoint (no state) over numpy doubles -> the six gradients in the order of ``gradients``:
        lambda_c[n] = (1 - f_c) mu_c[n + i_c] + f_c mu_c[n + i_c + 1]
        zeta_c[n]   = wet gy_c[n] + sum_c' F[c',c] lambda_c'[n]
        mu_c[n]     = (1 - a_c) zeta_c[n] + a_c mu_c[n + 1]
        gx_c[n]     = dry gy_c[n] + lambda_c[n]
    and the parameter gradients as plain sums over n."""
    R, C, L = x.shape
    xs, gy, dl, a, F, dr, we = _np(x, g, delay.reshape(R, C), damping.reshape(R, C), feedback.reshape(R, C, C), dry.reshape(R),
                                   wet.reshape(R))
    _, q, w, s = brute(x, delay, damping, feedback, dry, wet, Dmax, signals=True)
    i = np.floor(dl).astype(np.int64)
    f = dl - i
    mu = np.zeros((R, C, L + Dmax + 2))                              # zero beyond the row's end
    lam = np.zeros((R, C, L))
    for r in range(R):
        for n in range(L - 1, -1, -1):
            for c in range(C):
                lam[r, c, n] = (1 - f[r, c]) * mu[r, c, n + i[r, c]] + f[r, c] * mu[r, c, n + i[r, c] + 1]
            for c in range(C):
                zeta = we[r] * gy[r, c, n] + sum(F[r, d, c] * lam[r, d, n] for d in range(C))
                mu[r, c, n] = (1 - a[r, c]) * zeta + a[r, c] * mu[r, c, n + 1]
    mu = mu[..., :L]
    gx = dr[:, None, None] * gy + lam
    wpad = np.concatenate([np.zeros((R, C, Dmax + 1)), w], -1)      # sample k at index k + Dmax + 1
    qb = np.concatenate([np.zeros((R, C, 1)), q[..., :-1]], -1)     # q[n - 1]
    n = np.arange(L)
    gdelay, gdamp = np.zeros((R, C)), np.zeros((R, C))
    for r in range(R):
        for c in range(C):
            at = Dmax + 1 + n - i[r, c]
            gdelay[r, c] = (mu[r, c] * (wpad[r, c, at - 1] - wpad[r, c, at])).sum()
            gdamp[r, c] = (mu[r, c] * (qb[r, c] - s[r, c])).sum() / (1 - a[r, c])
    gF = np.einsum("rcn,rdn->rcd", lam, q)
    return gx, gdelay, gdamp, gF, (gy * xs).sum((1, 2)), (gy * q).sum((1, 2))


def draw_parameters(R, C, max_delay, seed, max_feedback=0.95, max_damping=0.95):
    """Physical parameters inside the contract, float32 -> (delay, damping (R, C), feedback (R, C, C), dry, wet (R,)).  By
    r mod 3:
      0: channel 0 at delay = 64.0 exactly with a = 0; with two channels the other one far away, a quarter sample under
         max_delay, with a = max_damping; the feedback a ping-pong mixture whose row sums are max_feedback;
      1: every delay within a sample of max_delay, a second channel's at max_delay exactly; a and the feedback drawn;
      2: everything drawn: the delays anywhere in the range, a general feedback matrix with signs, row sums of |F| <= 0.9."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)   # noqa: E731
    D = float(max_delay)
    delay = MIN_DELAY + (D - MIN_DELAY) * u(R, C)
    a = max_damping * u(R, C)
    F = (2 * u(R, C, C) - 1)
    F = F / F.abs().sum(-1, keepdim=True) * (0.3 + 0.6 * u(R, 1, 1))
    for r in range(R):
        kind = r % 3
        cross = float(u(1))
        pingpong = torch.tensor([[1 - cross, cross], [cross, 1 - cross]], dtype=torch.float64)[:C, :C] if C == 2 else torch.ones(1, 1)
        if kind == 0:
            delay[r, 0], a[r, 0] = float(MIN_DELAY), 0.0
            if C == 2:
                delay[r, 1], a[r, 1] = D - 0.25, max_damping
            F[r] = max_feedback * pingpong
        elif kind == 1:
            delay[r] = D - u(C)
            if C == 2:
                delay[r, 1] = D
            F[r] = (0.2 + 0.7 * float(u(1))) * pingpong
    delay = delay.float().clamp(float(MIN_DELAY), D)
    F = F.float()
    assert float(F.double().abs().sum(-1).max()) < 1
    dry, wet = 0.3 + 0.7 * u(R), 0.3 + 0.7 * u(R)
    return delay, a.float(), F, dry.float(), wet.float()


def bright_rows(R, C, L, seed):
    """float32 (R, C, L) white noise -- the worst case for a wrong fraction f -- with the last row (of more than one) quiet,
    at 1e-3."""
    x = torch.randn(R, C, L, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    if R > 1:
        x[-1] *= 1e-3
    return x
