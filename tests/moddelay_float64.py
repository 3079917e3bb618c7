"""Float64 yardstick of the modulated delay line (tests/test_moddelay_abi.py, tests/test_gpu_moddelay.py): the definition

    theta[v,c,n] = rate[r,v] p + phase[r,v,c]                            p = pos[r] + n; reduced mod 1
    d[v,c,n]     = clamp(delay[r,v] + depth[r,v] sin(2 pi theta), 1, Dmax)
    i = floor(d), f = d - i
    u[v,c,n]     = sum_j l_j(f) x[c, n - i - j]                          x zero, or the carried history, below the row's start
    y[c,n]       = dry[r] x[c,n] + sum_v gain[r,v,c] u[v,c,n]

as torch ops in float64 on float32 inputs on the CPU, so that autograd gives all seven gradients; the same as a brute-force
loop; the written adjoint; parameters drawn inside the contract 2 pi rate depth <= 1/2; and bright test signals.  Not a
test module."""
import math

import numpy as np
import torch

NODES = {"linear": (0, 1), "cubic": (-1, 0, 1, 2)}


def weights(f, interp):
    """l_j(f) for the nodes of ``interp``, in their order."""
    if interp == "linear":
        return [1 - f, f]
    return [-f * (f - 1) * (f - 2) / 6, (f + 1) * (f - 1) * (f - 2) / 2, -(f + 1) * f * (f - 2) / 2, (f + 1) * f * (f - 1) / 6]


def slopes(f, interp):
    """l'_j(f)."""
    if interp == "linear":
        return [-1 + 0 * f, 1 + 0 * f]
    q = 3 * f * f
    return [-(q - 6 * f + 2) / 6, (q - 4 * f - 1) / 2, -(q - 2 * f - 2) / 2, (q - 1) / 6]


def oscillator(delay, depth, rate, phase, L, Dmax, pos=None):
    """-> (sin, cos, the unclamped delay) of shape (R, V, C, L) in float64, differentiable in the four parameters."""
    R = delay.shape[0]
    pos = torch.zeros(R, dtype=torch.int64) if pos is None else pos
    p = (pos[:, None] + torch.arange(L)).double()[:, None, None, :]
    theta = rate.double()[:, :, None, None] * p + phase.double()[..., None]
    theta = theta - theta.detach().floor()
    s, c = torch.sin(2 * math.pi * theta), torch.cos(2 * math.pi * theta)
    return s, c, delay.double()[:, :, None, None] + depth.double()[:, :, None, None] * s


def read_positions(delay, depth, rate, phase, L, Dmax, pos=None):
    """m(n) = n - floor(d[n]) -> int64 (R, V, C, L)."""
    _, _, raw = oscillator(delay, depth, rate, phase, L, Dmax, pos)
    return torch.arange(L) - raw.clamp(1, Dmax).floor().long()


def forward(x, delay, depth, rate, phase, gain, dry, Dmax, interp, state=None):
    """-> (y (R, C, L) float64, (history (R, C, Dmax + 2) float64, position (R,) int64)); differentiable in x and the six
    parameters.  ``state``: the pair an earlier block returned."""
    x = x.double()
    R, C, L = x.shape
    V, S = delay.shape[1], Dmax + 2
    zi, pos = (x.new_zeros(R, C, S), torch.zeros(R, dtype=torch.int64)) if state is None else (state[0].double(), state[1])
    assert tuple(zi.shape) == (R, C, S) and tuple(pos.shape) == (R,)
    _, _, raw = oscillator(delay, depth, rate, phase, L, Dmax, pos)
    d = raw.clamp(1, Dmax)
    i = d.detach().floor()
    f = d - i
    xx = torch.cat([zi, x], -1)                                       # sample k at index k + S
    lines = xx[:, None].expand(R, V, C, S + L)
    base = S + torch.arange(L) - i.long()
    u = sum(w * lines.gather(-1, base - j) for j, w in zip(NODES[interp], weights(f, interp)))
    y = dry.double().reshape(R, 1, 1) * x + (gain.double()[..., None] * u).sum(1)
    return y, (xx[..., L:L + S].detach().clone(), pos + L)


def gradients(x, g, delay, depth, rate, phase, gain, dry, Dmax, interp):
    """-> (gx, g_delay, g_depth, g_rate, g_phase, g_gain, g_dry) of sum(g y) by torch autograd in float64."""
    leaves = [t.double().clone().requires_grad_(True) for t in (x, delay, depth, rate, phase, gain, dry)]
    y, _ = forward(*leaves, Dmax, interp)
    (y * g.double()).sum().backward()
    return tuple(t.grad for t in leaves)


def adjoint(x, g, delay, depth, rate, phase, gain, dry, Dmax, interp):
    """The written adjoint (no state) over numpy doubles -> the seven gradients in the order of ``gradients``."""
    R, C, L = x.shape
    V = delay.shape[1]
    s, cs, raw = (t.numpy() for t in oscillator(delay, depth, rate, phase, L, Dmax))
    x, g = x.double().numpy(), g.double().numpy()
    dl, dp, gn, dr = (t.double().numpy() for t in (delay, depth, gain, dry.reshape(R)))
    d = np.clip(raw, 1, Dmax)
    open_ = (raw >= 1) & (raw <= Dmax)
    i = np.floor(d).astype(np.int64)
    f = d - i
    n = np.arange(L)
    gx = dr[:, None, None] * g
    gdelay, gdepth, grate = np.zeros((R, V)), np.zeros((R, V)), np.zeros((R, V))
    gphase, ggain = np.zeros((R, V, C)), np.zeros((R, V, C))
    gdry = (g * x).sum((1, 2))
    for r in range(R):
        for v in range(V):
            for c in range(C):
                w, dw = weights(f[r, v, c], interp), slopes(f[r, v, c], interp)
                u, du = np.zeros(L), np.zeros(L)
                for j, wj, dwj in zip(NODES[interp], w, dw):
                    k = n - i[r, v, c] - j
                    ok = k >= 0
                    xv = np.where(ok, x[r, c, np.maximum(k, 0)], 0.0)
                    u += wj * xv
                    du += dwj * xv
                    np.add.at(gx[r, c], k[ok], gn[r, v, c] * (g[r, c] * wj)[ok])
                e = np.where(open_[r, v, c], g[r, c] * gn[r, v, c] * du, 0.0)
                turn = e * dp[r, v] * 2 * math.pi * cs[r, v, c]
                ggain[r, v, c] = (g[r, c] * u).sum()
                gdelay[r, v] += e.sum()
                gdepth[r, v] += (e * s[r, v, c]).sum()
                grate[r, v] += (turn * n).sum()
                gphase[r, v, c] = turn.sum()
    return gx, gdelay, gdepth, grate, gphase, ggain, gdry


def brute(x, delay, depth, rate, phase, gain, dry, Dmax, interp, state=None):
    """The definition as a loop over single samples in Python floats -> y (R, C, L) numpy float64."""
    R, C, L = x.shape
    V, S = delay.shape[1], Dmax + 2
    xs = x.double().numpy()
    zi = np.zeros((R, C, S)) if state is None else state[0].double().numpy()
    pos = [0] * R if state is None else state[1].tolist()
    y = np.zeros((R, C, L))
    for r in range(R):
        for c in range(C):
            def sample(k):
                if k >= 0:
                    return xs[r, c, k]
                return zi[r, c, S + k] if k >= -S else 0.0
            for n in range(L):
                acc = float(dry.reshape(R)[r]) * xs[r, c, n]
                for v in range(V):
                    theta = float(rate[r, v]) * (pos[r] + n) + float(phase[r, v, c])
                    theta -= math.floor(theta)
                    d = min(max(float(delay[r, v]) + float(depth[r, v]) * math.sin(2 * math.pi * theta), 1.0), float(Dmax))
                    i = math.floor(d)
                    for j, w in zip(NODES[interp], weights(d - i, interp)):
                        acc += float(gain[r, v, c]) * w * sample(n - i - j)
                y[r, c, n] = acc
    return y


def draw_parameters(R, V, C, max_delay, seed):
    """Physical parameters inside the contract, float32 -> (delay, depth, rate (R, V), phase, gain (R, V, C), dry (R,)):
    the delay uniform in [1, Dmax], the rate up to 2e-3 cycles per sample, the depth a uniform share of
    min(delay - 1, Dmax - delay, 0.5 / (2 pi rate)).  Row 0 is drawn like that throughout; in the rows after it voice v of
    row r is, by (r - 1 + v) mod 3: an integer delay with depth 0; a rate of 0; a swing delay +- depth that touches both
    clamps (delay = (1 + Dmax) / 2, depth = (Dmax - 1) / 2)."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)   # noqa: E731
    D = float(max_delay)
    delay = 1 + (D - 1) * u(R, V)
    rate = 2e-3 * u(R, V)
    share = 0.98 * u(R, V)
    for r in range(1, R):
        for v in range(V):
            kind = (r - 1 + v) % 3
            if kind == 0:
                delay[r, v], share[r, v] = float(torch.round(delay[r, v])), 0.0
            elif kind == 1:
                rate[r, v] = 0.0
            else:
                delay[r, v], share[r, v] = (1 + D) / 2, 1.0
                rate[r, v] = min(float(rate[r, v]), 0.9 * 0.5 / (2 * math.pi * (D - 1) / 2))
    room = torch.minimum(torch.minimum(delay - 1, D - delay), 0.5 / (2 * math.pi * rate.clamp_min(1e-30)))
    depth = share * room
    phase = u(R, V, C)
    gain = (0.2 + 0.8 * u(R, V, C)) * torch.where(u(R, V, C) < 0.5, -1.0, 1.0) / V
    dry = 0.3 + 0.7 * u(R)
    return tuple(t.float() for t in (delay, depth, rate, phase, gain, dry))


def bright_rows(R, C, L, seed):
    """float32 (R, C, L) white noise -- the worst case for a wrong fraction f -- with the last row (of more than one) quiet,
    at 1e-3."""
    x = torch.randn(R, C, L, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    if R > 1:
        x[-1] *= 1e-3
    return x
