"""Forward + backward of the exact biquad cascade: the native one-pass backward (autograd.BiquadCascadeFn on
gfx_biquad_cascade_bwd_f32) against the per-section formula it replaced, kept here as the baseline (nothing in the package
calls it), on the same tensors, interleaved rounds in one process; and the native path alone at the console shape.

    python tools/biquad_bwd_bench.py [rows_compare=512] [rows_native=8192] [rounds=3] [K ...=1 6 31]

Prints one line per K and shape: median milliseconds of forward + backward and of the backward alone, the peak memory above
the inputs in units of one (R, C, L) signal tensor, and for the native backward its rate over the bytes it must move: x
twice (both passes), g once, gx once = 16 B per channel-sample."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from grafx_amd import ops  # noqa: E402
from grafx_amd.autograd import BiquadCascadeFn  # noqa: E402

C, L = 2, 131072


class PerSectionFn(torch.autograd.Function):
    """The backward BiquadCascadeFn had before the one-pass kernel.  Forward: one launch per section, every section's output
    saved.  Backward, per section from the last to the first (g_K = dL/dy, u_0 = x, u_i = H_i u_{i-1}):
        v_i     = (1 / A_i)^T g_i                    the all-pole part run backwards in time (the forward kernel on the
                                                     time-reversed gradient)
        dB_i[d] =  sum_n v_i[n] u_{i-1}[n - d]       d = 0, 1, 2
        dA_i[d] = -sum_n v_i[n] u_i[n - d]           d = 0, 1, 2   (dy/da_d = -(z^-d / A) y)
        g_{i-1} = B_i^T v_i                          g_{i-1}[n] = sum_d b_d v_i[n + d]"""

    @staticmethod
    def forward(ctx, x, Bs, As):
        K = Bs.shape[2]
        us = [x.contiguous()]
        for i in range(K):
            us.append(ops.biquad_cascade(us[-1], Bs[:, :, i : i + 1].contiguous(), As[:, :, i : i + 1].contiguous()))
        ctx.save_for_backward(Bs, As, *us)
        return us[-1]

    @staticmethod
    def backward(ctx, gy):
        Bs, As, *us = ctx.saved_tensors
        R, Cf, K, _ = Bs.shape
        L = gy.shape[-1]
        g = gy.contiguous()
        Cout = g.shape[1]
        gB, gA = torch.zeros_like(Bs), torch.zeros_like(As)
        unit = torch.zeros((R, Cf, 1, 3), dtype=Bs.dtype, device=Bs.device)
        unit[..., 0] = 1.0

        def to_filter_channels(t):     # (R, Cout) -> (R, Cf)
            return t.sum(1, keepdim=True) if (Cf == 1 and Cout > 1) else t

        for i in reversed(range(K)):
            Ai = As[:, :, i : i + 1].contiguous()
            v = ops.biquad_cascade(g.flip(-1).contiguous(), unit, Ai).flip(-1)   # (R, Cout, L)
            u_in, u_out = us[i], us[i + 1]
            for d in range(3):
                vd = v[..., d:]
                gB[:, :, i, d] = to_filter_channels((vd * u_in[..., : L - d]).sum(-1).expand(R, Cout))
                gA[:, :, i, d] = -to_filter_channels((vd * u_out[..., : L - d]).sum(-1))
            b = Bs[:, :, i]                                                        # (R, Cf, 3), broadcasts over channels
            gp = b[..., 0:1] * v
            gp[..., :-1] += b[..., 1:2] * v[..., 1:]
            gp[..., :-2] += b[..., 2:3] * v[..., 2:]
            g = gp
        x = us[0]
        gx = g.sum(1, keepdim=True) if x.shape[1] == 1 and Cout > 1 else g
        return gx, gB, gA


def tensors(R, K):
    """Equaliser-like sections (zeros at the poles' angle, inside them): a long cascade stays well conditioned."""
    gen = torch.Generator().manual_seed(0)
    radius = 0.5 + 0.45 * torch.rand(R, C, K, generator=gen)
    theta = 0.1 + 2.9 * torch.rand(R, C, K, generator=gen)
    rz = radius * (0.8 + 0.2 * torch.rand(R, C, K, generator=gen))
    As = torch.stack([torch.ones_like(radius), -2 * radius * torch.cos(theta), radius.square()], -1)
    Bs = torch.stack([torch.ones_like(rz), -2 * rz * torch.cos(theta), rz.square()], -1)
    x = torch.randn(R, C, L, device="cuda")
    return x.requires_grad_(), Bs.cuda().requires_grad_(), As.cuda().requires_grad_(), torch.randn(R, C, L, device="cuda")


def step(fn, x, Bs, As, gy):
    """-> (ms forward + backward, ms backward, peak bytes above what was allocated before)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    y = fn(x, Bs, As)
    b.record()
    grads = torch.autograd.grad(y, [x, Bs, As], gy)
    c.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del y, grads
    return a.elapsed_time(c), b.elapsed_time(c), peak


def summary(runs, one):
    both, bwd, peak = zip(*runs)
    return (f"fwd+bwd {statistics.median(both):9.2f} ms  bwd {statistics.median(bwd):9.2f} ms  "
            f"peak {max(peak) / one:5.2f} tensors"), statistics.median(both), statistics.median(bwd)


def main():
    rows_cmp = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    rows_nat = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    Ks = [int(k) for k in sys.argv[4:]] or [1, 6, 31]
    for K in Ks:
        if rows_cmp:
            args, one = tensors(rows_cmp, K), rows_cmp * C * L * 4
            runs = {"native": [], "per-section": []}
            for r in range(rounds + 1):                     # (round 0 warms both up)
                for key, fn in (("native", BiquadCascadeFn.apply), ("per-section", PerSectionFn.apply)):
                    t = step(fn, *args)
                    if r:
                        runs[key].append(t)
            (nat, nat_ms, _), (old, old_ms, _) = summary(runs["native"], one), summary(runs["per-section"], one)
            print(f"K={K:2d} R={rows_cmp:5d}  native {nat} | per-section {old} | x{old_ms / nat_ms:.1f}", flush=True)
            del args
            torch.cuda.empty_cache()
        if rows_nat:
            args, one = tensors(rows_nat, K), rows_nat * C * L * 4
            text, _, bwd_ms = summary([step(BiquadCascadeFn.apply, *args) for _ in range(rounds + 1)][1:], one)
            moved = 16 * rows_nat * C * L
            print(f"K={K:2d} R={rows_nat:5d}  native {text} | backward {moved / bwd_ms / 1e9:.2f} TB/s over 16 B per "
                  f"channel-sample ({moved / 1e9:.1f} GB)", flush=True)
            del args
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
