"""Forward + backward of the look-ahead limiter alone: the fused tile kernels next to the same formula composed from
max_pool1d, conv1d and autograd (Limiter.torch_forward) in the same session (a measurement, not a test).

Two legs on 256 stereo items of 131072 samples: D = 239 with H = 0, and D = 239 with H = 2400 (the default 240 Hann taps).
One JSON line per (leg, path) with

    ms            forward + backward of ``route(x, log_ceiling).sum()``, a host clock around ``--steps`` steps that ends in
                  a device synchronise, per step; the median of ``--repeats`` rounds that alternate the two paths
    peak_MiB      torch.cuda.max_memory_allocated over one step, minus what was allocated before it (x, the parameter)

for path "fused" (csrc/limiter.hip through autograd.LimiterFn) and "composed".  Further lines give the two entries alone
under the launch hook of ops (HIP events around each call), with the bytes of their HBM bounds (8 per sample and channel
forward, 12 backward) and the fraction of 8 TB/s they make of them.

    python tools/limiter_timing.py [--steps 5] [--repeats 5] [--legs short hold]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (256, 2, 131072)
HBM_PEAK = 8e12          # bytes per second, the MI355X's specification
LEGS = {"short": (239, 0), "hold": (239, 2400)}


def clocked(fn, steps):
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3 / steps


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", nargs="+", choices=sorted(LEGS), default=["short", "hold"])
    ap.add_argument("--no-composed", action="store_true", help="the fused path and the entries only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("limiter_timing: no GPU -- a time taken anywhere else says nothing")

    import grafx_amd.processors as P
    from grafx_amd import ops

    R, C, L = SHAPE
    for leg in args.legs:
        D, H = LEGS[leg]
        m = P.Limiter(D, H, compensate_delay=True).cuda()
        what = f"Limiter(lookahead={D}, hold={H})"
        g = torch.Generator(device="cuda").manual_seed(R)
        x = torch.randn(R, C, L, device="cuda", generator=g) * 0.1
        x[..., L // 3:L // 2] *= 5.0                              # a stretch well above the ceiling, the rest mostly under it
        x.requires_grad_(True)
        lc = torch.full((R, 1), -1.6, device="cuda").requires_grad_(True)
        routes = {"fused": m}
        if not args.no_composed:
            routes["composed"] = m.torch_forward
        leaves = [x, lc]

        def step_of(route):
            def step():
                for t in leaves:
                    t.grad = None
                route(x, lc).sum().backward()

            return step

        steps = {path: step_of(route) for path, route in routes.items()}
        outs, grads, peaks, times = {}, {}, {}, {path: [] for path in steps}
        for path, step in steps.items():
            step()                                               # warm-up: code objects, the allocator's blocks
            grads[path] = [t.grad.clone() for t in leaves]
            with torch.no_grad():
                outs[path] = routes[path](x, lc)
            for t in leaves:
                t.grad = None                                    # (the peak counts the gradients)
            peaks[path] = peak_of(step)
        for _ in range(args.repeats):
            for path, step in steps.items():
                times[path].append(clocked(step, args.steps))
        err = gerr = None
        if "composed" in outs:   # faster and different is not faster: the two routes agree at the size they are timed at
            err = float((outs["fused"] - outs["composed"]).abs().max() / outs["composed"].abs().max())
            gerr = [float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads["fused"], grads["composed"])]
        for path in steps:
            t = times[path]
            print(json.dumps({"leg": what, "shape": [R, C, L], "taps": m.window.numel(), "tile": ops.limiter_tile(D + 1 + H),
                              "path": path, "steps": args.steps, "repeats": len(t), "ms": round(sorted(t)[len(t) // 2], 3),
                              "min_max_ms": [round(min(t), 3), round(max(t), 3)], "peak_MiB": round(peaks[path], 1),
                              "x_MiB": round(R * C * L * 4 / 2**20, 1), "out_peak_rel_fused_vs_composed": err,
                              "grad_peak_rel_fused_vs_composed": gerr}), flush=True)
        del outs, grads
        # the entries alone
        xd, ld, gy = x.detach(), lc.detach(), torch.ones(R, C, L, device="cuda")
        n = max(args.steps, 5)
        with ops.profiling() as prof:
            for _ in range(n):
                ops.limiter(xd, ld, m.window, D, H, compensate=True)
                ops.limiter_bwd(xd, gy, ld, m.window, D, H, compensate=True)
        torch.cuda.synchronize()
        for name, calls in prof.items():
            ms = sorted(a.elapsed_time(b) for a, b, _ in calls)[len(calls) // 2]
            print(json.dumps({"leg": what, "path": "fused", "entry": name, "ms": round(ms, 4), "bound_bytes": calls[0][2],
                              "bound_ms_at_8TBs": round(calls[0][2] / HBM_PEAK * 1e3, 4),
                              "fraction_of_8TBs": round(calls[0][2] / (ms * 1e-3) / HBM_PEAK, 3)}), flush=True)
        del x, xd, steps, routes, leaves, lc, ld, gy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
