"""Forward + backward of the modulated delay line alone: the fused tile kernels next to the same formula composed from
an index tensor, gathers and autograd (ModulatedDelay.torch_forward) in the same session (a measurement, not a test).

Two legs on 256 stereo items of 131072 samples: four voices on a delay line of 1764 samples with cubic interpolation, and
one voice on a line of 8192 samples with linear interpolation.  One JSON line per (leg, path) with

    ms            forward + backward of ``route(x, **z).sum()``, a host clock around ``--steps`` steps that ends in a device
                  synchronise, per step; the median of ``--repeats`` rounds that alternate the two paths
    peak_MiB      torch.cuda.max_memory_allocated over one step, minus what was allocated before it (x, the parameters)

for path "fused" (csrc/moddelay.hip through autograd.ModulatedDelayFn) and "composed", and the largest disagreement of the
two routes' outputs and gradients, each against the composed tensor's peak.  Further lines give the two entries alone
under the launch hook of ops (HIP events around each call), with the bytes of their HBM bounds (8 per sample and channel
forward, 12 backward) and the fraction of 8 TB/s they make of them.

    python tools/moddelay_timing.py [--steps 3] [--repeats 3] [--legs chorus long]
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
LEGS = {"chorus": (4, 1764, "cubic"), "long": (1, 8192, "linear")}      # voices, max_delay, interpolation
NAMES = ("x", "z_delay", "z_depth", "z_rate", "phase", "log_gain", "log_dry")


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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", nargs="+", choices=sorted(LEGS), default=["chorus", "long"])
    ap.add_argument("--no-composed", action="store_true", help="the fused path and the entries only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moddelay_timing: no GPU -- a time taken anywhere else says nothing")

    import grafx_amd.processors as P
    from grafx_amd import ops

    R, C, L = SHAPE
    for leg in args.legs:
        V, Dmax, interp = LEGS[leg]
        m = P.ModulatedDelay(V, 16, Dmax, interpolation=interp).cuda()
        what = f"ModulatedDelay(num_voices={V}, max_delay={Dmax}, interpolation={interp!r})"
        g = torch.Generator(device="cuda").manual_seed(R)
        x = torch.randn(R, C, L, device="cuda", generator=g).requires_grad_(True)
        z = [torch.randn(R, V, device="cuda", generator=g), torch.randn(R, V, device="cuda", generator=g),
             torch.randn(R, V, device="cuda", generator=g), torch.rand(R, V, C, device="cuda", generator=g),
             0.3 * torch.randn(R, V, C, device="cuda", generator=g) - 0.7, 0.3 * torch.randn(R, 1, device="cuda", generator=g)]
        z = [t.requires_grad_(True) for t in z]
        leaves = [x, *z]
        routes = {"fused": m}
        if not args.no_composed:
            routes["composed"] = m.torch_forward

        def step_of(route):
            def step():
                for t in leaves:
                    t.grad = None
                route(x, *z).sum().backward()

            return step

        steps = {path: step_of(route) for path, route in routes.items()}
        outs, grads, peaks, times = {}, {}, {}, {path: [] for path in steps}
        for path, step in steps.items():
            step()                                               # warm-up: code objects, the allocator's blocks
            grads[path] = [t.grad.clone() for t in leaves]
            with torch.no_grad():
                outs[path] = routes[path](x, *z)
            for t in leaves:
                t.grad = None                                    # (the peak counts the gradients)
            peaks[path] = peak_of(step)
            torch.cuda.empty_cache()
        for _ in range(args.repeats):
            for path, step in steps.items():
                times[path].append(clocked(step, args.steps))
        err = gerr = None
        if "composed" in outs:   # faster and different is not faster: the two routes agree at the size they are timed at
            err = float((outs["fused"] - outs["composed"]).abs().max() / outs["composed"].abs().max())
            gerr = {n: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
                    for n, a, b in zip(NAMES, grads["fused"], grads["composed"])}
        with torch.no_grad():
            delay, depth, rate = (t.double() for t in m.physical(*z)[:3])
        for path in steps:
            t = times[path]
            print(json.dumps({"leg": what, "shape": [R, C, L], "tile": ops.moddelay_tile(Dmax, C), "path": path,
                              "steps": args.steps, "repeats": len(t), "ms": round(sorted(t)[len(t) // 2], 3),
                              "min_max_ms": [round(min(t), 3), round(max(t), 3)], "peak_MiB": round(peaks[path], 1),
                              "x_MiB": round(R * C * L * 4 / 2**20, 1), "mean_delay": round(float(delay.mean()), 1),
                              "mean_depth": round(float(depth.mean()), 1), "max_slope": round(float((6.283185307 * rate * depth).max()), 3),
                              "out_peak_rel_fused_vs_composed": err, "grad_peak_rel_fused_vs_composed": gerr}), flush=True)
        del outs, grads
        # the entries alone
        with torch.no_grad():
            params = m.physical(*z)
        xd, gy = x.detach(), torch.ones(R, C, L, device="cuda")
        n = max(args.steps, 5)
        with ops.profiling() as prof:
            for _ in range(n):
                ops.moddelay(xd, *params, Dmax, interp)
                ops.moddelay_bwd(xd, gy, *params, Dmax, interp)
        torch.cuda.synchronize()
        for name, calls in prof.items():
            ms = sorted(a.elapsed_time(b) for a, b, _ in calls)[len(calls) // 2]
            print(json.dumps({"leg": what, "path": "fused", "entry": name, "ms": round(ms, 4), "bound_bytes": calls[0][2],
                              "bound_ms_at_8TBs": round(calls[0][2] / HBM_PEAK * 1e3, 4),
                              "fraction_of_8TBs": round(calls[0][2] / (ms * 1e-3) / HBM_PEAK, 3)}), flush=True)
        del x, xd, steps, routes, leaves, z, params, gy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
