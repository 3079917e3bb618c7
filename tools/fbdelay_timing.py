"""Forward + backward of the feedback delay alone: the native recursive walk next to the same formula composed from a
chunk loop of torch ops and autograd (FeedbackDelay.torch_forward) in the same session (a measurement, not a test).

Two legs on 256 stereo items of 131072 samples of white noise, every parameter drawn N(0, 1): the default constructor
(delays of 64 .. 22050 samples), and min_delay=64, max_delay=128, the short-chunk worst case of the walk.  One JSON line
per (leg, path) with

    ms            forward + backward of ``route(x, **z).sum()`` with all gradients, a host clock around ``--steps`` steps
                  that ends in a device synchronise, per step; the median of ``--repeats`` rounds that alternate the paths
    peak_MiB      torch.cuda.max_memory_allocated over one step, minus what was allocated before it (x, the parameters)
    rows          the batch the path was timed at: the composed route falls back to the largest power-of-two batch it can
                  hold (``--composed-rows`` caps it), and its ``ms_per_row`` is what compares

for path "fused" (csrc/fbdelay.hip through autograd.FeedbackDelayFn) and "composed", and the largest disagreement of the
two routes' outputs and gradients at the composed batch, each against the composed tensor's peak.  Further lines give the
two entries alone under the launch hook of ops (HIP events around each call), with the steps of the walk
(ceil(L / K), K = min(floor(min delay of the row), FBDELAY_CHUNK), the largest over the rows) and the time per step.

    python tools/fbdelay_timing.py [--steps 3] [--repeats 3] [--legs default short] [--composed-rows 256]
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
LEGS = {"default": dict(), "short": dict(min_delay=64, max_delay=128)}


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
    ap.add_argument("--legs", nargs="+", choices=sorted(LEGS), default=["default", "short"])
    ap.add_argument("--composed-rows", type=int, default=SHAPE[0], help="the largest batch the composed route is tried at")
    ap.add_argument("--no-composed", action="store_true", help="the fused path and the entries only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fbdelay_timing: no GPU -- a time taken anywhere else says nothing")

    import grafx_amd.processors as P
    from grafx_amd import ops

    R, C, L = SHAPE
    for leg in args.legs:
        m = P.FeedbackDelay(**LEGS[leg]).cuda()
        what = f"FeedbackDelay({', '.join(f'{k}={v}' for k, v in LEGS[leg].items())})"
        g = torch.Generator(device="cuda").manual_seed(R)
        x = torch.randn(R, C, L, device="cuda", generator=g).requires_grad_(True)
        z = {k: torch.randn(R, n, device="cuda", generator=g).requires_grad_(True) for k, n in m.parameter_size().items()}

        def step_of(route, rows):
            xs, zs = x[:rows].detach().requires_grad_(True), {k: v[:rows].detach().requires_grad_(True) for k, v in z.items()}

            def step():
                for t in (xs, *zs.values()):
                    t.grad = None
                route(xs, **zs).sum().backward()

            return step, xs, zs

        routes = {"fused": (m, R)}
        if not args.no_composed:
            rows = min(R, args.composed_rows)
            while rows >= 1:                                     # the largest batch the composed route holds
                try:
                    step, _, _ = step_of(m.torch_forward, rows)
                    step()
                    break
                except torch.cuda.OutOfMemoryError:
                    rows //= 2
                finally:
                    step = None
                    torch.cuda.empty_cache()
            if rows >= 1:
                routes["composed"] = (m.torch_forward, rows)
        steps, outs, grads, peaks, times = {}, {}, {}, {}, {path: [] for path in routes}
        small = routes.get("composed", (None, R))[1]
        for path, (route, rows) in routes.items():
            step, xs, zs = step_of(route, rows)
            steps[path] = step
            step()                                               # warm-up: code objects, the allocator's blocks
            for t in (xs, *zs.values()):
                t.grad = None                                    # (the peak counts the gradients)
            peaks[path] = peak_of(step)
            cstep, cx, cz = step_of(route, small)                # what the two routes are compared at
            cstep()
            grads[path] = [t.grad.clone() for t in (cx, *cz.values())]
            with torch.no_grad():
                outs[path] = route(cx.detach(), **{k: v.detach() for k, v in cz.items()})
            del cstep, cx, cz
            torch.cuda.empty_cache()
        for _ in range(args.repeats):
            for path, step in steps.items():
                times[path].append(clocked(step, args.steps))
        err = gerr = None
        if "composed" in outs:   # faster and different is not faster: the two routes agree at the size they are compared at
            err = float((outs["fused"] - outs["composed"]).abs().max() / outs["composed"].abs().max())
            gerr = {n: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
                    for n, a, b in zip(("x", *z), grads["fused"], grads["composed"])}
        with torch.no_grad():
            params = m.physical(**z)
        K = params[0].floor().amin(-1).clamp_max(ops.FBDELAY_CHUNK)
        walk_steps = int(torch.ceil(L / K).max())
        for path, (_, rows) in routes.items():
            t = times[path]
            ms = sorted(t)[len(t) // 2]
            print(json.dumps({"leg": what, "shape": [rows, C, L], "path": path, "rows": rows, "steps": args.steps,
                              "repeats": len(t), "ms": round(ms, 3), "ms_per_row": round(ms / rows, 4),
                              "min_max_ms": [round(min(t), 3), round(max(t), 3)], "peak_MiB": round(peaks[path], 1),
                              "x_MiB": round(rows * C * L * 4 / 2**20, 1), "min_delay_drawn": round(float(params[0].min()), 1),
                              "walk_steps_longest_row": walk_steps, "compared_at_rows": small,
                              "out_peak_rel_fused_vs_composed": err, "grad_peak_rel_fused_vs_composed": gerr}), flush=True)
        del outs, grads, steps
        # the entries alone
        xd, gy = x.detach(), torch.ones(R, C, L, device="cuda")
        n = max(args.steps, 5)
        with ops.profiling() as prof:
            for _ in range(n):
                _, (q, w) = ops.fbdelay(xd, *params, m.max_delay, tape=True)
                ops.fbdelay_bwd(xd, gy, q, w, *params, m.max_delay)
        torch.cuda.synchronize()
        for name, calls in prof.items():
            ms = sorted(a.elapsed_time(b) for a, b, _ in calls)[len(calls) // 2]
            print(json.dumps({"leg": what, "path": "fused", "entry": name, "ms": round(ms, 4), "walk_steps_longest_row": walk_steps,
                              "us_per_walk_step": round(ms * 1e3 / walk_steps, 3)}), flush=True)
        del x, xd, z, params, gy, q, w, routes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
