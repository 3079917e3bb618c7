"""Forward + backward of an oversampled distortion alone: the fused tile kernels next to the same formula composed from the
native polyphase and waveshaper nodes in the same session (a measurement, not a test).

Two legs on 256 stereo items of 131072 samples at F = 4: TanhDistortion() and ChebyshevDistortion(max_order=10).  One
JSON line per (leg, path) with

    ms            forward + backward of ``route(x, **parameters).sum()``, a host clock around ``--steps`` steps that ends in
                  a device synchronise, per step; the median of ``--repeats`` rounds that alternate the two paths
    peak_MiB      torch.cuda.max_memory_allocated over one step, minus what was allocated before it (x, the parameters)

for path "fused" (csrc/oversampled.hip through autograd.OversampledWaveshaperFn: the module with ``oversample=4``) and
"composed": UpfirdnFn (interpolate by 4) -> WaveshaperFn (the module with ``oversample=1``) -> UpfirdnFn (decimate by 4),
each a native kernel, the two signals at four times the rate written to memory and read back, and u kept on autograd's
tape.  Further lines give the entries alone under the launch hook of ops (HIP events around each call), fused and composed,
with the bytes of the fused pass's HBM bound (8 per sample forward, 12 backward) and the fraction of 8 TB/s the fused
entries make of it.

    python tools/oversampled_timing.py [--steps 5] [--repeats 5] [--legs tanh cheb] [--factor 4]
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
LEGS = {"tanh": ("TanhDistortion()", "TanhDistortion", {}), "cheb": ("ChebyshevDistortion(max_order=10)", "ChebyshevDistortion",
                                                                  {"max_order": 10})}


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
    ap.add_argument("--legs", nargs="+", choices=sorted(LEGS), default=["tanh", "cheb"])
    ap.add_argument("--factor", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("oversampled_timing: no GPU -- a time taken anywhere else says nothing")

    import grafx_amd.processors as P
    from grafx_amd import ops
    from grafx_amd.autograd import UpfirdnFn

    R, C, L = SHAPE
    F = args.factor
    for leg in args.legs:
        what, cls, kw = LEGS[leg]
        fused, plain = getattr(P, cls)(oversample=F, **kw).cuda(), getattr(P, cls)(**kw).cuda()
        h_up, o_up, h_dn, o_dn = fused.os_h_up, fused.os_offset_up, fused.os_h_dn, fused.os_offset_dn
        g = torch.Generator(device="cuda").manual_seed(R)
        x = (torch.rand(R, C, L, device="cuda", generator=g) * 1.1 - 0.55).requires_grad_(True)
        ps = {k: (-(0.5 * torch.randn(R, n, device="cuda", generator=g)).abs()).requires_grad_(True)
              for k, n in fused.parameter_size().items()}

        def composed(t, **p):
            u = UpfirdnFn.apply(t, h_up, F, 1, o_up, F * L)
            return UpfirdnFn.apply(plain(u, **p), h_dn, 1, F, o_dn, L)

        routes = {"fused": fused, "composed": composed}
        leaves = [x, *ps.values()]

        def step_of(route):
            def step():
                for t in leaves:
                    t.grad = None
                route(x, **ps).sum().backward()

            return step

        steps = {path: step_of(route) for path, route in routes.items()}
        outs, grads, peaks, times = {}, {}, {}, {path: [] for path in steps}
        for path, step in steps.items():
            step()                                               # warm-up: code objects, the allocator's blocks
            grads[path] = [t.grad.clone() for t in leaves]
            with torch.no_grad():
                outs[path] = routes[path](x, **ps)
            for t in leaves:
                t.grad = None                                    # (the peak counts the gradients)
            peaks[path] = peak_of(step)
        for _ in range(args.repeats):
            for path, step in steps.items():
                times[path].append(clocked(step, args.steps))
        # faster and different is not faster: the two routes agree at the size they are timed at
        err = float((outs["fused"] - outs["composed"]).abs().max() / outs["composed"].abs().max())
        gerr = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads["fused"], grads["composed"]))
        for path in steps:
            t = times[path]
            print(json.dumps({"leg": what, "shape": [R, C, L], "factor": F, "taps": [h_up.numel(), h_dn.numel()], "path": path,
                              "steps": args.steps, "repeats": len(t), "ms": round(sorted(t)[len(t) // 2], 3),
                              "min_max_ms": [round(min(t), 3), round(max(t), 3)], "peak_MiB": round(peaks[path], 1),
                              "x_MiB": round(R * C * L * 4 / 2**20, 1), "out_peak_rel_fused_vs_composed": err,
                              "grad_peak_rel_fused_vs_composed": gerr}), flush=True)
        del outs, grads
        # the entries alone
        xd, pd = x.detach(), {k: v.detach() for k, v in ps.items()}
        mode = ops.WS_TANH if leg == "tanh" else ops.WS_CHEBYSHEV
        names = {"log_pre_gain": pd["log_pre_gain"], "p0": pd.get("basis_weights")}
        cfg = dict(inverse_post_gain=leg == "tanh")
        gy = torch.ones_like(xd)
        n = max(args.steps, 5)
        with ops.profiling() as prof:
            for _ in range(n):
                ops.oversampled_waveshaper(xd, mode, F, h_up, o_up, h_dn, o_dn, **names, **cfg)
                ops.oversampled_waveshaper_bwd(xd, gy, mode, F, h_up, o_up, h_dn, o_dn, **names, **cfg)
        torch.cuda.synchronize()
        for name, calls in prof.items():
            ms = sorted(a.elapsed_time(b) for a, b, _ in calls)[len(calls) // 2]
            print(json.dumps({"leg": what, "path": "fused", "entry": name, "ms": round(ms, 4), "bound_bytes": calls[0][2],
                              "bound_ms_at_8TBs": round(calls[0][2] / HBM_PEAK * 1e3, 4),
                              "fraction_of_8TBs": round(calls[0][2] / (ms * 1e-3) / HBM_PEAK, 3)}), flush=True)
        with ops.profiling() as prof:
            for _ in range(n):
                u = ops.upfirdn(xd, h_up, F, 1, o_up, n_out=F * L)
                v = ops.waveshaper(u, mode, **names, **cfg)
                ops.upfirdn(v, h_dn, 1, F, o_dn, n_out=L)
                gv = ops.upfirdn(gy, h_dn.flip(0), F, 1, h_dn.numel() - 1 - o_dn, n_out=F * L)
                gu, _ = ops.waveshaper_bwd(u, gv, mode, **names, **cfg)
                ops.upfirdn(gu, h_up.flip(0), 1, F, h_up.numel() - 1 - o_up, n_out=L)
                del u, v, gv, gu
        torch.cuda.synchronize()
        for name, calls in prof.items():
            per_step = len(calls) // n
            ms = sum(sorted(a.elapsed_time(b) for a, b, _ in calls[i::per_step])[n // 2] for i in range(per_step))
            print(json.dumps({"leg": what, "path": "composed", "entry": name, "calls_per_step": per_step, "ms_per_step": round(ms, 4)}),
                  flush=True)
        del x, xd, steps, routes, leaves, ps, pd, gy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
