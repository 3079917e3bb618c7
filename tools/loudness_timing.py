"""Forward + backward of IntegratedLoudness alone: the native kernels next to the route composed of what the package had
before them (a measurement, not a test).

Two workloads: (a) the training leg, 256 stereo items of 131072 samples at 44.1 kHz; (b) one stereo item of 2^23 samples
at 48 kHz.  One JSON line per (workload, path) with

    ms            forward + backward of ``meter(x).sum()``, a host clock around ``--steps`` steps that ends in a device
                  synchronise, per step; the median of ``--repeats`` rounds that alternate the two paths (minimum, maximum)
    peak_MiB      torch.cuda.max_memory_allocated over one step, minus what was allocated before it (x)

for path "native" (IntegratedLoudness.forward: csrc/loudness.hip, double) and "composed": autograd.BiquadCascadeFn
(ops.biquad_cascade and its native backward, float32) on k_weighting cast to float32, then square, reshape-sum,
gated_loudness and torch autograd.  The composed route is the yardstick of the times.  The last lines give both routes'
sub-block energies, and the gradient of their sum, on white noise and on the bass input (0.5 sin 30 Hz + 1e-3 noise) at
44.1 kHz against scipy.signal.lfilter in float64, peak-relative per row-channel, the worst one.

    python tools/loudness_timing.py [--steps 5] [--repeats 5] [--workloads a b]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"a": (256, 2, 131072, 44100), "b": (1, 2, 1 << 23, 48000)}


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


def composed_energies(x, meter):
    """The sub-block sums of squares (R, C, n_sub) float64 by the float32 cascade and torch ops."""
    from grafx_amd.autograd import BiquadCascadeFn
    from grafx_amd.loudness import k_weighting

    Bs, As = (t.float().to(x.device).expand(x.shape[0], 1, 2, 3).contiguous() for t in k_weighting(meter.sample_rate))
    y = BiquadCascadeFn.apply(x, Bs, As)
    n_sub = x.shape[-1] // meter.hop
    return y[..., :n_sub * meter.hop].square().view(*x.shape[:-1], n_sub, meter.hop).sum(-1).double()


def composed_loudness(x, meter):
    from grafx_amd.loudness import gated_loudness

    return gated_loudness(composed_energies(x, meter) / meter.hop, meter.block_hops, (1.0,) * x.shape[-2],
                          meter.absolute_gate, meter.relative_gate).to(x.dtype)


def errors(kind):
    """Both routes against float64 on one small input: the sub-block energies and the gradient of their sum."""
    import numpy as np
    from scipy.signal import lfilter

    from grafx_amd import ops
    from grafx_amd.loudness import IntegratedLoudness, k_weighting

    fs, L = 44100, 131072
    meter = IntegratedLoudness(fs)
    g = torch.Generator().manual_seed(30)
    x = torch.randn(2, 2, L, generator=g, dtype=torch.float64)
    if kind == "bass":
        phase = torch.rand(2, 2, 1, generator=g, dtype=torch.float64)
        x = 0.5 * torch.sin(2 * math.pi * (30.0 * torch.arange(L, dtype=torch.float64) / fs + phase)) + 1e-3 * x
    x = x.float()

    def k_filter(v):
        for b, a in zip(*k_weighting(fs)):
            v = lfilter(b.numpy(), a.numpy(), v, axis=-1)
        return v

    n_sub = L // meter.hop
    y = k_filter(x.double().numpy())
    y[..., n_sub * meter.hop:] = 0.0
    want = torch.from_numpy(np.square(y[..., :n_sub * meter.hop]).reshape(2, 2, n_sub, meter.hop).sum(-1))
    want_grad = torch.from_numpy(k_filter(2.0 * y[..., ::-1])[..., ::-1].copy())

    def worst(got, ref):
        return float(((got.cpu() - ref).abs().amax(-1) / ref.abs().amax(-1)).max())

    xg = x.cuda().requires_grad_(True)
    composed = composed_energies(xg, meter)
    (composed_grad,) = torch.autograd.grad(composed.sum(), xg)
    native = ops.kweight_energy(xg.detach(), meter.coef, meter.hop)
    native_grad = ops.kweight_energy_bwd(xg.detach(), meter.coef, torch.ones_like(native), meter.hop)
    return {"input": f"{kind}, 44.1 kHz, (2, 2, 131072)",
            "yardstick": "scipy.signal.lfilter, float64, worst row-channel peak-relative",
            "native_energy": worst(native, want), "composed_energy": worst(composed.detach(), want),
            "native_gradient": worst(native_grad, want_grad), "composed_gradient": worst(composed_grad, want_grad)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", nargs="+", choices=sorted(WORKLOADS), default=sorted(WORKLOADS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loudness_timing: no GPU -- a time taken anywhere else says nothing")

    from grafx_amd.loudness import IntegratedLoudness

    for name in args.workloads:
        B, C, L, fs = WORKLOADS[name]
        meter = IntegratedLoudness(fs)
        g = torch.Generator(device="cuda").manual_seed(B)
        x = (0.1 * torch.randn(B, C, L, device="cuda", generator=g)).requires_grad_(True)

        def step_of(route):
            def step():
                x.grad = None
                route(x).sum().backward()

            return step

        steps = {"native": step_of(meter), "composed": step_of(lambda t: composed_loudness(t, meter))}
        grads, peaks, times = {}, {}, {"native": [], "composed": []}
        for path, step in steps.items():
            step()                                               # warm-up: code objects, the allocator's blocks
            grads[path] = x.grad.clone()
            x.grad = None                                        # (the peak counts the gradient)
            peaks[path] = peak_of(step)
        for _ in range(args.repeats):
            for path, step in steps.items():
                times[path].append(clocked(step, args.steps))
        # faster and different is not faster: the two routes give the same gradient at the size they are timed at
        err = float((grads["native"] - grads["composed"]).abs().max() / grads["composed"].abs().max())
        for path in steps:
            t = times[path]
            print(json.dumps({"workload": name, "shape": [B, C, L], "sample_rate": fs, "path": path, "steps": args.steps,
                              "repeats": len(t), "ms": round(sorted(t)[len(t) // 2], 3),
                              "min_max_ms": [round(min(t), 3), round(max(t), 3)], "peak_MiB": round(peaks[path], 1),
                              "x_MiB": round(B * C * L * 4 / 2**20, 1), "grad_peak_rel_native_vs_composed": err}), flush=True)
        # the entries behind the two routes called alone under the launch hook of ops (HIP events around each call)
        from grafx_amd import ops
        from grafx_amd.loudness import k_weighting

        xd = x.detach()
        Bs, As = (t.float().cuda().expand(B, 1, 2, 3).contiguous() for t in k_weighting(fs))
        with ops.profiling() as prof:
            for _ in range(args.steps):
                e = ops.kweight_energy(xd, meter.coef, meter.hop)
                g = ops.kweight_energy_bwd(xd, meter.coef, torch.ones_like(e), meter.hop)
                y = ops.biquad_cascade(xd, Bs, As)
                g = ops.biquad_cascade_bwd(xd, y, Bs, As, want=("x",))[0]
        torch.cuda.synchronize()
        print(json.dumps({"workload": name, "entries_ms": {
            k: round(sorted(a.elapsed_time(b) for a, b, _ in v)[len(v) // 2], 3) for k, v in prof.items()}}), flush=True)
        del xd, e, g, y
        del x, steps, grads
        torch.cuda.empty_cache()
    for kind in ("noise", "bass"):
        print(json.dumps(errors(kind)), flush=True)


if __name__ == "__main__":
    main()
