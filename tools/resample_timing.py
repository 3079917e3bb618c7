"""Forward + backward of Resample and TruePeak alone: the native polyphase kernel next to the same formula composed from
torch ops in the same session (a measurement, not a test).

Three legs on 256 stereo items of 131072 samples: Resample(44100, 48000), Resample(48000, 16000) and TruePeak().  One JSON
line per (leg, path) with

    ms            forward + backward of ``route(x).sum()``, a host clock around ``--steps`` steps that ends in a device
                  synchronise, per step; the median of ``--repeats`` rounds that alternate the two paths (minimum, maximum)
    peak_MiB      torch.cuda.max_memory_allocated over one step, minus what was allocated before it (x)

for path "native" (csrc/upfirdn.hip through autograd.UpfirdnFn / UpfirdnAbsmaxFn) and "composed": the phase bank
g_ph[j] = h[ph down + offset - j up] as the ``up`` output channels of one strided ``conv1d`` (stride ``down``), the channels
interleaved into the output, and for the peak ``abs().amax()`` of that, under torch autograd.  The composed route is the
yardstick of the times.  A last line per leg gives the native entry alone under the launch hook of ops (HIP events around
each call): its time, the bytes of the HBM bound 4 R C (L + M) (4 R C L for the peak, which writes no signal) and the
fraction of 8 TB/s that makes.

    python tools/resample_timing.py [--steps 5] [--repeats 5] [--legs up down peak]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (256, 2, 131072)
HBM_PEAK = 8e12          # bytes per second, the MI355X's specification
LEGS = {"up": ("Resample(44100, 48000)", 44100, 48000), "down": ("Resample(48000, 16000)", 48000, 16000),
        "peak": ("TruePeak()", 1, 4)}


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


def phase_bank(h, up, down, offset, device="cuda"):
    """-> (G (up, 1, K) float32 on the GPU, jmin): g_ph[j - jmin] = h[ph down + offset - j up], zero outside the taps."""
    N = h.numel()
    jmin, jmax = -((N - 1 - offset) // up), ((up - 1) * down + offset) // up
    j = torch.arange(jmin, jmax + 1)
    idx = torch.arange(up)[:, None] * down + offset - j[None, :] * up
    G = torch.where((idx >= 0) & (idx < N), h.cpu()[idx.clamp(0, N - 1)], torch.zeros(()))
    return G[:, None, :].float().to(device), jmin


def composed_upfirdn(x, bank, up, down, M):
    """y[i up + ph] = sum_j x[i down + j] g_ph[j]: one conv1d with ``up`` output channels and stride ``down``."""
    G, jmin = bank
    L, K = x.shape[-1], G.shape[-1]
    frames = -(-M // up)
    right = max(0, (frames - 1) * down + K - (L - jmin))
    y = F.conv1d(F.pad(x.reshape(-1, 1, L), (-jmin, right)), G, stride=down)[..., :frames]
    return y.transpose(1, 2).reshape(*x.shape[:-1], frames * up)[..., :M]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", nargs="+", choices=sorted(LEGS), default=["up", "down", "peak"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resample_timing: no GPU -- a time taken anywhere else says nothing")

    from grafx_amd import ops
    from grafx_amd.loudness import TruePeak
    from grafx_amd.resample import Resample

    B, C, L = SHAPE
    for leg in args.legs:
        what, orig, new = LEGS[leg]
        g = torch.Generator(device="cuda").manual_seed(B)
        x = (0.1 * torch.randn(B, C, L, device="cuda", generator=g)).requires_grad_(True)
        if leg == "peak":
            mod = TruePeak().cuda()
            up, down, M = mod.oversample, 1, mod.oversample * L
            bank = phase_bank(mod.taps, up, down, mod.offset)
            routes = {"native": mod.channel_peaks, "composed": lambda t: composed_upfirdn(t, bank, up, down, M).abs().amax(-1)}
        else:
            mod = Resample(orig, new).cuda()
            up, down, M = mod.up, mod.down, -(-L * mod.up // mod.down)
            bank = phase_bank(mod.taps, up, down, mod.offset)
            routes = {"native": mod, "composed": lambda t: composed_upfirdn(t, bank, up, down, M)}

        def step_of(route):
            def step():
                x.grad = None
                route(x).sum().backward()

            return step

        steps = {path: step_of(route) for path, route in routes.items()}
        outs, grads, peaks, times = {}, {}, {}, {path: [] for path in steps}
        for path, step in steps.items():
            step()                                               # warm-up: code objects, the allocator's blocks
            grads[path] = x.grad.clone()
            with torch.no_grad():
                outs[path] = routes[path](x)
            x.grad = None                                        # (the peak counts the gradient)
            peaks[path] = peak_of(step)
        for _ in range(args.repeats):
            for path, step in steps.items():
                times[path].append(clocked(step, args.steps))
        # faster and different is not faster: the two routes agree at the size they are timed at
        err = float((outs["native"] - outs["composed"]).abs().max() / outs["composed"].abs().max())
        gerr = float((grads["native"] - grads["composed"]).abs().max() / grads["composed"].abs().max())
        for path in steps:
            t = times[path]
            print(json.dumps({"leg": what, "shape": [B, C, L], "up": up, "down": down, "taps": mod.taps.numel(), "n_out": M,
                              "path": path, "steps": args.steps, "repeats": len(t), "ms": round(sorted(t)[len(t) // 2], 3),
                              "min_max_ms": [round(min(t), 3), round(max(t), 3)], "peak_MiB": round(peaks[path], 1),
                              "x_MiB": round(B * C * L * 4 / 2**20, 1), "out_peak_rel_native_vs_composed": err,
                              "grad_peak_rel_native_vs_composed": gerr}), flush=True)
        del outs, grads
        xd = x.detach()
        with ops.profiling() as prof:
            for _ in range(max(args.steps, 5)):
                if leg == "peak":
                    ops.upfirdn_absmax(xd, mod.taps, up, down, mod.offset, n_out=M)
                else:
                    y = ops.upfirdn(xd, mod.taps, up, down, mod.offset, n_out=M)
                    ops.upfirdn(y, mod.taps.flip(0), down, up, mod.taps.numel() - 1 - mod.offset, n_out=L)
        torch.cuda.synchronize()
        for name, calls in prof.items():
            for direction, part in (("forward", calls[0::2]), ("backward", calls[1::2])) if leg != "peak" else (("forward", calls),):
                ms = sorted(a.elapsed_time(b) for a, b, _ in part)[len(part) // 2]
                nbytes = part[0][2]
                print(json.dumps({"leg": what, "entry": name, "direction": direction, "ms": round(ms, 4), "bound_bytes": nbytes,
                                  "bound_ms_at_8TBs": round(nbytes / HBM_PEAK * 1e3, 4),
                                  "fraction_of_8TBs": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}), flush=True)
        del x, xd, steps, routes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
