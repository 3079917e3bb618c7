"""Forward + backward of the multi-resolution STFT loss alone: the native kernels next to the torch.stft chain (a measurement,
not a test).

The module's default resolutions (1024/256, 2048/512, 512/128), stereo with sum_and_difference=True -- four rows per graph
-- at bench.py's signal length.  One JSON line per (batch, path) with

    ms            forward + backward of ``loss(pred, target)``, a host clock around ``--steps`` steps that ends in a device
                  synchronise, per step; the median of ``--repeats`` rounds (and their minimum and maximum)
    peak_MiB      torch.cuda.max_memory_allocated over one step, minus what was allocated before it (pred, target)

for path "native" (MultiResolutionSTFTLoss.forward) and "torch" (MultiResolutionSTFTLoss.torch_forward: what a user of
torch.stft runs).  The torch path is tried from the largest batch of ``--batches`` down and measured at the first one that
fits in memory; the native path is measured there (the shared batch: the rounds alternate the two paths, so that they share
whatever else the machine is doing) and at the first batch of the list alone.

``--scale mel --n-bins N`` measures the loss on a mel scale instead (N Slaney bands per resolution at ``--sample-rate``):
the native path is then csrc/stft_band_loss.hip, the torch path the same formula through torch.stft and a matmul.

    python tools/stft_loss_timing.py [--batches 256 128 64 32 16 8] [--length 131072] [--steps 5] [--repeats 5] [--native-only]
                                     [--scale mel --n-bins 64 [--sample-rate 44100]]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 128, 64, 32, 16, 8])
    ap.add_argument("--length", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--native-only", action="store_true", help="stop after the first batch on the native path (for a profile)")
    ap.add_argument("--scale", choices=["mel"], default=None, help="compare filterbank bands instead of bins")
    ap.add_argument("--n-bins", type=int, default=64,
                    help="bands per resolution with --scale (at 44.1 kHz the 512-point resolution has bins for 80 at most)")
    ap.add_argument("--sample-rate", type=int, default=44100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stft_loss_timing: no GPU -- a time taken anywhere else says nothing")

    from grafx_amd.losses import MultiResolutionSTFTLoss

    scale = {} if args.scale is None else {"scale": args.scale, "n_bins": args.n_bins, "sample_rate": args.sample_rate}
    module = MultiResolutionSTFTLoss(sum_and_difference=True, **scale).cuda()

    def signals(batch):
        g = torch.Generator(device="cuda").manual_seed(batch)
        target = torch.randn(batch, 2, args.length, device="cuda", generator=g)
        pred = (0.5 * target + 0.02 * torch.randn(batch, 2, args.length, device="cuda", generator=g)).requires_grad_(True)
        return pred, target

    def step_of(path, pred, target):
        loss_fn = module if path == "native" else module.torch_forward

        def step():
            pred.grad = None
            loss_fn(pred, target).backward()

        return step

    def report(batch, path, times, peak, extra=None):
        row = {"batch": batch, "rows": 4 * batch, "length": args.length, "path": path, "steps": args.steps, "repeats": len(times),
               "ms": round(sorted(times)[len(times) // 2], 3), "min_max_ms": [round(min(times), 3), round(max(times), 3)],
               "peak_MiB": round(peak, 1)}
        row.update(scale)
        row.update(extra or {})
        print(json.dumps(row), flush=True)

    # the largest batch alone, native
    first = args.batches[0]
    pred, target = signals(first)
    step = step_of("native", pred, target)
    step()                                                   # warm-up: code objects, the allocator's blocks
    peak = peak_of(step)
    report(first, "native", [clocked(step, args.steps) for _ in range(args.repeats)], peak)
    del pred, target, step
    torch.cuda.empty_cache()
    if args.native_only:
        return

    # the shared batch: the largest at which the torch chain fits
    for batch in args.batches:
        pred, target = signals(batch)
        torch_step = step_of("torch", pred, target)
        try:
            torch_step()
            torch_peak = peak_of(torch_step)
        except torch.OutOfMemoryError:
            print(json.dumps({"batch": batch, "path": "torch", "fits": False}), flush=True)
            pred.grad = None
            del pred, target, torch_step
            torch.cuda.empty_cache()
            continue
        want = pred.grad.clone()
        native_step = step_of("native", pred, target)
        native_step()
        # faster and different is not faster: the two paths give the same gradient at the size they are timed at
        err = float((pred.grad - want).abs().max() / want.abs().max())
        native_peak = peak_of(native_step)
        times = {"native": [], "torch": []}
        for _ in range(args.repeats):
            times["native"].append(clocked(native_step, args.steps))
            times["torch"].append(clocked(torch_step, args.steps))
        report(batch, "native", times["native"], native_peak, {"grad_peak_rel_vs_torch": err})
        report(batch, "torch", times["torch"], torch_peak, {"fits": True})
        break


if __name__ == "__main__":
    main()
