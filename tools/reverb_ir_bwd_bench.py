"""Forward + backward of the STFT-masked-noise tap synthesis alone, from the parameters to dL/d(parameters) for a fixed
cotangent of the normalised left/right taps: the native node (autograd.StftReverbIrFn) against the torch chain it replaced
(_compute_ir_differentiable + ms_to_lr + normalize_impulse), on the same tensors, alternating in one process.

    python tools/reverb_ir_bwd_bench.py [rounds=7] [rows ...=1 256]

ir_len = 60000 (313 frames).  R = 1 is the console's batch-shared reverb, R = 256 per-graph parameters.  Device events
around work that ends in a synchronise; round 0 warms both paths up.  Prints per shape and path the median, the minimum and
the spread (max - min) in milliseconds and torch.cuda.max_memory_allocated over the path's rounds (bytes above what was
allocated before the first round)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from grafx_amd.processors import STFTMaskedNoiseReverb  # noqa: E402
from grafx_amd.processors.core.midside import ms_to_lr  # noqa: E402
from grafx_amd.processors.core.utils import normalize_impulse  # noqa: E402

IR_LEN = 60000


def step(fn, ps, gh):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    grads = torch.autograd.grad(fn(**ps), list(ps.values()), gh)
    b.record()
    torch.cuda.synchronize()
    del grads
    return a.elapsed_time(b)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    rows = [int(a) for a in sys.argv[2:]] or [1, 256]
    m = STFTMaskedNoiseReverb(ir_len=IR_LEN, flashfftconv=False).cuda()
    paths = {
        "native": lambda **p: m._native_taps(p["init_log_magnitude"], p["delta_log_magnitude"], None, True, True),
        "torch chain": lambda **p: normalize_impulse(ms_to_lr(m._compute_ir_differentiable(**p))),
    }
    for R in rows:
        gen = torch.Generator().manual_seed(0)
        ps = {k: torch.randn(R, *shape, generator=gen).cuda().requires_grad_() for k, shape in m.parameter_size().items()}
        gh = torch.randn(R, 2, IR_LEN, generator=gen).cuda()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        times = {k: [] for k in paths}
        peak = {k: 0 for k in paths}
        for r in range(rounds + 1):
            for key, fn in paths.items():
                torch.cuda.reset_peak_memory_stats()
                t = step(fn, ps, gh)
                if r:
                    times[key].append(t)
                    peak[key] = max(peak[key], torch.cuda.max_memory_allocated() - base)
        for key, t in times.items():
            print(f"R={R:4d}  {key:12s} median {statistics.median(t):8.3f} ms  min {min(t):8.3f} ms  "
                  f"spread {max(t) - min(t):7.3f} ms  peak {peak[key]:12d} B", flush=True)
        print(f"R={R:4d}  torch chain / native = "
              f"{statistics.median(times['torch chain']) / statistics.median(times['native']):.2f}", flush=True)
        del ps, gh
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
