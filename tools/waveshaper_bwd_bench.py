"""Forward + backward of the memoryless distortions: the native autograd node against the torch twin (torch_forward under
autograd) on the same tensors, interleaved rounds in one process, and the native node alone at the console shape.

    python tools/waveshaper_bwd_bench.py [rows_compare=512] [rows_native=8192] [rounds=5]

Prints one line per mode and shape: median and minimum milliseconds, and for the native node the share of the HBM roofline
on 20 B per channel-sample (forward 8 B: read x, write y; backward 12 B: read x and gy, write gx)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import grafx_amd.processors as P  # noqa: E402

HBM_PEAK_GBS = 8000.0   # the specification figure bench.py prices its rooflines on
C, L = 2, 131072

MODES = [
    ("TanhDistortion", lambda: P.TanhDistortion()),
    ("PiecewiseTanhDistortion", lambda: P.PiecewiseTanhDistortion()),
    ("ChebyshevDistortion(10)", lambda: P.ChebyshevDistortion(max_order=10)),
    ("ChebyshevDistortion(32, tanh)", lambda: P.ChebyshevDistortion(max_order=32, use_tanh=True)),
]


def tensors(m, R):
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(R, C, L, device="cuda") * 1.8 - 0.9
    ps = {k: (torch.randn(R, n, generator=gen) * 0.5).cuda() for k, n in m.parameter_size().items()}
    if "basis_weights" in ps:
        ps["log_pre_gain"] = -ps["log_pre_gain"].abs()
    return x.requires_grad_(), {k: v.requires_grad_() for k, v in ps.items()}, torch.randn(R, C, L, device="cuda")


def step(fn, x, ps, gy):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    grads = torch.autograd.grad(fn(x, **ps), [x, *ps.values()], gy)
    b.record()
    torch.cuda.synchronize()
    del grads
    return a.elapsed_time(b)


def main():
    rows_cmp = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    rows_nat = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    fmt = lambda t: f"median {statistics.median(t):8.3f} ms  min {min(t):8.3f} ms"  # noqa: E731
    for name, make in MODES:
        m = make().cuda()
        if rows_cmp:
            x, ps, gy = tensors(m, rows_cmp)
            times = {"native": [], "twin": []}
            for r in range(rounds + 1):                     # (round 0 warms both up)
                for key, fn in (("native", m), ("twin", m.torch_forward)):
                    t = step(fn, x, ps, gy)
                    if r:
                        times[key].append(t)
            print(f"{name:30s} R={rows_cmp:5d}  native {fmt(times['native'])} | torch twin {fmt(times['twin'])} | "
                  f"x{statistics.median(times['twin']) / statistics.median(times['native']):.1f}", flush=True)
            del x, ps, gy
            torch.cuda.empty_cache()
        if rows_nat:
            x, ps, gy = tensors(m, rows_nat)
            t = [step(m, x, ps, gy) for _ in range(rounds + 1)][1:]
            floor = 20 * rows_nat * C * L / (HBM_PEAK_GBS * 1e6)
            print(f"{name:30s} R={rows_nat:5d}  native {fmt(t)} | {floor / statistics.median(t):.2f} of the HBM roofline "
                  f"(20 B per channel-sample over {HBM_PEAK_GBS / 1000:.0f} TB/s = {floor:.2f} ms)", flush=True)
            del x, ps, gy
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
