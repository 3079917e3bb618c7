"""Time of one block of a streamed causal convolution, two ways:
   python tools/fftconv_state_bench.py [--rows 512] [--taps 4000 60000] [--blocks 4096 16384] [--iters 20] [--repeats 3]
"cat": the route without the state entry -- torch.cat([history, x]) followed by ops.fftconv(off = N - 1, Lout = L), the
next history sliced from the concatenation (runs on any commit); "state": ops.fftconv_state with preallocated output and
state buffers (gfx_fftconv_state_f32; skipped where the library has no such entry).  Stereo rows, one filter per row.
-> ms per call, the repeats' values and their spread, and the kernel that ran."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from grafx_amd import ops  # noqa: E402
from grafx_amd._lib import lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=512)
ap.add_argument("--taps", type=int, nargs="+", default=[4000, 60000])
ap.add_argument("--blocks", type=int, nargs="+", default=[4096, 16384])
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
torch.manual_seed(0)
R, C = a.rows, 2


def timed(fn):
    for _ in range(3):
        fn()
    out = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / a.iters)
    return out


for N in a.taps:
    h = torch.randn(R * C, N, device="cuda") / N**0.5
    Hs = ops.fir_spectrum(h)
    for L in a.blocks:
        x = torch.randn(R, C, L, device="cuda")
        hist = torch.randn(R, C, N - 1, device="cuda")

        def cat_route():
            xx = torch.cat([hist, x], -1)
            y = ops.fftconv(xx, Hs, N, C, Lout=L, off=N - 1)
            return y, xx[..., L:]

        rows = [("cat", timed(cat_route), lib().gfx_fftconv_last_kernel().decode())]
        if hasattr(ops, "fftconv_state"):
            out, zf = torch.empty(R, C, L, device="cuda"), torch.empty_like(hist)

            def state_route():
                return ops.fftconv_state(x, Hs, N, C, zi=hist, out=out, zf=zf)

            rows.append(("state", timed(state_route), lib().gfx_fftconv_last_kernel().decode()))
            y0, z0 = cat_route()
            err = float((out - y0).abs().max() / y0.abs().max())
            assert torch.equal(zf, z0) and err < 1e-5, err
        for name, ms, kernel in rows:
            print(f"N={N} L={L} rows={R}x{C} {name:5s}: median {sorted(ms)[len(ms) // 2]:.3f} ms "
                  f"[{', '.join(f'{m:.3f}' for m in ms)}] spread {max(ms) - min(ms):.3f} ms  ({kernel})")
