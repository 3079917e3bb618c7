"""Forward + backward of the filtered-noise-shaping tap synthesis alone, from the parameters to dL/d(parameters) for a fixed
cotangent of the normalised taps: the native node (autograd.NoiseShapingIrFn) against the chain of torch ops it replaced
(FilteredNoiseShapingReverb.torch_compute_ir + normalize_impulse), on the same tensors, alternating in one process.

    python tools/noise_shaping_ir_bwd_bench.py [rounds=7] [rows ...=1 256]

ir_len = 60000, 12 bands, two channels (upstream's defaults), noise_randomness="fixed" so that both paths read the same
noise; with and without fade-in.  R = 1 is a batch-shared reverb, R = 256 per-graph parameters.  Device events around work
that ends in a synchronise; round 0 warms both paths up.  Prints per shape and path the median, the minimum and the spread
(max - min) in milliseconds and torch.cuda.max_memory_allocated over the path's rounds (bytes above what was allocated before
the first round); for the native path also the backward entry alone (ops.noise_shaping_ir_bwd: both kernels of
gfx_noise_shaping_ir_bwd_f32 and the wrapper's allocations) with its rate over the bytes it must move -- grad_ir and ir
once from memory, and with the noise (C K ir_len floats, read once per row, from cache) counted as well."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from grafx_amd import ops  # noqa: E402
from grafx_amd.processors import FilteredNoiseShapingReverb  # noqa: E402
from grafx_amd.processors.core.utils import normalize_impulse  # noqa: E402

IR_LEN, BANDS = 60000, 12


def step(fn, ps, gh):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    grads = torch.autograd.grad(fn(**ps), list(ps.values()), gh)
    b.record()
    torch.cuda.synchronize()
    del grads
    return a.elapsed_time(b)


def entry_alone(m, ps, gh, rounds):
    """Milliseconds of ops.noise_shaping_ir_bwd alone (both kernels), on the taps and gains of the forward; one warm-up."""
    with torch.no_grad():
        q = {k: v.detach() for k, v in ps.items()}
        noise = m.get_filtered_noise()[0]
        ir = ops.noise_shaping_ir(noise, q["log_decay"], q["log_gain"], q.get("log_fade_in"), q.get("z_fade_in_gain"),
                                  IR_LEN, m.min_decay, m.max_decay)
        gain = torch.rsqrt((ir * ir).sum(-1, keepdim=True).mean(-2, keepdim=True) + 1e-12)
        out = []
        for r in range(rounds + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.noise_shaping_ir_bwd(gh, noise, q["log_decay"], q["log_gain"], q.get("log_fade_in"), q.get("z_fade_in_gain"),
                                     m.min_decay, m.max_decay, ir=ir, row_gain=gain)
            b.record()
            torch.cuda.synchronize()
            if r:
                out.append(a.elapsed_time(b))
    return out


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    rows = [int(a) for a in sys.argv[2:]] or [1, 256]
    for fade in (False, True):
        m = FilteredNoiseShapingReverb(ir_len=IR_LEN, num_bands=BANDS, noise_randomness="fixed", use_fade_in=fade,
                                       flashfftconv=False).cuda()
        C = m.num_channels
        paths = {
            "native": lambda **p: m._taps(p["log_decay"], p["log_gain"], p.get("log_fade_in"), p.get("z_fade_in_gain"), True),
            "torch chain": lambda **p: normalize_impulse(m.torch_compute_ir(**p)),
        }
        for R in rows:
            gen = torch.Generator().manual_seed(0)
            ps = {k: torch.randn(R, *shape, generator=gen).cuda().requires_grad_() for k, shape in m.parameter_size().items()}
            gh = torch.randn(R, C, IR_LEN, generator=gen).cuda()
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
            tag = f"fade={int(fade)} R={R:4d}"
            for key, t in times.items():
                print(f"{tag}  {key:12s} median {statistics.median(t):9.3f} ms  min {min(t):9.3f} ms  "
                      f"spread {max(t) - min(t):8.3f} ms  peak {peak[key]:13d} B", flush=True)
            print(f"{tag}  torch chain / native = "
                  f"{statistics.median(times['torch chain']) / statistics.median(times['native']):.2f}", flush=True)
            kernel = entry_alone(m, ps, gh, rounds)
            k_ms = statistics.median(kernel)
            signal, noise = 2 * 4 * R * C * IR_LEN, 4 * R * C * BANDS * IR_LEN
            print(f"{tag}  backward entry median {k_ms:9.3f} ms  min {min(kernel):9.3f} ms: grad_ir + ir {signal / 1e6:.1f} MB "
                  f"-> {signal / k_ms / 1e6:.1f} GB/s; with the noise once per row {(signal + noise) / 1e6:.1f} MB "
                  f"-> {(signal + noise) / k_ms / 1e6:.1f} GB/s", flush=True)
            del ps, gh
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
