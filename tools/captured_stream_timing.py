"""Per-block time of the streamed ballistics console: eager blocks next to the captured stream (a measurement, not a test).

The 32-strip / 4-bus console of tools/stream_console_timing.py (default tap counts: a 4000-tap equaliser, a 60 000-tap
reverb), one JSON line per (batch, block length) with the milliseconds per block of

    eager_ms            render_grafx(state=, return_state=True) from state=None: the stream as it renders without this tool's
                        classes (the first block takes the stateless kernels, every later one the state kernels)
    eager_silent_ms     the same loop started from silent_state(...): the state kernels from the first block on
    captured_ms         CapturedStream: one graph replay per block, the filter designs hoisted out of it
    captured_update_ms  CapturedStream with update_parameters() before every block: the design graph replayed per block

Every figure is a host clock around ``--blocks`` blocks that ends in a device synchronise, the median of ``--repeats``
rounds; a round times the four cases one after the other, so that they share whatever else the machine is doing.

    python tools/captured_stream_timing.py [--batches 1 4] [--block-lengths 512 16384] [--blocks 100] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def clocked(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--block-lengths", type=int, nargs="+", default=[512, 16384])
    ap.add_argument("--blocks", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    from stream_console_timing import build_console

    from grafx_amd.data import convert_to_tensor
    from grafx_amd.processors import Compressor, ParametricEqualizer, STFTMaskedNoiseReverb
    from grafx_amd.processors.core._buffer_io import carry_leaves
    from grafx_amd.render import CapturedStream, prepare_render, render_grafx, reorder_for_fast_render, silent_state
    from grafx_amd.utils import create_empty_parameters

    procs = {"eq": ParametricEqualizer(flashfftconv=False).cuda(),
             "compressor": Compressor(energy_smoother="ballistics", flashfftconv=False).cuda(),
             "reverb": STFTMaskedNoiseReverb(flashfftconv=False).cuda()}
    G = build_console()
    rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam")).to("cuda")
    torch.manual_seed(0)
    params = {t: {k: v.detach().cuda() for k, v in d.items()} for t, d in create_empty_parameters(procs, G, std=0.3).items()}

    for batch in args.batches:
        for n in args.block_lengths:
            ring = [0.3 * torch.randn(batch, 32, 2, n, device="cuda") for _ in range(8)]     # the blocks, over and over
            with torch.no_grad():
                silent = silent_state(procs, ring[0], params, rd)
                stream = CapturedStream(procs, ring[0], params, rd, keep_signal_buffer=False)

                def eager(state):
                    for k in range(args.blocks):
                        _, _, _, state = render_grafx(procs, ring[k % 8], params, rd, keep_signal_buffer=False, state=state,
                                                      return_state=True)
                    return state

                def captured(update):
                    stream.reset()
                    for k in range(args.blocks):
                        if update:
                            stream.update_parameters(params)
                        stream(ring[k % 8])

                cases = {"eager_ms": lambda: eager(None), "eager_silent_ms": lambda: eager(silent),
                         "captured_ms": lambda: captured(False), "captured_update_ms": lambda: captured(True)}
                # the captured stream computes the eager stream from silent_state, bit for bit
                want = eager(silent)
                captured(False)
                got = stream.state()
                same = all(torch.equal(a, b) for i in want.carries
                           for a, b in zip(carry_leaves(want.carries[i]), carry_leaves(got.carries[i])))
                times = {name: [] for name in cases}
                for _ in range(args.repeats):
                    for name, fn in cases.items():
                        times[name].append(clocked(fn) / args.blocks)
            row = {"batch": batch, "block": n, "blocks": args.blocks, "repeats": args.repeats,
                   "designed_steps": len(stream.designed), "state_bit_equal": same}
            for name, ts in times.items():
                row[name] = round(sorted(ts)[len(ts) // 2], 4)
                row[name.replace("_ms", "_min_max_ms")] = [round(min(ts), 4), round(max(ts), 4)]
            print(json.dumps(row), flush=True)
            del stream


if __name__ == "__main__":
    main()
