"""Per-block time of the streamed ballistics console next to the one-call render (a measurement, not a test).

The 32-strip / 4-bus console of the benchmark's shape with "ballistics" compressors (the "iir" smoother does not stream):
one call over the whole signal, then the same signal in blocks through render_grafx(state=, return_state=True).

    python tools/stream_console_timing.py [--batch 4] [--length 131072] [--block 16384] [--repeats 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_console(n_ch=32, n_bus=4):
    from grafx_amd.data import GRAFX, NodeConfigs

    G = GRAFX(config=NodeConfigs(["eq", "compressor", "reverb"]))
    out_id = G.add("out")
    buses = [G.add("mix") for _ in range(n_bus)]
    send = G.add("mix")
    for ch in range(n_ch):
        _, last = G.add_serial_chain(["in", "eq", "compressor"])
        G.connect(last, buses[ch // (n_ch // n_bus)])
        G.connect(last, send)
    for b in buses:
        e, c = G.add("eq"), G.add("compressor")
        G.connect(b, e)
        G.connect(e, c)
        G.connect(c, out_id)
    r = G.add("reverb")
    G.connect(send, r)
    G.connect(r, out_id)
    return G


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--length", type=int, default=131072)
    ap.add_argument("--block", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    from grafx_amd.data import convert_to_tensor
    from grafx_amd.processors import Compressor, ParametricEqualizer, STFTMaskedNoiseReverb
    from grafx_amd.processors.core.convolution import exact_convolution_scope
    from grafx_amd.render import prepare_render, render_grafx, reorder_for_fast_render
    from grafx_amd.utils import create_empty_parameters

    procs = {"eq": ParametricEqualizer(flashfftconv=False).cuda(),
             "compressor": Compressor(energy_smoother="ballistics", flashfftconv=False).cuda(),
             "reverb": STFTMaskedNoiseReverb(flashfftconv=False).cuda()}
    G = build_console()
    rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam")).to("cuda")
    torch.manual_seed(0)
    params = {t: {k: v.detach().cuda() for k, v in d.items()} for t, d in create_empty_parameters(procs, G, std=0.3).items()}
    x = 0.3 * torch.randn(args.batch, 32, 2, args.length, device="cuda")
    cuts = [(a, min(a + args.block, args.length)) for a in range(0, args.length, args.block)]

    def one_call():
        return render_grafx(procs, x, params, rd, keep_signal_buffer=False)[0]

    def streamed():
        state, out = None, []
        for a, b in cuts:
            y, _, _, state = render_grafx(procs, x[..., a:b], params, rd, keep_signal_buffer=False, state=state,
                                          return_state=True)
            out.append(y)
        return out

    with torch.no_grad(), exact_convolution_scope(True):
        whole = timed(one_call, args.repeats)
        blocks = timed(streamed, args.repeats)
        err = float((torch.cat(streamed(), -1) - one_call()).abs().max() / one_call().abs().max())
    print(json.dumps({"batch": args.batch, "length": args.length, "block": args.block, "blocks": len(cuts),
                      "one_call_ms": round(whole, 3), "streamed_total_ms": round(blocks, 3),
                      "streamed_per_block_ms": round(blocks / len(cuts), 3), "peak_rel_difference": err}))


if __name__ == "__main__":
    main()
