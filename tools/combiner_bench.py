#!/usr/bin/env python3
"""combiner_bench.py — settled, in-process timing of the channel combiner (if_fir_combiner_t) against the
chain it replaces.

Cases: 255 taps, 2^28 outputs, float32 input, (C, L) in {(2, 4), (8, 16), (16, 16), (64, 64)}, centres off the 1/4096 grid.
The chain: C interpolator contexts (if_fir_interp_t) with their NCOs at the centres on one stream, each writing a full-rate
stream, then torch additions into one buffer.  Both run in this process on the same inputs, settled first and then timed in
alternation (combiner, chain, combiner, ...), the median of --reps calls each.  Per case: ms per call, GS/s of outputs, the
bytes the combiner has to move (C*N*8 in + N*L*8 out) as a fraction of the 8 TB/s roofline, and the chain's time over the
combiner's.  Ends with one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8e12
CASES = ((2, 4), (8, 16), (16, 16), (64, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outputs", type=int, default=1 << 28)
    ap.add_argument("--taps", type=int, default=255)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", type=int, default=0, help="run only the case with this many channels (0 = all)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    M = args.outputs
    side = torch.cuda.Stream()  # the contexts run on the stream the events are recorded on
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    out = torch.empty(2 * M, dtype=torch.float32, device="cuda")
    tmp = torch.empty(2 * M, dtype=torch.float32, device="cuda")   # the chain's full-rate stream of one channel
    acc = torch.empty(2 * M, dtype=torch.float32, device="cuda")   # the chain's sum
    rows = []
    for C, L in CASES:
        if args.only and C != args.only:
            continue
        n = M // L
        h = (fir.bpf_design(args.taps, 0.0, 0.45 / L) * L).astype("float32")
        centres = -0.45 + 0.9 * (np.arange(C) + 0.5) / C + 0.3 / 4096
        xs = torch.empty(C, 2 * n, dtype=torch.float32, device="cuda")
        with fir.IfFir(fir.bpf_design(args.taps), decimation=1, max_samples=1024) as s:
            s.set_stream(stream)
            for c in range(C):
                s.synth_device(xs[c].data_ptr(), 0, n, c)
            s.synchronize()
        comb = fir.IfFirCombiner(h, L, centres, max_samples=1024)
        comb.set_stream(stream)
        chain = [fir.IfFirInterp(h, L, max_samples=1024) for _ in range(C)]
        for f, fc in zip(chain, centres):
            f.set_stream(stream)
            f.set_nco(fc)
        ptrs = [xs[c].data_ptr() for c in range(C)]

        def run_combiner():
            comb.process_device(ptrs, out.data_ptr(), n)

        def run_chain():
            chain[0].process_device(ptrs[0], acc.data_ptr(), n)
            for c in range(1, C):
                chain[c].process_device(ptrs[c], tmp.data_ptr(), n)
                acc.add_(tmp)

        for _ in range(args.warmup):
            run_combiner()
            run_chain()
        torch.cuda.synchronize()
        diff = ((out - acc).abs().max() / acc.abs().max()).item()   # the two compute the same stream
        ms = {"combiner": [], "chain": []}
        for _ in range(args.reps):
            for name, fn in (("combiner", run_combiner), ("chain", run_chain)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        comb.close()
        for f in chain:
            f.close()
        rows.append({"C": C, "L": L, "combiner_ms": med["combiner"], "chain_ms": med["chain"], "combiner_gsps": M / med["combiner"] / 1e6,
                     "chain_gsps": M / med["chain"] / 1e6, "roofline": (8.0 * C * n + 8.0 * M) / (med["combiner"] * 1e-3) / ROOF,
                     "speedup": med["chain"] / med["combiner"], "max_diff_of_peak": diff,
                     "combiner_ms_min_max": [min(ms["combiner"]), max(ms["combiner"])], "chain_ms_min_max": [min(ms["chain"]), max(ms["chain"])]})
        r = rows[-1]
        print("C=%2d L=%2d  combiner %9.4f ms %7.2f GS/s out %.3f of 8 TB/s | chain %9.4f ms %7.2f GS/s | chain/combiner %.2f | "
              "max difference %.2g of the peak" % (C, L, r["combiner_ms"], r["combiner_gsps"], r["roofline"], r["chain_ms"], r["chain_gsps"],
                                                   r["speedup"], diff), flush=True)
        del xs
    print(json.dumps({"outputs": M, "taps": args.taps, "rows": rows}))


if __name__ == "__main__":
    main()
