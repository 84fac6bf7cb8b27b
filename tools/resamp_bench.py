#!/usr/bin/env python3
"""resamp_bench.py — settled, in-process timing of the rational resampler (if_fir_resamp_t).

Cases (L, M, T): (2, 3, 63), (3, 4, 95), (25, 24, 801), (1, 4, 255); float32 input, 2^26 input samples (fewer where the
interpolate-then-decimate chain's L-times intermediate would pass --max-intermediate samples; the size used is reported).
Per case: ms per call (median of --reps timed calls after --warmup, HIP events on a side stream), input GS/s, and the bytes
the resampler must move, (8 + 8 L / M) N, as a fraction of the 8 TB/s roofline.  Beside it, in the same run and on the same
data: the chain users had before, IfFirInterp(h, L) followed by IfFir([1.0], decimation=M) (two launches and an intermediate
stream at L times the input rate), and for (1, 4) the decimator's AUTO route (informational: its overlap-save kernel is expected
to win there).  Ends with one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8e12
CASES = ((2, 3, 63), (3, 4, 95), (25, 24, 801), (1, 4, 255))


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--max-intermediate", type=int, default=1 << 29, help="most samples of the chain's L-times stream")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="run only this case (index; -1 = all)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()  # the contexts run on the stream the events are recorded on (not the null stream: handle 0
    torch.cuda.set_stream(side)  # would select a context's own stream)
    stream = side.cuda_stream
    x = torch.empty(2 * args.samples, dtype=torch.float32, device="cuda")
    with fir.IfFir(fir.bpf_design(255), decimation=1, max_samples=1024) as f:
        f.set_stream(stream)
        f.synth_device(x.data_ptr(), 0, args.samples, 0)
        f.synchronize()
    rows = []
    for idx, (L, M, T) in enumerate(CASES):
        if args.only >= 0 and idx != args.only:
            continue
        n = min(args.samples, args.max_intermediate // L)
        n -= n % M   # whole periods: every call of the stream then starts on phase 0 and emits n L / M outputs, so the timed
        #              calls are one stream continued, with no reset (a host-side wait) between them
        h = (fir.bpf_design(T, 0.0, 0.45 / max(L, M)) * L).astype(np.float32)
        outs = n * L // M
        out = torch.empty(2 * outs + 16, dtype=torch.float32, device="cuda")
        row = {"L": L, "M": M, "taps": T, "samples": n}
        with fir.IfFirResamp(h, L, M, max_samples=1024) as f:
            f.set_stream(stream)

            def one():
                assert f.process_device(x.data_ptr(), out.data_ptr(), n) == outs

            row["ms"] = timed(torch, one, args.warmup, args.reps)
        row["gsps_in"] = n / row["ms"] / 1e6
        row["roofline"] = (8.0 + 8.0 * L / M) * n / (row["ms"] * 1e-3) / ROOF
        mid = torch.empty(2 * n * L, dtype=torch.float32, device="cuda")
        with fir.IfFirInterp(h, L, max_samples=1024) as up, \
                fir.IfFir(np.ones(1, dtype=np.float32), decimation=M, max_samples=1024) as down:
            up.set_stream(stream)
            down.set_stream(stream)

            def chain():
                up.process_device(x.data_ptr(), mid.data_ptr(), n)
                assert down.process_device(mid.data_ptr(), out.data_ptr(), n * L) == outs

            row["chain_ms"] = timed(torch, chain, args.warmup, args.reps)
            row["chain_interp_backend"], row["chain_decimator_backend"] = up.get_backend(), down.get_backend()
        del mid
        row["speedup_vs_chain"] = row["chain_ms"] / row["ms"]
        if L == 1:
            with fir.IfFir(h, decimation=M, max_samples=1024) as d:
                d.set_stream(stream)

                def dec():
                    assert d.process_device(x.data_ptr(), out.data_ptr(), n) == outs

                row["decimator_auto_ms"] = timed(torch, dec, args.warmup, args.reps)
        rows.append(row)
    print("%-14s %10s %10s %9s %9s %10s %8s" % ("L/M taps", "samples", "ms", "GS/s in", "of 8TB/s", "chain ms", "speedup"))
    for r in rows:
        print("%2d/%-2d %-8d %10d %10.4f %9.2f %9.3f %10.4f %8.2f%s" % (
            r["L"], r["M"], r["taps"], r["samples"], r["ms"], r["gsps_in"], r["roofline"], r["chain_ms"], r["speedup_vs_chain"],
            "   (decimator AUTO route: %.4f ms)" % r["decimator_auto_ms"] if "decimator_auto_ms" in r else ""))
    print(json.dumps({"samples_requested": args.samples, "warmup": args.warmup, "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
