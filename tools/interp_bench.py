#!/usr/bin/env python3
"""interp_bench.py — settled, in-process timing of the interpolator (if_fir_interp_t).

Cases: 255 taps, L in {2, 4, 8, 16, 64}, 2^28 outputs, float32 input; the overlap-save kernel's small form (L >= 4) and its
full form (every L).  Per case: ms per call (median of --reps timed calls after --warmup), GS/s of outputs, and the bytes
moved (N*8 in + N*L*8 out) as a fraction of the 8 TB/s roofline.  For comparison in the same run: the decimator at D = 1 (the
full-rate pipeline) on 2^28 samples.  Ends with one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8e12


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
    ap.add_argument("--outputs", type=int, default=1 << 28)
    ap.add_argument("--taps", type=int, default=255)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=0, help="run only this L (0 = all)")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    M = args.outputs
    out = torch.empty(2 * M, dtype=torch.float32, device="cuda")
    x = torch.empty(2 * M, dtype=torch.float32, device="cuda")  # big enough for every L and for the decimator
    side = torch.cuda.Stream()  # the contexts run on the stream the events are recorded on (not the null stream: handle 0
    torch.cuda.set_stream(side)  # would select a context's own stream)
    stream = side.cuda_stream
    with fir.IfFir(fir.bpf_design(args.taps), decimation=1, max_samples=1024) as f:
        f.set_stream(stream)
        f.synth_device(x.data_ptr(), 0, M, 0)
        torch.cuda.synchronize()
        rows = []
        if not args.only:
            ms = timed(torch, lambda: f.process_device(x.data_ptr(), out.data_ptr(), M), args.warmup, args.reps)
            rows.append({"case": "decimator D=1", "L": 1, "form": "dec1", "ms": ms, "gsps": M / ms / 1e6,
                         "roofline": 16.0 * M / (ms * 1e-3) / ROOF})
    for L in (2, 4, 8, 16, 64):
        if args.only and L != args.only:
            continue
        n = M // L
        h = (fir.bpf_design(args.taps, 0.0, 0.45 / L) * L).astype("float32")
        with fir.IfFirInterp(h, L, max_samples=1024, dev=True) as f:
            f.set_stream(stream)
            for form in (("small", "full") if L >= 4 else ("full",)):
                f.debug_config(force_full=(form == "full"))
                ms = timed(torch, lambda: f.process_device(x.data_ptr(), out.data_ptr(), n), args.warmup, args.reps)
                rows.append({"case": "interp L=%d %s" % (L, form), "L": L, "form": form, "ms": ms, "gsps": M / ms / 1e6,
                             "roofline": (8.0 * n + 8.0 * M) / (ms * 1e-3) / ROOF})
    for r in rows:
        print("%-22s %9.4f ms  %7.2f GS/s out  %.3f of 8 TB/s" % (r["case"], r["ms"], r["gsps"], r["roofline"]))
    res = {"outputs": M, "taps": args.taps, "rows": rows}
    small = {r["L"]: r["ms"] for r in rows if r["form"] == "small"}
    full = {r["L"]: r["ms"] for r in rows if r["form"] == "full"}
    res["small_speedup"] = {str(k): full[k] / small[k] for k in small if k in full}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
