#!/usr/bin/env python3
"""arb_bench.py — settled, in-process timing of the arbitrary-ratio resampler (if_fir_arb_t).

The case run against a baseline: b = 6 (64 phases), 1537 taps (K = 25), R = 63 * 2^26 + 1, one unit above the rational 64/63,
float32 input, 2^26 samples (--samples).  The baseline, timed alternately with it in the same process on the same data: the
rational resampler at 64/63 with the same 1537 taps -- the same K and the same bytes.  Then the steps rho ~ 0.2874, 2/3 + eps
and 3 + eps, and int16 input.  Per case: ms per process_device call (median, fastest and slowest of --reps timed calls after
--warmup, HIP events on a side stream), output MS/s, ns per output, and the bytes the call must move as a fraction of the
8 TB/s roofline.  Every timed call is one stream continued.  Ends with one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8e12
BITS, TAPS = 6, 1537
STEP_BASE = 63 * 2 ** 26 + 1
# (label, step, int16 input)
CASES = (("64/63 + 1 unit", STEP_BASE, False), ("64/63 + 1 unit", STEP_BASE, True), ("0.2874", 1234567891, False),
         ("2/3 + eps", 2863311531, False), ("3 + eps", 3 * 2 ** 32 + 1234567, False), ("3 + eps", 3 * 2 ** 32 + 1234567, True))


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()  # the contexts run on the stream the events are recorded on (not the null stream: handle 0
    torch.cuda.set_stream(side)  # would select a context's own stream)
    stream = side.cuda_stream
    n = args.samples
    x32 = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    with fir.IfFir(fir.bpf_design(255), decimation=1, max_samples=1024) as f:
        f.set_stream(stream)
        f.synth_device(x32.data_ptr(), 0, n, 0)
        f.synchronize()
    x16 = (x32 * 14000.0).round().to(torch.int16)
    rows = []

    def taps_for(step):
        return (fir.bpf_design(TAPS, 0.0, 0.45 / (64 * max(1.0, step / 2.0 ** 32))) * 64.0).astype("float32")

    for label, step, i16 in CASES:
        src = x16 if i16 else x32
        h = taps_for(step)
        cap = (n << 32) // step + 2
        out = torch.empty(2 * cap + 16, dtype=torch.float32, device="cuda")
        row = {"case": label, "bits": BITS, "taps": TAPS, "step": step, "input": "int16" if i16 else "float32", "samples": n}
        base = step == STEP_BASE and not i16
        with fir.IfFirArb(h, BITS, step, max_samples=1024) as f, fir.IfFirResamp(h, 64, 63, max_samples=1024) as r:
            f.set_stream(stream)
            r.set_stream(stream)
            if i16:
                f.set_input_format(fir.INPUT_I16)
            counts = {}

            def arb():
                counts["arb"] = f.process_device(src.data_ptr(), out.data_ptr(), n)

            def rational():
                counts["rational"] = r.process_device(src.data_ptr(), out.data_ptr(), n)

            # the two timed alternately, call by call, so that neither has the settled clock to itself
            runs = [arb, rational] if base else [arb]
            for _ in range(args.warmup):
                for fn in runs:
                    fn()
            torch.cuda.synchronize()
            ms = {fn.__name__: [] for fn in runs}
            for _ in range(args.reps):
                for fn in runs:
                    ms[fn.__name__].append(event_ms(torch, fn))
        row["ms"], row["ms_min"], row["ms_max"] = stats(ms["arb"])
        row["outputs"] = counts["arb"]
        row["ns_per_output"] = row["ms"] * 1e6 / row["outputs"]
        row["msps_out"] = row["outputs"] / row["ms"] / 1e3
        row["roofline"] = ((4.0 if i16 else 8.0) * n + 8.0 * row["outputs"]) / (row["ms"] * 1e-3) / ROOF
        if base:
            row["rational_ms"], row["rational_ms_min"], row["rational_ms_max"] = stats(ms["rational"])
            row["rational_outputs"] = counts["rational"]
            row["rational_ns_per_output"] = row["rational_ms"] * 1e6 / row["rational_outputs"]
            row["time_ratio_per_output"] = row["ns_per_output"] / row["rational_ns_per_output"]
        rows.append(row)
        del out
    print("%-15s %-8s %12s %10s %12s %9s %19s %10s %9s %9s" % ("rho", "input", "step", "samples", "outputs", "ms", "[min, max]", "ns/output",
                                                             "MS/s out", "of 8TB/s"))
    for r in rows:
        print("%-15s %-8s %12d %10d %12d %9.4f [%8.4f,%8.4f] %10.5f %9.1f %9.3f" % (r["case"], r["input"], r["step"], r["samples"], r["outputs"],
                                                                                  r["ms"], r["ms_min"], r["ms_max"], r["ns_per_output"],
                                                                                  r["msps_out"], r["roofline"]))
        if "rational_ms" in r:
            print("%-15s %-8s %12s %10d %12d %9.4f [%8.4f,%8.4f] %10.5f   <- IfFirResamp 64/63, same taps, timed alternately"
                  % ("64/63 rational", r["input"], "-", r["samples"], r["rational_outputs"], r["rational_ms"], r["rational_ms_min"],
                     r["rational_ms_max"], r["rational_ns_per_output"]))
            print("time per output, arbitrary / rational: %.2f" % r["time_ratio_per_output"])
    print(json.dumps({"samples": n, "warmup": args.warmup, "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
