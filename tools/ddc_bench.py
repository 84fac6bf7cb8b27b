#!/usr/bin/env python3
"""ddc_bench.py — settled, in-process timing of the real-input down-converter (if_fir_ddc_t).

Cases (T, D): (255, 4), (255, 16), (255, 64), (1023, 8), (1023, 64); float32 and int16 input, 2^28 real samples (--samples),
an NCO at 0.2 cycles/sample.  Per case: ms per if_fir_ddc_process_device call (median, fastest and slowest of --reps timed
calls after --warmup, HIP events on a side stream), input GS/s, and the bytes the call must move, (4 + 8 / D) N -- (2 + 8 / D) N
for int16 --, as a fraction of the 8 TB/s roofline.  Beside it, in the same run and on the same data: the chain it replaces,
a widening pass r -> (r, 0) in torch followed by IfFir with set_nco on the overlap-save backend (float32: one copy of the real
tensor into a complex64 one; int16: a strided copy of r into the I halves of a buffer whose Q halves were zeroed once, outside
the timing -- the cheaper form).  Ends with one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8e12
CASES = ((255, 4), (255, 16), (255, 64), (1023, 8), (1023, 64))
FREQ = 0.2


def timed(torch, fn, warmup, reps):
    """(median, fastest, slowest) ms"""
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
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 28)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="run only this case (index; -1 = all)")
    ap.add_argument("--no-chain", action="store_true", help="time the down-converter alone")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()  # the contexts run on the stream the events are recorded on (not the null stream: handle 0
    torch.cuda.set_stream(side)  # would select a context's own stream)
    stream = side.cuda_stream
    n = args.samples - args.samples % 64   # whole decimation periods: the timed calls are one stream continued
    r32 = torch.empty(n, dtype=torch.float32, device="cuda")
    with fir.IfFir(fir.bpf_design(255), decimation=1, max_samples=1024) as f:
        f.set_stream(stream)
        f.synth_device(r32.data_ptr(), 0, n // 2, 0)   # the I, Q values of the synthetic stream read as n real samples
        f.synchronize()
    r16 = (r32 * 14000.0).round().to(torch.int16)
    rows = []
    for idx, (T, D) in enumerate(CASES):
        if args.only >= 0 and idx != args.only:
            continue
        h = fir.bpf_design(T, 0.0, 0.45 / D)
        outs = n // D
        out = torch.empty(2 * outs + 16, dtype=torch.float32, device="cuda")
        for i16 in (False, True):
            src = r16 if i16 else r32
            row = {"taps": T, "D": D, "input": "int16" if i16 else "float32", "samples": n}
            with fir.IfFirDdc(h, D, max_samples=1024) as f:
                f.set_stream(stream)
                f.set_nco(FREQ)
                if i16:
                    f.set_input_format(fir.INPUT_I16)

                def one():
                    assert f.process_device(src.data_ptr(), out.data_ptr(), n) == outs

                row["ms"], row["ms_min"], row["ms_max"] = timed(torch, one, args.warmup, args.reps)
            row["gsps_in"] = n / row["ms"] / 1e6
            row["roofline"] = ((2.0 if i16 else 4.0) + 8.0 / D) * n / (row["ms"] * 1e-3) / ROOF
            if not args.no_chain:
                wide = torch.zeros(2 * n, dtype=torch.int16 if i16 else torch.float32, device="cuda")
                wide_i = wide.view(n, 2)[:, 0]
                wide_c = None if i16 else torch.view_as_complex(wide.view(n, 2))
                with fir.IfFir(h, decimation=D, max_samples=1024) as d:
                    d.set_stream(stream)
                    if i16:
                        d.set_input_format(fir.INPUT_I16)
                    d.set_nco(FREQ)
                    assert d.get_backend() == fir.BACKEND_HIP_FFT

                    def widen():
                        if i16:
                            wide_i.copy_(src)
                        else:
                            wide_c.copy_(src)

                    def chain():
                        widen()
                        assert d.process_device(wide.data_ptr(), out.data_ptr(), n) == outs

                    row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = timed(torch, chain, args.warmup, args.reps)
                    row["widen_ms"] = timed(torch, widen, args.warmup, args.reps)[0]
                del wide, wide_i, wide_c
                row["speedup_vs_chain"] = row["chain_ms"] / row["ms"]
            rows.append(row)
    print("%-10s %-8s %11s %9s %17s %8s %9s %10s %17s %9s %8s" % ("taps /D", "input", "samples", "ms", "[min, max]", "GS/s in", "of 8TB/s",
                                                                "chain ms", "[min, max]", "widen ms", "speedup"))
    for r in rows:
        line = "%4d /%-4d %-8s %11d %9.4f [%7.4f,%7.4f] %8.1f %9.3f" % (r["taps"], r["D"], r["input"], r["samples"], r["ms"], r["ms_min"],
                                                                      r["ms_max"], r["gsps_in"], r["roofline"])
        if "chain_ms" in r:
            line += " %10.4f [%7.4f,%7.4f] %9.4f %8.2f" % (r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"], r["widen_ms"],
                                                          r["speedup_vs_chain"])
        print(line)
    print(json.dumps({"samples_requested": args.samples, "warmup": args.warmup, "reps": args.reps, "nco": FREQ, "rows": rows}))


if __name__ == "__main__":
    main()
