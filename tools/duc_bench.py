#!/usr/bin/env python3
"""duc_bench.py — settled, in-process timing of the real-output up-converter (if_fir_duc_t).

Cases (T, L): (255, 4), (255, 8), (255, 16), (255, 64), (255, 3), (1023, 8), (1023, 64); float32 and int16 output, float32
input, 2^28 outputs (--outputs), an NCO at 0.2 cycles/sample, device-resident buffers.  Per case: ms per
if_fir_duc_process_device call (median, fastest and slowest of --reps timed calls after --warmup, HIP events on a side stream),
output GS/s, and the bytes the call must move, (8 / L + 4) per output -- (8 / L + 2) for int16 --, as a fraction of the 8 TB/s
roofline.  Beside it, alternated in the same process and on the same data: the chain it replaces, IfFirInterp with set_nco
followed by the torch pass over the L-times stream that takes the real part (int16: and scales, rounds, clamps and casts), and
that pass alone.  One more row has the NCO off, against IfFirResamp(h, L, 1) followed by the same pass.  Ends with one JSON
line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8e12
CASES = ((255, 4), (255, 8), (255, 16), (255, 64), (255, 3), (1023, 8), (1023, 64))
NCO_OFF_CASE = (255, 16)
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
    ap.add_argument("--outputs", type=int, default=1 << 28)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="run only this case (index; -1 = all)")
    ap.add_argument("--no-chain", action="store_true", help="time the up-converter alone")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()  # the contexts run on the stream the events are recorded on (not the null stream: handle 0
    torch.cuda.set_stream(side)  # would select a context's own stream)
    stream = side.cuda_stream
    n_max = args.outputs // min(L for _, L in CASES)
    x = torch.empty(2 * n_max, dtype=torch.float32, device="cuda")
    with fir.IfFir(fir.bpf_design(255), decimation=1, max_samples=1024) as f:
        f.set_stream(stream)
        f.synth_device(x.data_ptr(), 0, n_max, 0)
        f.synchronize()
    out32 = torch.empty(args.outputs + 16, dtype=torch.float32, device="cuda")
    out16 = torch.empty(args.outputs + 16, dtype=torch.int16, device="cuda")
    wide = None if args.no_chain else torch.empty(2 * args.outputs, dtype=torch.float32, device="cuda")
    rows = []
    cases = [(T, L, FREQ) for T, L in CASES] + [NCO_OFF_CASE + (0.0,)]
    for idx, (T, L, freq) in enumerate(cases):
        if args.only >= 0 and idx != args.only:
            continue
        h = fir.bpf_design(T, 0.0, 0.45 / L) * L
        n = args.outputs // L
        outs = n * L
        for o16 in (False, True):
            if not freq and o16:
                continue
            out = out16 if o16 else out32
            row = {"taps": T, "L": L, "output": "int16" if o16 else "float32", "nco": freq, "outputs": outs}
            with fir.IfFirDuc(h, L, max_samples=1024) as f:
                f.set_stream(stream)
                f.set_nco(freq)
                if o16:
                    f.set_output_format(fir.OUTPUT_I16)

                def one():
                    assert f.process_device(x.data_ptr(), out.data_ptr(), n) == outs

                row["ms"], row["ms_min"], row["ms_max"] = timed(torch, one, args.warmup, args.reps)
            row["gsps_out"] = outs / row["ms"] / 1e6
            row["roofline"] = (8.0 / L + (2.0 if o16 else 4.0)) * outs / (row["ms"] * 1e-3) / ROOF
            if not args.no_chain:
                re = wide.view(-1, 2)[:outs, 0]
                with (fir.IfFirInterp(h, L, max_samples=1024) if freq else fir.IfFirResamp(h, L, 1, max_samples=1024)) as c:
                    c.set_stream(stream)
                    if freq:
                        c.set_nco(freq)

                    def real_part():
                        if o16:
                            out[:outs].copy_((re * 32768.0).round().clamp(-32768.0, 32767.0))
                        else:
                            out[:outs].copy_(re)

                    def chain():
                        assert c.process_device(x.data_ptr(), wide.data_ptr(), n) == outs
                        real_part()

                    row["chain"] = "interp+nco" if freq else "resamp L/1"
                    row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = timed(torch, chain, args.warmup, args.reps)
                    row["pass_ms"] = timed(torch, real_part, args.warmup, args.reps)[0]
                row["speedup_vs_chain"] = row["chain_ms"] / row["ms"]
                row["slowest_beats_chain_fastest"] = bool(row["ms_max"] < row["chain_ms_min"])
            rows.append(row)
    print("%-10s %-8s %-4s %11s %9s %17s %9s %9s %10s %17s %8s %8s %6s" % ("taps xL", "output", "nco", "outputs", "ms", "[min, max]", "GS/s out",
                                                                        "of 8TB/s", "chain ms", "[min, max]", "pass ms", "speedup", "max<min"))
    for r in rows:
        line = "%4d x%-4d %-8s %-4s %11d %9.4f [%7.4f,%7.4f] %9.1f %9.3f" % (r["taps"], r["L"], r["output"], "on" if r["nco"] else "off",
                                                                            r["outputs"], r["ms"], r["ms_min"], r["ms_max"], r["gsps_out"],
                                                                            r["roofline"])
        if "chain_ms" in r:
            line += " %10.4f [%7.4f,%7.4f] %8.4f %8.2f %6s" % (r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"], r["pass_ms"],
                                                              r["speedup_vs_chain"], "yes" if r["slowest_beats_chain_fastest"] else "no")
        print(line)
    print(json.dumps({"outputs_requested": args.outputs, "warmup": args.warmup, "reps": args.reps, "nco": FREQ, "rows": rows}))


if __name__ == "__main__":
    main()
