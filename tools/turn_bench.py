#!/usr/bin/env python3
"""turn_bench.py — settled, in-process timing of the corner turn (if_fir_turn_t) against the route a Python user
has today, a torch chain.  (A caller of the C ABI has no such chain: a strided copy per channel or a trip through the host.)

Rows (B elements per frame, C channels, selection, frames per call): (1024, 1024, span, 2^16), (1024, 16, scattered, 2^18),
(4097, 64, span, 2^16), (8192, 918, span, 2^13), (64, 64, span, 2^20); both directions; float32 and int16 in with float32 out,
and float32 in with int16 out.  --scale divides every frame count (for a quick look).  The row pitch is the frame count.
The other side of each row, timed alternately with it call by call in the same process on the same data:
  TO_STREAMS  frames[:, sel].t().contiguous()                            (int16 in: .to(float32) * 2^-15 first on the gathered part;
  TO_FRAMES   z = zeros(F, B); z[:, sel] = rows[:, :F].t()                int16 out: * 2^15, round, clamp, .to(int16) last)
The two results are compared bit for bit before the timing (int16 out on finite data).
Per row: ms per call (median, fastest and slowest of --reps timed calls after --warmup, HIP events on a side stream), the
chain's, the ratio, and two shares of the 8 TB/s roofline: on ALGORITHMIC bytes -- the listed elements in plus every byte
written -- and, for TO_STREAMS, on bytes at the FETCH GRANULARITY -- every 128-byte line of the frames that holds a listed
element, counted from the addresses, plus the bytes written (128 bytes: the L2 line of CDNA 3 / CDNA 4; for a span the two
agree to within the lines at its ends).  The chip's streaming-copy rate, about 0.79 of the roofline, is the practical ceiling.
Ends with one JSON line; --out also writes the text to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF = 8e12
LINE = 128
# (B, C, selection, log2 frames)
SHAPES = ((1024, 1024, "span", 16), (1024, 16, "scattered", 18), (4097, 64, "span", 16), (8192, 918, "span", 13), (64, 64, "span", 20))
# (int16 in, int16 out)
FORMATS = ((False, False), (True, False), (False, True))


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


def timed(torch, runs, warmup, reps):
    """the runs alternately, call by call: {name: (median, min, max) ms}"""
    for _ in range(warmup):
        for fn in runs:
            fn()
    torch.cuda.synchronize()
    ms = {fn.__name__: [] for fn in runs}
    for _ in range(reps):
        for fn in runs:
            ms[fn.__name__].append(event_ms(torch, fn))
    torch.cuda.synchronize()
    return {k: stats(v) for k, v in ms.items()}


def lines_per_frame(np, sel, B, e):
    """128-byte lines holding a listed element, averaged over the frames of one alignment period (the buffer starts on a line)"""
    period = LINE // np.gcd(LINE, (B * e) % LINE or LINE)
    total = 0
    for a in range(period):
        total += np.unique((a * B + np.asarray(sel, dtype=np.int64)) * e // LINE).size
    return total / period


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    import turn_ref
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()  # the contexts run on the stream the events are recorded on (not the null stream: handle 0
    torch.cuda.set_stream(side)  # would select a context's own stream)
    stream = side.cuda_stream
    rows = []
    for direction in (fir.TURN_TO_STREAMS, fir.TURN_TO_FRAMES):
        for B, C, kind, logf in SHAPES:
            for i16, o16 in FORMATS:
                F = max((1 << logf) // args.scale, 64)
                sel = turn_ref.selection(kind, B, C) if kind != "span" else list(range(C))
                dsel = torch.tensor(sel, dtype=torch.int64, device="cuda")
                gen = torch.Generator(device="cuda").manual_seed(B + C)
                shape = (F, B, 2) if direction == fir.TURN_TO_STREAMS else (C, F, 2)
                if i16:
                    src = torch.randint(-32768, 32768, shape, dtype=torch.int16, device="cuda", generator=gen)
                else:
                    src = torch.randn(shape, dtype=torch.float32, device="cuda", generator=gen) * 0.3
                odt = torch.int16 if o16 else torch.float32
                dst = torch.zeros((C, F, 2) if direction == fir.TURN_TO_STREAMS else (F, B, 2), dtype=odt, device="cuda")
                keep = {}
                row = {"direction": "to_streams" if direction == fir.TURN_TO_STREAMS else "to_frames", "B": B, "C": C, "selection": kind,
                       "frames": F, "input": "int16" if i16 else "float32", "output": "int16" if o16 else "float32"}

                def convert(v):
                    if i16 and not o16:
                        return v.to(torch.float32) * (2.0 ** -15)
                    if o16 and not i16:
                        return torch.clamp(torch.round(v * 32768.0), -32768, 32767).to(torch.int16)
                    return v

                with fir.IfFirTurn(direction, B, sel=None if kind == "span" else sel, channels=C, input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32,
                                   output_format=fir.OUTPUT_I16 if o16 else fir.OUTPUT_F32, max_frames=F) as t:
                    t.set_stream(stream)

                    def chain():
                        if direction == fir.TURN_TO_STREAMS:
                            keep["chain"] = convert(src[:, dsel]).transpose(0, 1).contiguous()
                        else:
                            z = torch.zeros((F, B, 2), dtype=odt, device="cuda")
                            z[:, dsel] = convert(src[:, :F]).transpose(0, 1)
                            keep["chain"] = z

                    def stage():
                        t.process_device(src.data_ptr(), dst.data_ptr(), F, F)

                    stage()
                    chain()
                    torch.cuda.synchronize()
                    word = torch.int32 if o16 else torch.int64
                    row["equal"] = bool(torch.equal(dst.view(word), keep["chain"].view(word)))
                    tm = timed(torch, [stage, chain], args.warmup, args.reps)
                    t.synchronize()
                ein, eout = (4 if i16 else 8), (4 if o16 else 8)
                written = (C * F if direction == fir.TURN_TO_STREAMS else F * B) * eout
                row["ms"], row["ms_min"], row["ms_max"] = tm["stage"]
                row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = tm["chain"]
                row["bytes"] = C * F * ein + written
                row["roofline"] = row["bytes"] / (row["ms"] * 1e-3) / ROOF
                if direction == fir.TURN_TO_STREAMS:
                    row["fetch_bytes"] = int(lines_per_frame(np, sel, B, ein) * LINE * F) + written
                    row["fetch_roofline"] = row["fetch_bytes"] / (row["ms"] * 1e-3) / ROOF
                row["chain_over_stage"] = row["chain_ms"] / row["ms"]
                rows.append(row)
                keep.clear()
                del src, dst
                torch.cuda.empty_cache()
    lines = ["%-10s %-5s %-5s %-9s %-8s %-8s %9s %9s %19s %9s %9s %10s %21s %12s %6s" % (
        "direction", "B", "C", "selection", "input", "output", "frames", "ms", "[min, max]", "of 8TB/s", "at 128 B", "chain ms", "[min, max]",
        "chain/stage", "equal")]
    for r in rows:
        lines.append("%-10s %-5d %-5d %-9s %-8s %-8s %9d %9.4f [%8.4f,%8.4f] %9.3f %9s %10.3f [%9.3f,%9.3f] %12.2f %6s"
                     % (r["direction"], r["B"], r["C"], r["selection"], r["input"], r["output"], r["frames"], r["ms"], r["ms_min"], r["ms_max"],
                        r["roofline"], "%.3f" % r["fetch_roofline"] if "fetch_roofline" in r else "-", r["chain_ms"], r["chain_ms_min"],
                        r["chain_ms_max"], r["chain_over_stage"], "yes" if r["equal"] else "NO"))
    lines.append("chain: to_streams frames[:, sel].t().contiguous(); to_frames z = zeros(F, B); z[:, sel] = rows[:, :F].t(); int16 in: "
                 ".to(float32) * 2^-15; int16 out: * 2^15, round, clamp, .to(int16).  of 8TB/s: listed elements in plus bytes written; at 128 B: "
                 "every 128-byte line of the frames holding a listed element, plus bytes written (the streaming-copy rate of the chip is about 0.79)")
    lines.append(json.dumps({"scale": args.scale, "warmup": args.warmup, "reps": args.reps, "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
