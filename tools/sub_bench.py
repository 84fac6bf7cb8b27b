#!/usr/bin/env python3
"""sub_bench.py — settled, in-process timing of the per-channel FIR stage over filter-bank frames (if_fir_sub_t)
against a torch chain.

Rows (B bins, T taps, tap rows, decimation R, frames per call): (1024, 32, 1, 2, 2^16) with float32 and int16 input, NCO words
on and all 0; (4096, 16, 1, 1, 2^14); (64, 64, 64, 4, 2^20); (16, 128, 1, 8, 2^22); (200, 48, 200, 3, 2^18), words on.  --scale
divides every frame count (for a quick look).  The other side of each row, timed alternately with it call by call in the same
process on the same frames: the frames times a precomputed phasor table (skipped where the words are 0), permuted to
channel-major, torch.nn.functional.conv1d(groups = 2 B, stride = R) over the left-padded streams, permuted back.  Both start
from a zero history at position 0 and a spread of the outputs is compared.
Per row: ms per call (median, fastest and slowest of --reps timed calls after --warmup, HIP events on a side stream), input
frames per second, and the algorithmic bytes -- frames in plus frames out -- as a fraction of the 8 TB/s roofline.
Every timed call of the stage is one stream continued.  Ends with one JSON line; --out also writes the text to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF = 8e12
# (B, T, rows, R, log2 frames, int16 input, words on)
CASES = ((1024, 32, 1, 2, 16, False, True), (1024, 32, 1, 2, 16, True, True), (1024, 32, 1, 2, 16, False, False),
         (1024, 32, 1, 2, 16, True, False), (4096, 16, 1, 1, 14, False, True), (64, 64, 64, 4, 20, False, True),
         (16, 128, 1, 8, 22, False, True), (200, 48, 200, 3, 18, False, True))


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
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()  # the contexts run on the stream the events are recorded on (not the null stream: handle 0
    torch.cuda.set_stream(side)  # would select a context's own stream)
    stream = side.cuda_stream
    rows = []
    for B, T, trows, R, logf, i16, words_on in CASES:
        F = max((1 << logf) // args.scale, 4 * T)
        count = -(-F // R)
        rng = np.random.default_rng([B, T, R])
        # the usual channel filter: a windowed sinc with its cut-off at the decimated band's edge, a little different per row
        t = np.arange(T) - (T - 1) / 2.0
        h = np.stack([np.sinc(t / R * (1.0 - 0.1 * r / trows)) / R * np.hamming(T) for r in range(trows)]).astype(np.float32)
        freqs = rng.uniform(-0.5, 0.5, B) if words_on else None
        gen = torch.Generator(device="cuda").manual_seed(B + T)
        x16 = torch.randint(-14000, 14001, (F, B, 2), dtype=torch.int16, device="cuda", generator=gen)
        x32 = x16.to(torch.float32) * (2.0 ** -15) if i16 else torch.randn((F, B, 2), dtype=torch.float32, device="cuda", generator=gen)
        if not i16:
            del x16
        src = x16 if i16 else x32
        X = torch.view_as_complex(x32)
        out = torch.empty(2 * count * B + 16, dtype=torch.float32, device="cuda")
        keep = {}
        row = {"B": B, "taps": T, "rows": trows, "R": R, "frames": F, "input": "int16" if i16 else "float32", "words": "on" if words_on else "0"}
        with fir.IfFirSub(h, B, R, max_frames=F) as f:
            f.set_stream(stream)
            if i16:
                f.set_input_format(fir.INPUT_I16)
            f.set_nco(freqs)
            phasor = None
            if words_on:
                # exp(-j 2 pi ((P_j a) mod 2^32) / 2^32) for the quantised words, a = 0 .. F - 1: the phase in integers
                words = torch.from_numpy(np.round(f.get_nco() * 4294967296.0).astype(np.int64) % (1 << 32)).cuda()
                ph = (torch.arange(F, dtype=torch.int64, device="cuda")[:, None] * words[None, :]) % (1 << 32)
                ang = ph.to(torch.float64) * (-2.0 * np.pi / 4294967296.0)
                phasor = torch.complex(torch.cos(ang).to(torch.float32), torch.sin(ang).to(torch.float32))
                del ph, ang
            w = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(h[:, ::-1], (B, T)))).cuda()
            weight = w.repeat_interleave(2, dim=0).view(2 * B, 1, T).contiguous()    # channel 2 j + c: bin j, component c

            def chain():
                v = X * phasor if phasor is not None else X
                c = torch.view_as_real(v).permute(1, 2, 0).reshape(1, 2 * B, F)
                y = torch.nn.functional.conv1d(torch.nn.functional.pad(c, (T - 1, 0)), weight, stride=R, groups=2 * B)
                keep["chain"] = torch.view_as_complex(y.view(B, 2, -1).permute(2, 0, 1).contiguous())

            def stage():
                keep["frames"] = f.process_device(src.data_ptr(), out.data_ptr(), F)

            stage()
            chain()
            torch.cuda.synchronize()
            assert keep["frames"] == count == keep["chain"].shape[0]
            y = torch.view_as_complex(out[:2 * count * B].view(-1, 2))
            want = keep["chain"].reshape(-1)
            n = count * B
            at = torch.unique(torch.arange(4096, dtype=torch.int64) * (n - 1) // 4095).cuda()   # (in integers: 0 .. n - 1 exactly)
            row["chain_max_diff"] = (y[at] - want[at]).abs().max().item() / want[at].abs().max().item()
            del y, want
            runs = [stage, chain]
            for _ in range(args.warmup):
                for fn in runs:
                    fn()
            torch.cuda.synchronize()
            ms = {fn.__name__: [] for fn in runs}
            for _ in range(args.reps):
                for fn in runs:
                    ms[fn.__name__].append(event_ms(torch, fn))
            f.synchronize()
        row["ms"], row["ms_min"], row["ms_max"] = stats(ms["stage"])
        row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = stats(ms["chain"])
        row["mframes_per_s"] = F / row["ms"] / 1e3
        row["bytes"] = F * B * (4 if i16 else 8) + count * B * 8
        row["roofline"] = row["bytes"] / (row["ms"] * 1e-3) / ROOF
        row["chain_over_stage"] = row["chain_ms"] / row["ms"]
        rows.append(row)
        keep.clear()
        del out, X, x32, src, phasor, weight, w
        torch.cuda.empty_cache()
    lines = ["%-5s %-4s %-5s %-3s %-8s %-5s %9s %9s %19s %11s %9s %10s %21s %12s %10s" % (
        "B", "T", "rows", "R", "input", "words", "frames", "ms", "[min, max]", "Mframes/s", "of 8TB/s", "chain ms", "[min, max]", "chain/stage",
        "max diff")]
    for r in rows:
        lines.append("%-5d %-4d %-5d %-3d %-8s %-5s %9d %9.4f [%8.4f,%8.4f] %11.3f %9.3f %10.3f [%9.3f,%9.3f] %12.2f %10.2g"
                     % (r["B"], r["taps"], r["rows"], r["R"], r["input"], r["words"], r["frames"], r["ms"], r["ms_min"], r["ms_max"],
                        r["mframes_per_s"], r["roofline"], r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"], r["chain_over_stage"],
                        r["chain_max_diff"]))
    lines.append("chain: frames x phasor table (words on) -> permute to channel-major -> conv1d(groups = 2 B, stride = R) over the left-padded "
                 "streams -> permute back, float32, from a zero history; max diff: a spread of 4096 outputs against the stage's, of the largest "
                 "value; of 8TB/s: frames in plus frames out")
    lines.append(json.dumps({"scale": args.scale, "warmup": args.warmup, "reps": args.reps, "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
