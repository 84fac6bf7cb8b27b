#!/usr/bin/env python3
"""subup_bench.py — settled, in-process timing of the per-bin interpolating FIR stage over frames (if_fir_subup_t, DESIGN.md
§3.21) against a torch chain.

Rows (B bins, T taps, tap rows, interpolation R, input frames per call), each with float32 and int16 input, NCO words on:
(1024, 64, 1, 2, 2^15); (4096, 16, 1, 1, 2^14); (64, 128, 64, 4, 2^18) -- the longest row R = 4 admits: ceil(T / R) <= 32 --;
(16, 1024, 1, 64, 2^16); (200, 96, 200, 3, 2^17).  --scale divides every frame count (for a quick look).  The other side of each row, timed alternately with it call by call in the same
process on the same frames: the frames permuted to channel-major, torch.nn.functional.conv_transpose1d(groups = 2 B, stride = R)
trimmed to F R outputs, permuted back, times a precomputed phasor table.  Both start from a zero history at position 0 and a
spread of the outputs is compared.
Per row: ms per call (median, fastest and slowest of --reps timed calls after --warmup, HIP events on a side stream), output
frames per second, and the algorithmic bytes -- frames in plus frames out -- as a fraction of the 8 TB/s roofline.
--words0 sets every word to 0 (the stage skips its rotation, the chain its table).
Every timed call of the stage is one stream continued.  Ends with one JSON line; --out also writes the text to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF = 8e12
# (B, T, rows, R, log2 frames)
SHAPES = ((1024, 64, 1, 2, 15), (4096, 16, 1, 1, 14), (64, 128, 64, 4, 18), (16, 1024, 1, 64, 16), (200, 96, 200, 3, 17))
CASES = tuple(s + (i16,) for s in SHAPES for i16 in (False, True))


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
    ap.add_argument("--words0", action="store_true", help="every NCO word 0: the stage skips the rotation, the chain its table")
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
    for B, T, trows, R, logf, i16 in CASES:
        J = -(-T // R)
        F = max((1 << logf) // args.scale, 4 * J)
        count = F * R
        rng = np.random.default_rng([B, T, R])
        # the usual interpolation filter: a windowed sinc with its cut-off at the input band's edge, a little different per row
        t = np.arange(T) - (T - 1) / 2.0
        h = np.stack([np.sinc(t / R * (1.0 - 0.1 * r / trows)) * np.hamming(T) for r in range(trows)]).astype(np.float32)
        freqs = np.zeros(B) if args.words0 else rng.uniform(-0.5, 0.5, B)
        gen = torch.Generator(device="cuda").manual_seed(B + T)
        x16 = torch.randint(-14000, 14001, (F, B, 2), dtype=torch.int16, device="cuda", generator=gen)
        x32 = x16.to(torch.float32) * (2.0 ** -15) if i16 else torch.randn((F, B, 2), dtype=torch.float32, device="cuda", generator=gen)
        if not i16:
            del x16
        src = x16 if i16 else x32
        out = torch.empty(2 * count * B + 16, dtype=torch.float32, device="cuda")
        keep = {}
        row = {"B": B, "taps": T, "rows": trows, "R": R, "frames": F, "input": "int16" if i16 else "float32"}
        with fir.IfFirSubUp(h, B, R, max_frames=F) as f:
            f.set_stream(stream)
            if i16:
                f.set_input_format(fir.INPUT_I16)
            f.set_nco(freqs)
            # exp(+j 2 pi ((P_j n) mod 2^32) / 2^32) for the quantised words, n = 0 .. F R - 1: the phase in integers
            words = torch.from_numpy(np.round(f.get_nco() * 4294967296.0).astype(np.int64) % (1 << 32)).cuda()
            ph = (torch.arange(count, dtype=torch.int64, device="cuda")[:, None] * words[None, :]) % (1 << 32)
            ang = ph.to(torch.float64) * (2.0 * np.pi / 4294967296.0)
            phasor = torch.complex(torch.cos(ang).to(torch.float32), torch.sin(ang).to(torch.float32))
            del ph, ang
            if args.words0:
                phasor = None
            w = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(h, (B, T)))).cuda()
            weight = w.repeat_interleave(2, dim=0).view(2 * B, 1, T).contiguous()    # channel 2 j + c: bin j, component c

            def chain():
                c = x32.permute(1, 2, 0).reshape(1, 2 * B, F)
                y = torch.nn.functional.conv_transpose1d(c, weight, stride=R, groups=2 * B)[:, :, :count]
                v = torch.view_as_complex(y.reshape(B, 2, count).permute(2, 0, 1).contiguous())
                keep["chain"] = v * phasor if phasor is not None else v

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
        row["mframes_per_s"] = count / row["ms"] / 1e3
        row["bytes"] = F * B * (4 if i16 else 8) + count * B * 8
        row["roofline"] = row["bytes"] / (row["ms"] * 1e-3) / ROOF
        row["chain_over_stage"] = row["chain_ms"] / row["ms"]
        rows.append(row)
        keep.clear()
        del out, x32, src, phasor, weight, w
        torch.cuda.empty_cache()
    lines = ["%-5s %-5s %-5s %-3s %-8s %9s %9s %19s %11s %9s %10s %21s %12s %10s" % (
        "B", "T", "rows", "R", "input", "frames", "ms", "[min, max]", "Mframes/s", "of 8TB/s", "chain ms", "[min, max]", "chain/stage", "max diff")]
    for r in rows:
        lines.append("%-5d %-5d %-5d %-3d %-8s %9d %9.4f [%8.4f,%8.4f] %11.3f %9.3f %10.3f [%9.3f,%9.3f] %12.2f %10.2g"
                     % (r["B"], r["taps"], r["rows"], r["R"], r["input"], r["frames"], r["ms"], r["ms_min"], r["ms_max"],
                        r["mframes_per_s"], r["roofline"], r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"], r["chain_over_stage"],
                        r["chain_max_diff"]))
    lines.append("chain: permute to channel-major -> conv_transpose1d(groups = 2 B, stride = R) trimmed to F R -> permute back -> x phasor "
                 "table, float32, from a zero history; frames: input frames per call, Mframes/s: output frames; max diff: a spread of 4096 "
                 "outputs against the stage's, of the largest value; of 8TB/s: frames in plus frames out")
    lines.append("NCO words: %s" % ("all 0 (no rotation on either side)" if args.words0 else "on"))
    lines.append(json.dumps({"scale": args.scale, "words0": args.words0, "warmup": args.warmup, "reps": args.reps, "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
