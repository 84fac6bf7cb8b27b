#!/usr/bin/env python3
"""pfb_bench.py — settled, in-process timing of the polyphase filter bank (if_fir_pfb_t) against a torch chain.

Rows (M channels, K = T / M rows of taps, hop D), 2^26 input samples (--samples), all M bins out: (1024, 8, 1024) and
(1024, 8, 512) with float32 and int16 input, (64, 16, 64), (4096, 4, 4096), (256, 8, 192).  The other side of each row, timed
alternately with it call by call in the same process on the same data: x.unfold(0, K M, D) times the reversed taps, summed
over the K rows, rolled by the frame's (a + 1) mod M, torch.fft.fft.  The chain starts at the first full window (it has no
history) at an offset that puts its frames on the bank's grid, and a spread of its frames is compared with the bank's.
Per row: ms per call (median, fastest and slowest of --reps timed calls after --warmup, HIP events on a side stream), input
MS/s, and the algorithmic bytes -- 8 (or 4) in and 8 ulBins / D out per input sample -- as a fraction of the 8 TB/s roofline.
Every timed call of the bank is one stream continued.  Ends with one JSON line; --out also writes the text to a file."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF = 8e12
# (M, K, D, int16 input)
CASES = ((1024, 8, 1024, False), (1024, 8, 1024, True), (1024, 8, 512, False), (1024, 8, 512, True), (64, 16, 64, False),
         (4096, 4, 4096, False), (256, 8, 192, False))


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
    n = args.samples
    x32 = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    with fir.IfFir(fir.bpf_design(255), decimation=1, max_samples=1024) as f:
        f.set_stream(stream)
        f.synth_device(x32.data_ptr(), 0, n, 0)
        f.synchronize()
    x16 = (x32 * 14000.0).round().to(torch.int16)
    x16f = x16.to(torch.float32) * (2.0 ** -15)   # what the chain of an int16 row reads: the conversion is not timed
    rows = []
    for M, K, D, i16 in CASES:
        T = K * M
        # the usual prototype: a windowed sinc with its cut-off at half a channel, unity gain per channel
        t = np.arange(T) - (T - 1) / 2.0
        h = (np.sinc(t / M) * np.hamming(T) / M).astype(np.float32)
        src = x16 if i16 else x32
        frames = -(-n // D)
        out = torch.empty(2 * frames * M + 16, dtype=torch.float32, device="cuda")
        xc = torch.view_as_complex((x16f if i16 else x32).view(-1, 2))
        off = (1 - T) % D
        win = xc[off:].unfold(0, T, D)
        F = win.shape[0]
        hrev = torch.from_numpy(h[::-1].copy()).cuda()
        period = M // math.gcd(D, M)
        shifts = [(off + s * D + T) % M for s in range(period)]
        keep = {}

        def chain():
            w = (win * hrev).view(F, K, M).sum(1)
            u = torch.empty_like(w)
            for s in range(period):
                u[s::period] = torch.roll(w[s::period], shifts[s], dims=1)
            keep["chain"] = torch.fft.fft(u, dim=1)

        row = {"M": M, "K": K, "D": D, "taps": T, "input": "int16" if i16 else "float32", "samples": n, "bins": M, "chain_frames": F}
        with fir.IfFirPfb(h, M, D, max_samples=n) as f:
            f.set_stream(stream)
            if i16:
                f.set_input_format(fir.INPUT_I16)

            def pfb():
                keep["frames"] = f.process_device(src.data_ptr(), out.data_ptr(), n)

            # a fresh stream for the comparison: chain frame j is the bank's frame (off + j D + T - 1) / D
            pfb()
            chain()
            torch.cuda.synchronize()
            y = torch.view_as_complex(out[:2 * keep["frames"] * M].view(-1, 2)).view(keep["frames"], M)
            js = torch.unique(torch.linspace(0, F - 1, 64).long()).cuda()
            ms_of = (off + js * D + T - 1) // D
            diff = (y[ms_of] - keep["chain"][js]).abs().max().item() / keep["chain"][js].abs().max().item()
            row["frames"] = keep["frames"]
            row["chain_max_diff"] = diff
            runs = [pfb, chain]
            for _ in range(args.warmup):
                for fn in runs:
                    fn()
            torch.cuda.synchronize()
            ms = {fn.__name__: [] for fn in runs}
            for _ in range(args.reps):
                for fn in runs:
                    ms[fn.__name__].append(event_ms(torch, fn))
        row["ms"], row["ms_min"], row["ms_max"] = stats(ms["pfb"])
        row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = stats(ms["chain"])
        row["msps_in"] = n / row["ms"] / 1e3
        row["bytes_per_sample"] = (4.0 if i16 else 8.0) + 8.0 * M / D
        row["roofline"] = row["bytes_per_sample"] * n / (row["ms"] * 1e-3) / ROOF
        row["chain_over_pfb"] = row["chain_ms"] / row["ms"]
        rows.append(row)
        keep.clear()
        del out, win, xc, hrev, y
        torch.cuda.empty_cache()
    lines = ["%-5s %-3s %-5s %-8s %10s %9s %19s %9s %9s %10s %21s %11s %10s" % ("M", "K", "D", "input", "samples", "ms", "[min, max]", "MS/s in", "of 8TB/s",
                                                                               "chain ms", "[min, max]", "chain/bank", "max diff")]
    for r in rows:
        lines.append("%-5d %-3d %-5d %-8s %10d %9.4f [%8.4f,%8.4f] %9.1f %9.3f %10.3f [%9.3f,%9.3f] %11.2f %10.2g"
                     % (r["M"], r["K"], r["D"], r["input"], r["samples"], r["ms"], r["ms_min"], r["ms_max"], r["msps_in"], r["roofline"],
                        r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"], r["chain_over_pfb"], r["chain_max_diff"]))
    lines.append("chain: unfold(0, K M, D) x reversed taps -> sum over the K rows -> roll by (a + 1) mod M -> torch.fft.fft, complex64, from the "
                 "first full window; max diff: a spread of 64 chain frames against the bank's, of the largest value")
    lines.append(json.dumps({"samples": n, "warmup": args.warmup, "reps": args.reps, "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
