#!/usr/bin/env python3
"""rsynth_bench.py — settled, in-process timing of the real-output polyphase synthesis bank (if_fir_rsynth_t)
against the route it replaces and against a torch chain.

Rows (M channels, T taps, hop L), 2^26 REAL output samples (--samples), all M/2 + 1 bins in: (1024, 8 M, 1024), (1024, 8 M, 512),
(128, 16 M, 128), (8192, 4 M, 8192), (256, 8 M, 192), each with float32 and int16 input and float32 and int16 output.  The other
sides of each row, timed alternately with it call by call in the same process on the same frames:
  route: the Hermitian extension of every frame in torch (M - 2 bins written), IfFirSynth on all M channels, a real-part pass
         (and, for int16 output, SPEC §11's conversion in torch); no such route at M = 8192 (no size of if_fir_synth_t);
  chain: torch.fft.irfft x M, each frame rolled to its output position and tiled to J L values, times the tap rows, overlap-added
         with J slice additions (and the conversion for int16 output).
All start from a zero history and a spread of the outputs is compared (float32 output: of the largest value; int16: in LSB).
Per row: ms per call (median, fastest and slowest of --reps timed calls after --warmup, HIP events on a side stream), output
MS/s, and the algorithmic bytes -- 8 (or 4) (M/2 + 1) / L in and 4 (or 2) out per output sample -- as a fraction of the 8 TB/s
roofline.  Every timed call of the bank is one stream continued.  Ends with one JSON line; --out also writes the text to a file."""
import argparse
import contextlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF = 8e12
# (M, T / M, L)
ROWS = ((1024, 8, 1024), (1024, 8, 512), (128, 16, 128), (8192, 4, 8192), (256, 8, 192))


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
    ap.add_argument("--rows", default=None, help="comma-separated indices into the rows above (default: all)")
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
    for M, K, L in ([ROWS[int(i)] for i in args.rows.split(",")] if args.rows else ROWS):
        T, H = K * M, M // 2
        bins = H + 1
        J = -(-T // L)
        F = args.samples // L
        n = F * L
        # the usual prototype: a windowed sinc with its cut-off at half a channel, scaled so that the output stays inside +-1
        t = np.arange(T) - (T - 1) / 2.0
        h = (np.sinc(t / M) * np.hamming(T) * (0.2 / math.sqrt(M))).astype(np.float32)
        hp = np.zeros(J * L, dtype=np.float32)
        hp[:T] = h
        rows_t = torch.from_numpy(hp).cuda().view(J, L)
        period = M // math.gcd(L, M)
        reps_t = -(-J * L // M)
        has_route = M <= 4096
        for i16 in (False, True):
            gen = torch.Generator(device="cuda").manual_seed(M + L)
            x16 = torch.randint(-14000, 14001, (F, bins, 2), dtype=torch.int16, device="cuda", generator=gen)
            x32 = x16.to(torch.float32) * (2.0 ** -15) if i16 else torch.randn((F, bins, 2), dtype=torch.float32, device="cuda", generator=gen)
            if not i16:
                del x16
            src = x16 if i16 else x32
            X = torch.view_as_complex(x32)
            ext = torch.empty((F, M, 2), dtype=src.dtype, device="cuda") if has_route else None
            mid = torch.empty(2 * n + 16, dtype=torch.float32, device="cuda") if has_route else None
            for o16 in (False, True):
                out = torch.empty(n + 16, dtype=torch.int16 if o16 else torch.float32, device="cuda")
                keep = {}

                def convert(y):
                    return torch.clamp(torch.round(y * 32768.0), -32768.0, 32767.0).to(torch.int16) if o16 else y

                def chain():
                    v = torch.fft.irfft(X, n=M, dim=1) * M
                    r = torch.empty_like(v)
                    for s in range(period):
                        r[s::period] = torch.roll(v[s::period], -((s * L) % M), dims=1)
                    w = r.repeat(1, reps_t)[:, :J * L].view(F, J, L) * rows_t
                    y = torch.zeros((F + J - 1, L), dtype=torch.float32, device="cuda")
                    for j in range(J):
                        y[j:j + F] += w[:, j, :]
                    keep["chain"] = convert(y.view(-1)[:n])

                row = {"M": M, "taps": T, "L": L, "J": J, "input": "int16" if i16 else "float32", "output": "int16" if o16 else "float32",
                       "outputs": n, "frames": F, "bins": bins}
                with fir.IfFirRsynth(h, M, L, max_frames=F) as f, contextlib.ExitStack() as stack:
                    old = stack.enter_context(fir.IfFirSynth(h, M, L, max_frames=F)) if has_route else None
                    for c in (f, old) if has_route else (f,):
                        c.set_stream(stream)
                        if i16:
                            c.set_input_format(fir.INPUT_I16)
                    if o16:
                        f.set_output_format(fir.OUTPUT_I16)

                    def bank():
                        keep["outputs"] = f.process_device(src.data_ptr(), out.data_ptr(), F)

                    def route():
                        ext[:, :bins] = src
                        ext[:, 0, 1] = 0
                        ext[:, H, 1] = 0
                        ext[:, bins:, 0] = torch.flip(src[:, 1:H, 0], dims=[1])
                        ext[:, bins:, 1] = -torch.flip(src[:, 1:H, 1], dims=[1])
                        old.process_device(ext.data_ptr(), mid.data_ptr(), F)
                        keep["route"] = convert(mid[:2 * n].view(-1, 2)[:, 0].contiguous())

                    runs = [bank, chain] + ([route] if has_route else [])
                    for fn in runs:
                        fn()
                    torch.cuda.synchronize()
                    at = torch.unique(torch.arange(4096, dtype=torch.int64) * (n - 1) // 4095).cuda()   # (in integers: 0 .. n - 1 exactly)
                    assert int(at.min()) >= 0 and int(at.max()) < n and keep["outputs"] == n
                    y = out[:n][at].to(torch.float32)
                    for name in ("chain", "route")[:len(runs) - 1]:
                        want = keep[name][at].to(torch.float32)
                        row[name + "_max_diff"] = (y - want).abs().max().item() / (1.0 if o16 else want.abs().max().item())
                    row["peak"] = out[:n].to(torch.float32).abs().max().item() / (32768.0 if o16 else 1.0)
                    for _ in range(args.warmup):
                        for fn in runs:
                            fn()
                    torch.cuda.synchronize()
                    ms = {fn.__name__: [] for fn in runs}
                    for _ in range(args.reps):
                        for fn in runs:
                            ms[fn.__name__].append(event_ms(torch, fn))
                    f.synchronize()
                    if has_route:
                        old.synchronize()
                row["ms"], row["ms_min"], row["ms_max"] = stats(ms["bank"])
                row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = stats(ms["chain"])
                row["chain_over_bank"] = row["chain_ms"] / row["ms"]
                if has_route:
                    row["route_ms"], row["route_ms_min"], row["route_ms_max"] = stats(ms["route"])
                    row["route_over_bank"] = row["route_ms"] / row["ms"]
                row["msps_out"] = n / row["ms"] / 1e3
                row["bytes_per_output"] = (4.0 if i16 else 8.0) * bins / L + (2.0 if o16 else 4.0)
                row["roofline"] = row["bytes_per_output"] * n / (row["ms"] * 1e-3) / ROOF
                rows.append(row)
                keep.clear()
                del out
                torch.cuda.empty_cache()
            del X, x32, src, ext, mid
            torch.cuda.empty_cache()
    lines = ["%-5s %-6s %-5s %-8s %-8s %9s %19s %9s %9s %9s %19s %11s %9s %10s %21s %11s %9s"
             % ("M", "T", "L", "input", "output", "ms", "[min, max]", "MS/s out", "of 8TB/s", "route ms", "[min, max]", "route/bank", "max diff",
                "chain ms", "[min, max]", "chain/bank", "max diff")]
    for r in rows:
        head = "%-5d %-6d %-5d %-8s %-8s %9.4f [%8.4f,%8.4f] %9.1f %9.3f " % (r["M"], r["taps"], r["L"], r["input"], r["output"], r["ms"],
                                                                         r["ms_min"], r["ms_max"], r["msps_out"], r["roofline"])
        if "route_ms" in r:
            mid_ = "%9.4f [%8.4f,%8.4f] %11.2f %9.2g " % (r["route_ms"], r["route_ms_min"], r["route_ms_max"], r["route_over_bank"], r["route_max_diff"])
        else:
            mid_ = "%9s %19s %11s %9s " % ("n/a", "", "", "")
        lines.append(head + mid_ + "%10.3f [%9.3f,%9.3f] %11.2f %9.2g" % (r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"], r["chain_over_bank"],
                                                                        r["chain_max_diff"]))
    lines.append("%d real outputs a call; bank = if_fir_rsynth_t, all M/2 + 1 bins; route: the Hermitian extension of every frame in torch + "
                 "if_fir_synth_t on all M channels + a real-part pass (+ the int16 conversion in torch); n/a at M = 8192: no size of if_fir_synth_t"
                 % args.samples)
    lines.append("chain: torch.fft.irfft x M -> roll to the frame's output position, tile to J L -> x tap rows -> J overlapping slice additions "
                 "(+ the int16 conversion), from a zero history; max diff: a spread of 4096 outputs of the bank against the other side's, of the "
                 "largest value (float32 output) or in LSB (int16 output)")
    lines.append(json.dumps({"outputs": args.samples, "warmup": args.warmup, "reps": args.reps, "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
