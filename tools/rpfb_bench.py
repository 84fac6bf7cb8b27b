#!/usr/bin/env python3
"""rpfb_bench.py — settled, in-process timing of the real-input polyphase filter bank (if_fir_rpfb_t) against the
route it replaces and against a torch chain.

Rows (M channels, K = T / M rows of taps, hop D), 2^26 REAL input samples (--samples), the M/2 + 1 bins out, each with float32
and int16 input: (1024, 8, 1024), (1024, 8, 512), (128, 16, 128), (8192, 4, 8192), (256, 8, 192).  The other sides of each row,
timed alternately with it call by call in the same process on the same data:
* route: what a real stream had to go through before -- a widening pass in torch (r -> (r, 0), same sample format) and
  if_fir_pfb_t with the span 0 .. M/2.  M = 8192 is no size of if_fir_pfb_t: that row has no such route (n/a).
* chain: r.unfold(0, K M, D) times the reversed taps, summed over the K rows, rolled by the frame's (a + 1) mod M,
  torch.fft.rfft.  It starts at the first full window (it has no history) at an offset that puts its frames on the bank's grid.
A spread of the bank's frames is compared with both.  Per row: ms per call (median, fastest and slowest of --reps timed calls
after --warmup, HIP events on a side stream), input MS/s, and the algorithmic bytes -- 4 (or 2) in and 8 ulBins / D out per input
sample -- as a fraction of the 8 TB/s roofline.  Every timed call of a bank is one stream continued.  Ends with one JSON line;
--out also writes the text to a file."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF = 8e12
SHAPES = ((1024, 8, 1024), (1024, 8, 512), (128, 16, 128), (8192, 4, 8192), (256, 8, 192))
PFB_MAX_M = 4096


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
    iq = torch.empty(2 * ((n + 1) // 2), dtype=torch.float32, device="cuda")
    with fir.IfFir(fir.bpf_design(255), decimation=1, max_samples=1024) as f:
        f.set_stream(stream)
        f.synth_device(iq.data_ptr(), 0, iq.numel() // 2, 0)
        f.synchronize()
    r32 = iq[:n].contiguous()   # the I, Q values of the synthetic stream read as n real samples
    del iq
    r16 = (r32 * 14000.0).round().to(torch.int16)
    r16f = r16.to(torch.float32) * (2.0 ** -15)   # what the chain of an int16 row reads: the conversion is not timed
    rows = []
    for M, K, D in SHAPES:
        for i16 in (False, True):
            T, bins = K * M, M // 2 + 1
            # the usual prototype: a windowed sinc with its cut-off at half a channel, unity gain per channel
            t = np.arange(T) - (T - 1) / 2.0
            h = (np.sinc(t / M) * np.hamming(T) / M).astype(np.float32)
            src = r16 if i16 else r32
            frames = -(-n // D)
            out = torch.empty(2 * frames * bins + 16, dtype=torch.float32, device="cuda")
            has_route = M <= PFB_MAX_M
            out_route = torch.empty(2 * frames * bins + 16, dtype=torch.float32, device="cuda") if has_route else None
            wide = torch.zeros(2 * n, dtype=src.dtype, device="cuda") if has_route else None
            xr = r16f if i16 else r32
            off = (1 - T) % D
            win = xr[off:].unfold(0, T, D)
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
                keep["chain"] = torch.fft.rfft(u, dim=1)

            row = {"M": M, "K": K, "D": D, "taps": T, "input": "int16" if i16 else "float32", "samples": n, "bins": bins, "chain_frames": F}
            p = fir.IfFirPfb(h, M, D, first_bin=0, bins=bins, max_samples=n) if has_route else None
            with fir.IfFirRpfb(h, M, D, max_samples=n) as f:
                f.set_stream(stream)
                if i16:
                    f.set_input_format(fir.INPUT_I16)
                if p:
                    p.set_stream(stream)
                    if i16:
                        p.set_input_format(fir.INPUT_I16)

                def rpfb():
                    keep["frames"] = f.process_device(src.data_ptr(), out.data_ptr(), n)

                def route():
                    wide[0::2] = src      # the widening pass: (r, 0), the imaginary halves stay zero
                    keep["route_frames"] = p.process_device(wide.data_ptr(), out_route.data_ptr(), n)

                # a fresh stream for the comparison: chain frame j is the bank's frame (off + j D + T - 1) / D
                rpfb()
                chain()
                if p:
                    route()
                torch.cuda.synchronize()
                y = torch.view_as_complex(out[:2 * keep["frames"] * bins].view(-1, 2)).view(keep["frames"], bins)
                js = torch.unique(torch.linspace(0, F - 1, 64).long()).cuda()
                ms_of = (off + js * D + T - 1) // D
                row["frames"] = keep["frames"]
                row["chain_max_diff"] = (y[ms_of] - keep["chain"][js]).abs().max().item() / keep["chain"][js].abs().max().item()
                if p:
                    assert keep["route_frames"] == keep["frames"]
                    yr = torch.view_as_complex(out_route[:2 * keep["frames"] * bins].view(-1, 2)).view(keep["frames"], bins)
                    row["route_max_diff"] = (y[ms_of] - yr[ms_of]).abs().max().item() / yr[ms_of].abs().max().item()
                    del yr
                runs = [rpfb, route, chain] if p else [rpfb, chain]
                for _ in range(args.warmup):
                    for fn in runs:
                        fn()
                torch.cuda.synchronize()
                ms = {fn.__name__: [] for fn in runs}
                for _ in range(args.reps):
                    for fn in runs:
                        ms[fn.__name__].append(event_ms(torch, fn))
            if p:
                p.close()
            row["ms"], row["ms_min"], row["ms_max"] = stats(ms["rpfb"])
            row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = stats(ms["chain"])
            if p:
                row["route_ms"], row["route_ms_min"], row["route_ms_max"] = stats(ms["route"])
                row["route_over_rpfb"] = row["route_ms"] / row["ms"]
            row["msps_in"] = n / row["ms"] / 1e3
            row["bytes_per_sample"] = (2.0 if i16 else 4.0) + 8.0 * bins / D
            row["roofline"] = row["bytes_per_sample"] * n / (row["ms"] * 1e-3) / ROOF
            row["chain_over_rpfb"] = row["chain_ms"] / row["ms"]
            rows.append(row)
            keep.clear()
            del out, out_route, wide, win, hrev, y
            torch.cuda.empty_cache()
    lines = ["%-5s %-3s %-5s %-8s %9s %19s %9s %9s %10s %21s %11s %10s %10s %21s %11s %10s"
             % ("M", "K", "D", "input", "ms", "[min, max]", "MS/s in", "of 8TB/s", "route ms", "[min, max]", "route/bank", "max diff", "chain ms",
                "[min, max]", "chain/bank", "max diff")]
    for r in rows:
        route = ("%10.4f [%9.4f,%9.4f] %11.2f %10.2g" % (r["route_ms"], r["route_ms_min"], r["route_ms_max"], r["route_over_rpfb"], r["route_max_diff"])
                 if "route_ms" in r else "%10s %21s %11s %10s" % ("n/a", "", "", ""))
        lines.append("%-5d %-3d %-5d %-8s %9.4f [%8.4f,%8.4f] %9.1f %9.3f %s %10.3f [%9.3f,%9.3f] %11.2f %10.2g"
                     % (r["M"], r["K"], r["D"], r["input"], r["ms"], r["ms_min"], r["ms_max"], r["msps_in"], r["roofline"], route,
                        r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"], r["chain_over_rpfb"], r["chain_max_diff"]))
    lines.append("%d real samples a call; bank = if_fir_rpfb_t, all M/2 + 1 bins; route: a widening pass in torch (r -> (r, 0)) + if_fir_pfb_t with the "
                 "span 0 .. M/2 (n/a at M = 8192: no size of if_fir_pfb_t)" % n)
    lines.append("chain: unfold(0, K M, D) x reversed taps -> sum over the K rows -> roll by (a + 1) mod M -> torch.fft.rfft, from the first full "
                 "window; max diff: a spread of 64 frames of the bank against the other side's, of the largest value")
    lines.append(json.dumps({"samples": n, "warmup": args.warmup, "reps": args.reps, "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
