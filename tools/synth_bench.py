#!/usr/bin/env python3
"""synth_bench.py — settled, in-process timing of the polyphase synthesis bank (if_fir_synth_t) against a torch
chain, at several workspace budgets, and at M = 64 against the channel combiner.

Rows (M channels, T taps, hop L), 2^26 output samples (--samples), all M bins in: (1024, 8 M, 1024) and (1024, 8 M, 512) with
float32 and int16 input, (64, 16 M, 64), (4096, 4 M, 4096), (256, 8 M, 192).  The other side of each row, timed alternately
with it call by call in the same process on the same frames: torch.fft.ifft x M, each frame rolled to its output position and
tiled to J L values, times the tap rows, overlap-added with J slice additions.  Both start from a zero history and a spread of
the outputs is compared.  At (64, 16 M, 64) IfFirCombiner with C = 64, L = 64 and centres k / 64 is timed in the same
alternation, on the same values laid out one stream per channel.
Per row: ms per call (median, fastest and slowest of --reps timed calls after --warmup, HIP events on a side stream), output
MS/s, and the algorithmic bytes -- 8 (or 4) M / L in and 8 out per output sample -- as a fraction of the 8 TB/s roofline; then
the workspace route's median at each workspace budget of --budgets (MB; the first is the library's default), and the two routes
against each other where the LDS ring fits.
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
# (M, T / M, L, int16 input)
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
    ap.add_argument("--budgets", default="128,32,4")
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
    budgets = [int(b) for b in args.budgets.split(",")]
    rows = []
    for M, K, L, i16 in CASES:
        T = K * M
        J = -(-T // L)
        F = args.samples // L
        n = F * L
        # the usual prototype: a windowed sinc with its cut-off at half a channel
        t = np.arange(T) - (T - 1) / 2.0
        h = (np.sinc(t / M) * np.hamming(T)).astype(np.float32)
        gen = torch.Generator(device="cuda").manual_seed(M + L)
        x16 = torch.randint(-14000, 14001, (F, M, 2), dtype=torch.int16, device="cuda", generator=gen)
        x32 = x16.to(torch.float32) * (2.0 ** -15) if i16 else torch.randn((F, M, 2), dtype=torch.float32, device="cuda", generator=gen)
        if not i16:
            del x16
        src = x16 if i16 else x32
        X = torch.view_as_complex(x32)
        out = torch.empty(2 * n + 16, dtype=torch.float32, device="cuda")
        hp = np.zeros(J * L, dtype=np.float32)
        hp[:T] = h
        rows_t = torch.from_numpy(hp).cuda().view(J, L)
        period = M // math.gcd(L, M)
        reps_t = -(-J * L // M)
        keep = {}

        def chain():
            v = torch.fft.ifft(X, dim=1) * M
            r = torch.empty_like(v)
            for s in range(period):
                r[s::period] = torch.roll(v[s::period], -((s * L) % M), dims=1)
            w = r.repeat(1, reps_t)[:, :J * L].view(F, J, L) * rows_t
            y = torch.zeros((F + J - 1, L), dtype=torch.complex64, device="cuda")
            for j in range(J):
                y[j:j + F] += w[:, j, :]
            keep["chain"] = y

        row = {"M": M, "taps": T, "L": L, "J": J, "input": "int16" if i16 else "float32", "outputs": n, "frames": F}
        with fir.IfFirSynth(h, M, L, max_frames=F, dev=True) as f:
            f.set_stream(stream)
            if i16:
                f.set_input_format(fir.INPUT_I16)

            def bank():
                keep["outputs"] = f.process_device(src.data_ptr(), out.data_ptr(), F)

            bank()
            chain()
            torch.cuda.synchronize()
            y = torch.view_as_complex(out[:2 * n].view(-1, 2))
            want = keep["chain"].view(-1)[:n]
            at = torch.unique(torch.arange(4096, dtype=torch.int64) * (n - 1) // 4095).cuda()   # (in integers: 0 .. n - 1 exactly)
            assert int(at.min()) >= 0 and int(at.max()) < n
            row["chain_max_diff"] = (y[at] - want[at]).abs().max().item() / want[at].abs().max().item()
            del y, want
            runs = [bank, chain]
            comb = None
            if M == 64 and L == 64:
                xt = [X[:, k].contiguous() for k in range(M)]   # one stream per channel: the combiner's layout
                centres = ((np.arange(M) / M + 0.5) % 1.0) - 0.5
                comb = fir.IfFirCombiner(h, L, centres, max_samples=F)
                comb.set_stream(stream)
                out_c = torch.empty(2 * n + 16, dtype=torch.float32, device="cuda")
                ptrs = [c.data_ptr() for c in xt]

                def combiner():
                    keep["combiner"] = comb.process_device(ptrs, out_c.data_ptr(), F)

                combiner()
                torch.cuda.synchronize()
                a, b = torch.view_as_complex(out_c[:2 * n].view(-1, 2)), torch.view_as_complex(out[:2 * n].view(-1, 2))
                row["combiner_max_diff"] = (a[at] - b[at]).abs().max().item() / b[at].abs().max().item()
                runs.append(combiner)
            for _ in range(args.warmup):
                for fn in runs:
                    fn()
            torch.cuda.synchronize()
            ms = {fn.__name__: [] for fn in runs}
            for _ in range(args.reps):
                for fn in runs:
                    ms[fn.__name__].append(event_ms(torch, fn))
            if comb is not None:
                row["combiner_ms"], row["combiner_ms_min"], row["combiner_ms_max"] = stats(ms["combiner"])
                comb.close()
                del xt, out_c
            keep.pop("chain", None)
            torch.cuda.empty_cache()
            # the workspace budgets, the workspace route alone, alternating
            f.debug_config(route=fir.IfFirSynth.ROUTE_WORKSPACE)
            row["budget_ms"] = {}
            per = {b: [] for b in budgets}
            for _ in range(args.reps):
                for b in budgets:
                    f.debug_workspace(b << 20)
                    bank()
                    per[b].append(event_ms(torch, bank))
            for b in budgets:
                row["budget_ms"][str(b)] = stats(per[b])
            # the two routes, where the LDS ring fits, alternating (the workspace at the library's default budget)
            f.debug_workspace(budgets[0] << 20)
            row["route"] = f.debug_config()
            row["route_ms"] = {}
            try:
                f.debug_config(route=fir.IfFirSynth.ROUTE_LDS)
                routes = {"workspace": fir.IfFirSynth.ROUTE_WORKSPACE, "ring": fir.IfFirSynth.ROUTE_LDS}
            except fir.IfFirError:
                routes = {}
            per = {name: [] for name in routes}
            for rep in range(args.reps + 1):
                for name, route in routes.items():
                    f.debug_config(route=route)
                    t = event_ms(torch, bank)
                    if rep:                       # (the first round warms both up)
                        per[name].append(t)
            for name in routes:
                row["route_ms"][name] = stats(per[name])
            f.synchronize()
        row["ms"], row["ms_min"], row["ms_max"] = stats(ms["bank"])
        row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = stats(ms["chain"])
        row["msps_out"] = n / row["ms"] / 1e3
        row["bytes_per_output"] = (4.0 if i16 else 8.0) * M / L + 8.0
        row["roofline"] = row["bytes_per_output"] * n / (row["ms"] * 1e-3) / ROOF
        row["chain_over_bank"] = row["chain_ms"] / row["ms"]
        rows.append(row)
        keep.clear()
        del out, X, x32, src, rows_t
        torch.cuda.empty_cache()
    lines = ["%-5s %-6s %-5s %-8s %10s %9s %19s %9s %9s %10s %21s %11s %10s" % ("M", "T", "L", "input", "outputs", "ms", "[min, max]", "MS/s out",
                                                                               "of 8TB/s", "chain ms", "[min, max]", "chain/bank", "max diff")]
    for r in rows:
        lines.append("%-5d %-6d %-5d %-8s %10d %9.4f [%8.4f,%8.4f] %9.1f %9.3f %10.3f [%9.3f,%9.3f] %11.2f %10.2g"
                     % (r["M"], r["taps"], r["L"], r["input"], r["outputs"], r["ms"], r["ms_min"], r["ms_max"], r["msps_out"], r["roofline"],
                        r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"], r["chain_over_bank"], r["chain_max_diff"]))
    lines.append("chain: torch.fft.ifft x M -> roll to the frame's output position, tile to J L -> x tap rows -> J overlapping slice additions, "
                 "complex64, from a zero history; max diff: a spread of 4096 outputs against the bank's, of the largest value")
    for r in rows:
        if "combiner_ms" in r:
            lines.append("IfFirCombiner C = 64, L = 64, centres k / 64, the same values one stream per channel: %.3f ms [%.3f, %.3f], %.1f x the "
                         "bank's; max diff %.2g" % (r["combiner_ms"], r["combiner_ms_min"], r["combiner_ms_max"], r["combiner_ms"] / r["ms"],
                                                    r["combiner_max_diff"]))
    lines.append("workspace budget (MB): median ms [min, max] of the workspace route alone, budgets alternating call by call")
    for r in rows:
        lines.append("%-5d %-6d %-5d %-8s " % (r["M"], r["taps"], r["L"], r["input"]) +
                     "   ".join("%s MB: %.4f [%.4f, %.4f]" % ((b,) + tuple(v)) for b, v in r["budget_ms"].items()))
    lines.append("routes (the table above is the plan's choice: 1 = workspace, 2 = LDS ring): median ms [min, max] of the bank alone, routes "
                 "alternating call by call")
    for r in rows:
        lines.append("%-5d %-6d %-5d %-8s plan %d   " % (r["M"], r["taps"], r["L"], r["input"], r["route"]) +
                     ("   ".join("%s: %.4f [%.4f, %.4f]" % ((k,) + tuple(v)) for k, v in r["route_ms"].items())
                      or "the ring does not fit two workgroups a CU: workspace only"))
    lines.append(json.dumps({"outputs": args.samples, "warmup": args.warmup, "reps": args.reps, "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
