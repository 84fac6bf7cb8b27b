#!/usr/bin/env python3
"""fpow_bench.py — settled, in-process timing of the frame power stage (if_fir_fpow_t) against the route a user
has today, a torch chain, and the instrument comparison bank + stage against the power-spectrum estimator.

Rows (B elements per frame, G, K, frames per call): (918, 1, 64, 2^16), (1024, 1, 8, 2^16), (4097, 4, 16, 2^14), (8192, 8, 64,
2^13), (64, 1, 1024, 2^20), each with float32 and int16 input; Bo = B // G output bins from element 0.  --scale divides every
frame count (for a quick look).  The other side of each row, timed alternately with it call by call in the same process on
the same frames: (int16: to float32 times 2^-15 ->) re^2 + im^2 -> view(F / K, K, Bo, G).sum((1, 3)) -> times scale ->
10 log10 -> codes.  A spread of the powers is compared.  Order of a round: stage with codes, stage with codes and powers, chain --
the first follows the chain, the second follows the first and may find part of its frames in the Infinity Cache.
Per row: ms per call of the stage with codes only and with codes and powers (median, fastest and slowest of --reps timed calls
after --warmup, HIP events on a side stream), the chain's, the ratio, and the algorithmic bytes -- 8 or 4 per element in, 2 per
code out, 4 per power where asked for -- as a fraction of the 8 TB/s roofline (the chip's streaming-copy rate, about 6.3 TB/s,
is the practical ceiling: 0.79 of it).
Instrument comparison at 2^26 samples (--scale divides them): IfFirPfb(1024 channels, 8192 taps, hop 1024) + IfFirFpow(K = 64)
against IfFirPsd(1024, 1024, 64), and on the CPU the highest sidelobe of the two responses: what the extra time buys.
Ends with one JSON line; --out also writes the text to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF = 8e12
# (B, G, K, log2 frames)
SHAPES = ((918, 1, 64, 16), (1024, 1, 8, 16), (4097, 4, 16, 14), (8192, 8, 64, 13), (64, 1, 1024, 20))
ZERO_DB, FULL_DB = -3.35, 16.7


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


def highest_sidelobe_db(h, M, pad=32):
    """the highest sidelobe of the response of the real taps h, in dB below its value at 0: the largest value beyond the first
    minimum after the response has fallen to half (a flat passband has ripples of its own before that)"""
    import numpy as np
    H = np.abs(np.fft.rfft(h, pad * max(M, len(h))))
    H = H / H[0]
    k = int(np.argmax(H < 0.5))
    while k + 1 < H.size and H[k + 1] < H[k]:
        k += 1
    return float(20.0 * np.log10(np.max(H[k:])))


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
    code_dtype = getattr(torch, "uint16", torch.int32)
    slope = (FULL_DB - ZERO_DB) / 65535
    rows = []
    for B, G, K, logf in SHAPES:
        for i16 in (False, True):
            F = max(((1 << logf) // args.scale) // K * K, K)
            Bo, out = B // G, F // K
            norm, ref = 0.8125, 0.1
            scale = float(np.float32(1.0 / (K * G * norm)))
            gen = torch.Generator(device="cuda").manual_seed(B + K)
            if i16:
                src = torch.randint(-14000, 14001, (F, B, 2), dtype=torch.int16, device="cuda", generator=gen)
            else:
                src = torch.randn((F, B, 2), dtype=torch.float32, device="cuda", generator=gen) * 0.5
            codes = torch.zeros(out * Bo + 16, dtype=torch.int16, device="cuda")
            power = torch.zeros(out * Bo + 16, dtype=torch.float32, device="cuda")
            keep = {}
            row = {"B": B, "G": G, "K": K, "frames": F, "input": "int16" if i16 else "float32"}
            with fir.IfFirFpow(B, K, norm=norm, group=G, out_bins=Bo, ref_power=ref, input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32,
                               max_frames=F) as f:
                f.set_stream(stream)

                def chain():
                    v = src.to(torch.float32) * (2.0 ** -15) if i16 else src
                    p = (v[:, :Bo * G, 0] ** 2 + v[:, :Bo * G, 1] ** 2).view(out, K, Bo, G).sum((1, 3)) * scale
                    db = 10.0 * torch.log10(p / ref)
                    keep["chain_power"] = p
                    keep["chain_codes"] = torch.clamp(torch.round((db - ZERO_DB) / slope), 0, 65535).to(code_dtype)

                def stage():
                    keep["frames"] = f.process_device(src.data_ptr(), F, codes.data_ptr())

                def stage_power():
                    keep["frames"] = f.process_device(src.data_ptr(), F, codes.data_ptr(), power.data_ptr())

                stage_power()
                chain()
                torch.cuda.synchronize()
                assert keep["frames"] == out == keep["chain_power"].shape[0]
                want = keep["chain_power"].reshape(-1)
                at = torch.unique(torch.arange(4096, dtype=torch.int64) * (want.numel() - 1) // 4095).cuda()
                row["chain_max_diff"] = ((power[:out * Bo][at] - want[at]).abs() / want[at]).max().item()
                t = timed(torch, [stage, stage_power, chain], args.warmup, args.reps)
                f.synchronize()
            row["ms"], row["ms_min"], row["ms_max"] = t["stage"]
            row["power_ms"], row["power_ms_min"], row["power_ms_max"] = t["stage_power"]
            row["chain_ms"], row["chain_ms_min"], row["chain_ms_max"] = t["chain"]
            row["bytes"] = F * B * (4 if i16 else 8) + out * Bo * 2
            row["roofline"] = row["bytes"] / (row["ms"] * 1e-3) / ROOF
            row["power_roofline"] = (row["bytes"] + out * Bo * 4) / (row["power_ms"] * 1e-3) / ROOF
            row["chain_over_stage"] = row["chain_ms"] / row["ms"]
            rows.append(row)
            keep.clear()
            del src, codes, power, want
            torch.cuda.empty_cache()
    lines = ["%-5s %-3s %-5s %-8s %9s %9s %19s %9s %10s %19s %9s %10s %21s %12s %10s" % (
        "B", "G", "K", "input", "frames", "ms", "[min, max]", "of 8TB/s", "+power ms", "[min, max]", "of 8TB/s", "chain ms", "[min, max]",
        "chain/stage", "max diff")]
    for r in rows:
        lines.append("%-5d %-3d %-5d %-8s %9d %9.4f [%8.4f,%8.4f] %9.3f %10.4f [%8.4f,%8.4f] %9.3f %10.3f [%9.3f,%9.3f] %12.2f %10.2g"
                     % (r["B"], r["G"], r["K"], r["input"], r["frames"], r["ms"], r["ms_min"], r["ms_max"], r["roofline"], r["power_ms"],
                        r["power_ms_min"], r["power_ms_max"], r["power_roofline"], r["chain_ms"], r["chain_ms_min"], r["chain_ms_max"],
                        r["chain_over_stage"], r["chain_max_diff"]))
    lines.append("chain: (int16: to float32 times 2^-15 ->) re^2 + im^2 -> view(F / K, K, Bo, G).sum((1, 3)) -> times scale -> 10 log10 -> "
                 "round, clamp, to 16-bit codes; max diff: a spread of 4096 powers against the stage's, relative; of 8TB/s: 8 or 4 bytes "
                 "per element in, 2 per code out, 4 per power in the +power columns (the streaming-copy rate of the chip is about 0.79)")

    # ---- the instrument comparison: bank + stage against the estimator ----
    M, K = 1024, 64
    n = max((1 << 26) // args.scale, 4 * K * M) // (K * M) * (K * M)
    T = 8 * M
    tt = np.arange(T) - (T - 1) / 2.0
    h = (np.sinc(tt / M) * np.kaiser(T, 10.0)).astype(np.float32)
    h /= np.float32(np.sum(h))
    norm = float(np.sum(h.astype(np.float64) ** 2))
    hann = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(M) / M)).astype(np.float32)
    x = torch.randn(2 * n, dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(26)) * 0.5
    frames = n // M
    bank_out = torch.zeros(2 * frames * M + 16, dtype=torch.float32, device="cuda")
    c1 = torch.zeros(frames // K * M + 16, dtype=torch.int16, device="cuda")
    c2 = torch.zeros(frames // K * M + 16, dtype=torch.int16, device="cuda")
    inst = {"samples": n, "channels": M, "taps": T, "K": K}
    with fir.IfFirPfb(h, M, hop=M, max_samples=n) as bank, fir.IfFirFpow(M, K, norm=norm, ref_power=0.5, max_frames=frames) as f, \
            fir.IfFirPsd(M, M, K, -M // 2, M, ref_power=0.5, max_samples=n) as est:
        for c in (bank, f, est):
            c.set_stream(stream)
        got = {}

        def bank_and_stage():
            got["bank"] = bank.process_device(x.data_ptr(), bank_out.data_ptr(), n)
            got["stage"] = f.process_device(bank_out.data_ptr(), frames, c1.data_ptr())

        def stage_alone():
            got["stage"] = f.process_device(bank_out.data_ptr(), frames, c1.data_ptr())

        def estimator():
            got["est"] = est.process_device(x.data_ptr(), n, c2.data_ptr())

        t = timed(torch, [bank_and_stage, stage_alone, estimator], args.warmup, args.reps)
        assert got["bank"] == frames and got["stage"] == frames // K
        for c in (bank, f, est):
            c.synchronize()
    inst["bank_and_stage_ms"], inst["stage_ms"], inst["estimator_ms"] = t["bank_and_stage"], t["stage_alone"], t["estimator"]
    inst["sidelobe_db_bank"] = highest_sidelobe_db(h, M)
    inst["sidelobe_db_hann"] = highest_sidelobe_db(hann, M)
    lines.append("instrument, %d samples: IfFirPfb(%d channels, %d taps, hop %d) + IfFirFpow(K = %d) %.3f ms [%.3f, %.3f], of which the stage "
                 "%.3f ms [%.3f, %.3f]; IfFirPsd(%d, %d, %d) %.3f ms [%.3f, %.3f]"
                 % ((n, M, T, M, K) + t["bank_and_stage"] + t["stage_alone"] + (M, M, K) + t["estimator"]))
    lines.append("what the extra time buys (CPU, float64 transform of the taps): highest sidelobe of the bank's prototype (sinc x Kaiser 10, "
                 "%d taps) %.1f dB, of the estimator's Hann window (%d taps) %.1f dB" % (T, inst["sidelobe_db_bank"], M, inst["sidelobe_db_hann"]))
    lines.append(json.dumps({"scale": args.scale, "warmup": args.warmup, "reps": args.reps, "rows": rows, "instrument": inst}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
