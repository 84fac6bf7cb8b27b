#!/usr/bin/env python3
"""psd_bench.py — settled, in-process timing of the streaming power-spectrum estimator (if_fir_psd_t).

Workloads: 2^26 samples, float32 and int16 input; N = 1024, K = 64, 918 centred bins; H = N and H = N / 2.  Per case: ms per
call of if_fir_psd_process_device (its chunk, frame and carry kernels together; median of --reps timed calls after --warmup, HIP
events on a side stream; the calls are one stream continued), input GS/s, and the bytes the estimator must move -- 8 per
sample (4 for int16) in, the frames out -- as a fraction of the 8 TB/s roofline.  Beside it, in the same run and on the same
data: torch.stft -> abs()^2 -> mean over each frame's K segments (int16: the conversion to complex64 included, since torch.stft
takes no int16).  Ends with one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8e12
N, K, FIRST, BINS = 1024, 64, -459, 918


def timed(torch, fn, warmup, reps):
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
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    n = args.samples - args.samples % (K * N)   # whole frames at either hop: every call after the first emits the same count
    x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    with fir.IfFir(fir.bpf_design(255), decimation=1, max_samples=1024) as f:
        f.set_stream(stream)
        f.synth_device(x.data_ptr(), 0, n, 0)
        f.synchronize()
    xi = (x * 8192.0).round().clamp(-32768, 32767).to(torch.int16)
    hann = torch.hann_window(N, periodic=True, dtype=torch.float32, device="cuda")
    rows = []
    for i16 in (False, True):
        for H in (N, N // 2):
            frames = n // (K * H)
            codes = torch.empty((frames + 1) * BINS, dtype=torch.int16, device="cuda")
            power = torch.empty((frames + 1) * BINS, dtype=torch.float32, device="cuda")
            src = xi if i16 else x
            row = {"input": "int16" if i16 else "float32", "N": N, "H": H, "K": K, "bins": BINS, "samples": n}
            with fir.IfFirPsd(N, H, K, FIRST, BINS, ref_power=1.0, input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32,
                              max_samples=n) as f:
                f.set_stream(stream)
                emitted = []

                def one():
                    emitted.append(f.process_device(src.data_ptr(), n, codes.data_ptr(), power.data_ptr()))

                row["ms"] = timed(torch, one, args.warmup, args.reps)
                assert emitted[-1] == frames, (emitted, frames)
            row["frames_per_call"] = frames
            row["gsps_in"] = n / row["ms"] / 1e6
            row["bytes"] = n * (4 if i16 else 8) + frames * BINS * 6
            row["roofline"] = row["bytes"] / (row["ms"] * 1e-3) / ROOF

            def chain():
                xc = torch.view_as_complex((src.to(torch.float32) * (1.0 / 32768.0) if i16 else src).view(-1, 2))
                s = torch.stft(xc, n_fft=N, hop_length=H, win_length=N, window=hann, center=False, return_complex=True)
                p = s.abs() ** 2
                whole = (p.shape[1] // K) * K
                return p[:, :whole].view(N, -1, K).mean(dim=2)

            row["stft_ms"] = timed(torch, chain, args.warmup, args.reps)
            row["speedup_vs_stft"] = row["stft_ms"] / row["ms"]
            del codes, power
            torch.cuda.empty_cache()
            rows.append(row)
    print("%-8s %5s %5s %10s %10s %9s %9s %10s %8s" % ("input", "N", "H", "samples", "ms", "GS/s in", "of 8TB/s", "stft ms", "speedup"))
    for r in rows:
        print("%-8s %5d %5d %10d %10.4f %9.2f %9.3f %10.4f %8.2f" % (r["input"], r["N"], r["H"], r["samples"], r["ms"], r["gsps_in"],
                                                                     r["roofline"], r["stft_ms"], r["speedup_vs_stft"]))
    print(json.dumps({"samples_requested": args.samples, "warmup": args.warmup, "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
