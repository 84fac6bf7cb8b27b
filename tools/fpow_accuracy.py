#!/usr/bin/env python3
"""fpow_accuracy.py — the frame power stage's error against the float64 definition (tests/fpow_ref.py power_f64) over the matrix
of tests/test_fpow_gpu.py, float32 and int16 input: per case the worst relative error per bin in units of 2^-24 beside SPEC
§19's bound (G + ceil(K / 8) + 12) and whether the powers are the float32 order model's bits; then the chain
IfFirPfb(taps = reversed window) -> IfFirFpow against the float64 estimator at the two shapes of SPEC §19, beside the figure of a
plain complex64 model and the tolerance derived from it, and the estimator's own error on the same stream.  --out also writes
the text to a file."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import __graft_entry__ as g
    import fpow_ref
    import psd_ref
    import test_fpow_gpu as t
    import test_fpow_host as th
    fir = g.load_pkg().if_fir
    lines = ["%-5s %-5s %-3s %-5s %-6s %-8s %-7s %-12s %-6s %s" % ("B", "first", "G", "Bo", "K", "input", "frames", "units 2^-24", "bound", "model bits")]
    for B, first, G, Bo, K in fpow_ref.MATRIX:
        for i16 in (False, True):
            F = t.stream_frames(K)
            raw = t.signal(F, B, first, G, Bo, i16)
            v = fpow_ref.values_f32(raw, i16, B)
            with t.make(fir, B, first, G, Bo, K, i16, F) as f:
                _, power = f.process(raw)
            ref = fpow_ref.power_f64(v, first, G, Bo, K, t.NORM)
            live = ref > 0
            units = float(np.max(np.abs(power[live].astype(np.float64) - ref[live]) / ref[live]) * 2.0 ** 24)
            same = np.array_equal(power.view(np.uint32), t.model(F, B, first, G, Bo, K, i16).view(np.uint32))
            lines.append("%-5d %-5d %-3d %-5d %-6d %-8s %-7d %-12.2f %-6d %s" % (B, first, G, Bo, K, "int16" if i16 else "float32", power.shape[0],
                                                                                units, fpow_ref.bound_units(G, K), "same" if same else "DIFFER"))
    lines.append("chain IfFirPfb(N, taps = reversed Hann window, hop H) -> IfFirFpow(K) against psd_ref.power_f64, per frame of the frame's peak:")
    for N, H, K in fpow_ref.CHAIN_SHAPES:
        x = fpow_ref.chain_stream(N, H, K)
        w = psd_ref.hann(N)
        d, q = fpow_ref.chain_align(N, H)
        ref = psd_ref.power_f64(x, N, H, K, w)
        order = psd_ref.bin_indices(N, -N // 2, N)
        with fir.IfFirPfb(w[::-1].copy(), N, hop=H, max_samples=x.size // 2 + d) as bank, \
                fir.IfFirFpow(N, K, norm=float(np.sum(w.astype(np.float64) ** 2)), ref_power=fpow_ref.CHAIN_REF_POWER, max_frames=1 << 12) as f, \
                fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=fpow_ref.CHAIN_REF_POWER, window=w, max_samples=x.size // 2) as est:
            frames = bank.process(np.concatenate([np.zeros(2 * d, dtype=np.float32), x]))[q:]
            _, power = f.process(frames)
            _, epower = est.process(x)
        n = ref.shape[0]
        err = np.max(np.max(np.abs(power[:n][:, order].astype(np.float64) - ref), axis=1) / np.max(ref, axis=1))
        eerr = np.max(np.max(np.abs(epower.astype(np.float64) - ref), axis=1) / np.max(ref, axis=1))
        lines.append("N=%-5d H=%-4d K=%-2d bank -> stage %.3g, complex64 model %.3g, estimator %.3g"
                     % (N, H, K, err, th.chain_c64_error(N, H, K), eerr))
    lines.append("complex64 model's worst %.5g; tolerance of the chain CHAIN_EPS = 4 x that = %.5g (cap 1e-5); the estimator's own EPS %.5g"
                 % (fpow_ref.CHAIN_C64_WORST, fpow_ref.CHAIN_EPS, psd_ref.EPS))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
