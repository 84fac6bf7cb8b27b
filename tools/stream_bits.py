#!/usr/bin/env python3
"""stream_bits.py — the output bits of the streaming families (interpolator, channel combiner, rational resampler, power spectrum)
for a fixed seed and a short fixed list of small cases, written to one .npz; and the comparison of two such files.

A refactor of the kernels must leave every output the same bits (the compiler may fuse multiply-adds across statements, so this is
observed, not assumed): run `stream_bits.py OUT.npz` from the tree before and from the tree after -- each run imports the package
beside this file, as the bench tools do -- then `stream_bits.py --compare A.npz B.npz`, which exits non-zero unless both files hold
the same arrays with the same bytes.  Every stream is fed in three unequal pieces.

Cases: interpolator, overlap-save route at L = 1, 4, 64 and generic route at L = 5, each with T = 31, 257, 1023, real and complex
taps, float32 and int16 input, NCO off and on; combiner, overlap-save (L = 8, C = 8, T = 255, complex taps) and generic (L = 5,
C = 3, T = 31); resampler 2/3 at T = 63 and 25/24 at T = 801, real and complex taps; power spectrum N = 256, 512, 4096 with
H = N / 2, K = 8, int16 and float32."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261019


def pieces(n):
    """three unequal cuts of n samples"""
    a, b = n // 7, n // 7 + n // 2
    return (0, a), (a, b), (b, n)


def stream_input(rng, n, i16):
    """n samples as an interleaved array: float32 in [-1, 1), or int16"""
    if i16:
        return rng.integers(-32768, 32768, 2 * n).astype(np.int16)
    return rng.uniform(-1.0, 1.0, 2 * n).astype(np.float32)


def taps_of(rng, T, ct):
    return (rng.standard_normal(2 * T if ct else T) / T).astype(np.float32)


def run_cases(fir):
    rng = np.random.default_rng(SEED)
    out = {}
    for route, backend, Ls in (("fft", fir.BACKEND_HIP_FFT, (1, 4, 64)), ("generic", fir.BACKEND_HIP_GENERIC, (5,))):
        for L in Ls:
            n = 9001 // L + 160   # three or more blocks of the overlap-save kernel, the last one partial
            for T in (31, 257, 1023):
                for ct in (False, True):
                    h = taps_of(rng, T, ct)
                    for i16 in (False, True):
                        x = stream_input(rng, n, i16)
                        for nco in (0.0, 0.1234567):
                            with fir.IfFirInterp(h, L, max_samples=n, backend=backend, complex_taps=ct) as f:
                                assert f.get_backend() == backend
                                if i16:
                                    f.set_input_format(fir.INPUT_I16)
                                f.set_nco(nco)
                                y = np.concatenate([f.process(x[2 * a:2 * b]) for a, b in pieces(n)])
                            out["interp_%s_L%d_T%d_%s_%s_%s" % (route, L, T, "ct" if ct else "rt", "i16" if i16 else "f32",
                                                               "nco" if nco else "plain")] = y
    for route, backend, L, C, T, ct in (("fft", fir.BACKEND_HIP_FFT, 8, 8, 255, True), ("generic", fir.BACKEND_HIP_GENERIC, 5, 3, 31, False)):
        n = 9001 // L + 160
        h = taps_of(rng, T, ct)
        centres = np.linspace(-0.4, 0.4, C) + 1.0e-4   # off the 1/4096 grid: every channel has a residual
        for i16 in (False, True):
            xs = [stream_input(rng, n, i16) for _ in range(C)]
            with fir.IfFirCombiner(h, L, centres, max_samples=n, backend=backend, complex_taps=ct) as f:
                assert f.get_backend() == backend
                if i16:
                    f.set_input_format(fir.INPUT_I16)
                y = np.concatenate([f.process([x[2 * a:2 * b] for x in xs]) for a, b in pieces(n)])
            out["combiner_%s_%s" % (route, "i16" if i16 else "f32")] = y
    for L, M, T in ((2, 3, 63), (25, 24, 801)):
        n = 20011
        for ct in (False, True):
            h = taps_of(rng, T, ct)
            for i16 in (False, True):
                x = stream_input(rng, n, i16)
                with fir.IfFirResamp(h, L, M, max_samples=n, complex_taps=ct) as f:
                    if i16:
                        f.set_input_format(fir.INPUT_I16)
                    y = np.concatenate([f.process(x[2 * a:2 * b]) for a, b in pieces(n)])
                out["resamp_%d_%d_T%d_%s_%s" % (L, M, T, "ct" if ct else "rt", "i16" if i16 else "f32")] = y
    for N in (256, 512, 4096):
        H, K = N // 2, 8
        n = H * K * 5 + N + 77   # five frames and an open one
        for i16 in (True, False):
            x = stream_input(rng, n, i16)
            with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32,
                              max_samples=n) as f:
                got = [f.process(x[2 * a:2 * b]) for a, b in pieces(n)]
            key = "psd_N%d_%s" % (N, "i16" if i16 else "f32")
            out[key + "_codes"] = np.concatenate([g[0] for g in got])
            out[key + "_power"] = np.concatenate([g[1] for g in got])
    return out


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            bad.append(k)
    print("%d arrays in %s, %d in %s, %d differ or are missing%s" % (len(a.files), path_a, len(b.files), path_b, len(bad),
                                                                   ": " + ", ".join(bad) if bad else ""))
    return 1 if bad or not a.files else 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import __graft_entry__ as g
    out = run_cases(g.load_pkg().if_fir)
    np.savez(sys.argv[1], **out)
    print("%d arrays, %d bytes to %s" % (len(out), sum(v.nbytes for v in out.values()), sys.argv[1]))


if __name__ == "__main__":
    main()
