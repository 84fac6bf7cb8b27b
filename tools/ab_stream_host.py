#!/usr/bin/env python3
"""ab_stream_host.py --libs a.so b.so ... [--rounds R] [--reps K] [--samples N] — host time per call of a small
process_device call of three streaming families (ddc, pfb, interp), several builds of the library alternately in ONE process
(development tool, in the manner of ab_inproc.py).  Every (family, library) pair gets its own context on the same resident
input.  A round times K back-to-back calls of N samples per pair with the host clock -- what the shim and the launch cost the
caller -- and synchronizes the context's stream outside the timed region; the pair that goes first rotates from round to
round.  Prints per pair the median / min / max of the round means in microseconds per call and the ratio to the first library.
Give the same build twice under two file names to see the spread of a build against itself."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as g  # noqa: E402

vp = ctypes.c_void_p


def open_ctx(fir, L, family, taps, max_samples):
    ctx, t = vp(), taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    if family == "ddc":
        ok = L.if_fir_ddc_init(ctypes.byref(ctx), t, 15, 4, max_samples, 0)
    elif family == "interp":
        ok = L.if_fir_interp_init(ctypes.byref(ctx), t, 15, 4, max_samples, 0)
    else:
        ok = L.if_fir_pfb_init(ctypes.byref(ctx), ctypes.byref(fir.PfbConfig(64, 32, -16, 32)), t, 131, max_samples, 0)
    if not ok:
        raise SystemExit(getattr(L, "if_fir_%s_last_error" % family)(None).decode())
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", required=True)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--samples", type=int, default=256)
    args = ap.parse_args()
    fir = g.load_pkg().if_fir
    torch.cuda.set_device(0)
    taps = np.linspace(-1.0, 1.0, 131, dtype=np.float32)
    x = torch.randn(2 * args.samples, dtype=torch.float32, device="cuda")
    y = torch.zeros(64 * args.samples, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for family in ("ddc", "pfb", "interp"):
        pairs = []
        for path in args.libs:
            L = fir._load(os.path.abspath(path), False)
            ctx = open_ctx(fir, L, family, taps, args.samples)
            pairs.append((os.path.basename(path), ctx, getattr(L, "if_fir_%s_process_device" % family),
                          getattr(L, "if_fir_%s_synchronize" % family), []))
        m = ctypes.c_uint64(0)
        xin, yout, n, pm = vp(x.data_ptr()), vp(y.data_ptr()), args.samples, ctypes.byref(m)
        for rnd in range(-3, args.rounds):   # three warm-up rounds
            for k in range(len(pairs)):
                name, ctx, call, sync, means = pairs[(k + rnd) % len(pairs)]
                ok = 1
                t0 = time.perf_counter_ns()
                for _ in range(args.reps):
                    ok &= call(ctx, xin, yout, n, pm)
                t1 = time.perf_counter_ns()
                if not ok or not sync(ctx):
                    raise SystemExit("%s %s: a call failed" % (family, name))
                if rnd >= 0:
                    means.append((t1 - t0) / args.reps / 1e3)
        base = statistics.median(pairs[0][4])
        for name, ctx, call, sync, means in pairs:
            med = statistics.median(means)
            print("%-7s %-22s median %7.3f us/call  min %7.3f  max %7.3f  ratio to %s %.4f" %
                  (family, name, med, min(means), max(means), pairs[0][0], med / base), flush=True)
        for path, (name, ctx, call, sync, means) in zip(args.libs, pairs):
            getattr(fir._load(os.path.abspath(path), False), "if_fir_%s_destroy" % family)(ctx)


if __name__ == "__main__":
    main()
