#!/usr/bin/env python3
"""sub_accuracy.py — the per-channel FIR stage's error against the float64 decimator it is defined by (tests/sub_ref.py
channel_f64: oracle.fir_nco_f64 per bin) over the matrix of tests/test_sub_gpu.py (taps loud at both ends of every row), float32
and int16 input, NCO words all 0 and mixed: the l2 and max figure over the whole output of a case (SPEC §15), and beside each
the same figure of the complex64 model.  The bound is 1e-6 for both metrics.  --out also writes the text to a file."""
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
    import sub_ref
    import test_sub_gpu as t
    from matrix_util import signal
    fir = g.load_pkg().if_fir
    oracle = g.load_oracle()
    lines = ["%-6s %-4s %-5s %-3s %-8s %-6s %-10s %-10s %-10s %s" % ("B", "T", "rows", "R", "input", "words", "l2", "max", "model l2", "model max")]
    worst = [0.0, 0.0, 0.0, 0.0]
    for B, T, rows, R in t.MATRIX:
        for i16 in (False, True):
            for mixed in (False, True):
                F = t.stream_frames(B)
                raw, xf = signal(oracle, F * B, i16)
                taps, words = t.taps_of(B, T, rows), t.words_of(B, mixed)
                ref = sub_ref.iq(t.reference(B, T, rows, R, i16, mixed, F))
                with fir.IfFirSub(taps, B, R, max_frames=F) as f:
                    if i16:
                        f.set_input_format(fir.INPUT_I16)
                    f.set_nco(t.freqs_of(B, mixed))
                    got = oracle.err_metrics(sub_ref.iq(f.process(raw)), ref)
                model = oracle.err_metrics(sub_ref.iq(sub_ref.model_c64(taps, xf.view(np.complex64).reshape(F, B), R, words)), ref)
                worst = [max(a, b) for a, b in zip(worst, got + model)]
                lines.append("%-6d %-4d %-5d %-3d %-8s %-6s %-10.3g %-10.3g %-10.3g %.3g" % (
                    B, T, rows, R, "int16" if i16 else "float32", "mixed" if mixed else "0", got[0], got[1], model[0], model[1]))
    lines.append("overall: l2 %.3g, max %.3g of the peak, bound 1e-6 (docs/SPEC.md §15); the complex64 model: l2 %.3g, max %.3g" % tuple(worst))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
