#!/usr/bin/env python3
"""subup_accuracy.py — the per-bin interpolating FIR stage's error against the float64 interpolator it is defined by
(tests/subup_ref.py channel_f64: combiner_ref.reference per bin) over the matrix of tests/test_subup_gpu.py (every phase's taps
loud at both ends), float32 and int16 input, NCO words all 0 and mixed: the l2 and max figure over the whole output of a case
(SPEC §16), and beside each the same figure of the complex64 model.  The bound is 1e-6 for both metrics.  --out also writes the
text to a file."""
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
    import subup_ref
    import test_subup_gpu as t
    from matrix_util import signal
    fir = g.load_pkg().if_fir
    oracle = g.load_oracle()
    lines = ["%-6s %-5s %-5s %-3s %-8s %-6s %-10s %-10s %-10s %s" % ("B", "T", "rows", "R", "input", "words", "l2", "max", "model l2", "model max")]
    worst = [0.0, 0.0, 0.0, 0.0]
    for B, T, rows, R in t.MATRIX:
        for i16 in (False, True):
            for mixed in (False, True):
                F = t.stream_frames(B, R)
                raw, xf = signal(oracle, F * B, i16)
                taps, words = t.taps_of(B, T, rows, R), t.words_of(B, mixed)
                ref = subup_ref.iq(t.reference(B, T, rows, R, i16, mixed, F))
                with fir.IfFirSubUp(taps, B, R, max_frames=F) as f:
                    if i16:
                        f.set_input_format(fir.INPUT_I16)
                    f.set_nco(t.freqs_of(B, mixed))
                    got = oracle.err_metrics(subup_ref.iq(f.process(raw)), ref)
                model = oracle.err_metrics(subup_ref.iq(subup_ref.model_c64(taps, xf.view(np.complex64).reshape(F, B), R, words)), ref)
                worst = [max(a, b) for a, b in zip(worst, got + model)]
                lines.append("%-6d %-5d %-5d %-3d %-8s %-6s %-10.3g %-10.3g %-10.3g %.3g" % (
                    B, T, rows, R, "int16" if i16 else "float32", "mixed" if mixed else "0", got[0], got[1], model[0], model[1]))
    lines.append("overall: l2 %.3g, max %.3g of the peak, bound 1e-6 (docs/SPEC.md §16); the complex64 model: l2 %.3g, max %.3g" % tuple(worst))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
