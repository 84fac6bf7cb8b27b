#!/usr/bin/env python3
"""rsynth_accuracy.py — the real-output polyphase synthesis bank's error against float64 (the half-size fold form of
tests/rsynth_ref.py) over the matrix of tests/test_rsynth_gpu.py and SPEC §18's model matrix of tests/test_rsynth_host.py (taps
loud at both ends of every row), float32 and int16 input: the worst l2 and max figure per transform instantiation, taken over
the whole output of a case, and beside each the same figure of the float32 model.  The bound (SPEC §18) is twice the model's
worst per metric.  --out also writes the text to a file."""
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
    import __graft_entry__ as g
    import rsynth_ref
    import test_rsynth_gpu as t
    import test_rsynth_host as th
    from matrix_util import row_edge_taps
    fir = g.load_pkg().if_fir
    oracle = g.load_oracle()
    worst = {}
    cases = list(t.MATRIX) + [c for c in th.model_matrix() if c not in t.MATRIX]
    for M, T, L in cases:
        for i16 in (False, True):
            F = t.stream_frames(M, T, L) if (M, T, L) in t.MATRIX else 2 * rsynth_ref.terms(T, L) + 6
            raw, X = t.frames_signal(oracle, F, M // 2 + 1, i16)
            taps = row_edge_taps(T, L, False)
            ref = rsynth_ref.fold_f64(taps, X, M, L)
            with fir.IfFirRsynth(taps, M, L, max_frames=F) as f:
                if i16:
                    f.set_input_format(fir.INPUT_I16)
                l2, mx = oracle.err_metrics(f.process(raw), ref)
            ml2, mmx = oracle.err_metrics(rsynth_ref.model_f32(taps, X, M, L), ref)
            inst = "rsynth_transform_kernel<%d, %s in>" % (M, "int16" if i16 else "float32")
            w = worst.setdefault(inst, [0.0, 0.0, 0, None, None, 0.0, 0.0, M, i16])
            w[2] += 1
            if l2 > w[0]:
                w[0], w[3] = l2, (T, L)
            if mx > w[1]:
                w[1], w[4] = mx, (T, L)
            w[5], w[6] = max(w[5], ml2), max(w[6], mmx)
    lines = ["%-46s %5s  %-10s %-16s %-10s %-16s %-10s %s" % ("instantiation (+ rsynth_emit_kernel<float32>)", "cases", "worst l2", "at (T, L)",
                                                             "worst max", "at (T, L)", "model l2", "model max")]
    for inst in sorted(worst, key=lambda k: (worst[k][7], worst[k][8])):
        w = worst[inst]
        lines.append("%-46s %5d  %-10.3g %-16s %-10.3g %-16s %-10.3g %.3g" % (inst, w[2], w[0], w[3], w[1], w[4], w[5], w[6]))
    lines.append("overall: l2 %.3g, max %.3g of the peak, bound l2 %.3g, max %.3g (docs/SPEC.md §18); the float32 model: l2 %.3g, max %.3g"
                 % (max(w[0] for w in worst.values()), max(w[1] for w in worst.values()), t.TOL_L2, t.TOL_MAX,
                    max(w[5] for w in worst.values()), max(w[6] for w in worst.values())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
