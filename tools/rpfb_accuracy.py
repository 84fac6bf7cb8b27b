#!/usr/bin/env python3
"""rpfb_accuracy.py — the real-input polyphase filter bank's error against the float64 fold form of tests/rpfb_ref.py over the
matrix of tests/test_rpfb_gpu.py (taps loud at both ends of every row), float32 and int16 input: the worst l2 and max figure per
kernel instantiation, taken over the whole output of a case (all channels of all frames together, SPEC §17), and beside each the
same figure of the float32 model.  The bound is 1e-6 for both metrics.  --out also writes the text to a file."""
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
    import rpfb_ref
    import test_rpfb_gpu as t
    from matrix_util import row_edge_taps
    fir = g.load_pkg().if_fir
    oracle = g.load_oracle()
    worst = {}
    for M, T, D in t.MATRIX:
        for i16 in (False, True):
            n = t.stream_len(M, T, D)
            raw, x = t.signal(n, i16)
            taps = row_edge_taps(T, M, False)
            ref = rpfb_ref.iq(rpfb_ref.fold_f64(taps, x, M, D))
            with fir.IfFirRpfb(taps, M, D, max_samples=n) as f:
                if i16:
                    f.set_input_format(fir.INPUT_I16)
                l2, mx = oracle.err_metrics(rpfb_ref.iq(f.process(raw)), ref)
            ml2, mmx = oracle.err_metrics(rpfb_ref.iq(rpfb_ref.model_c64(taps, x, M, D)), ref)
            inst = "rpfb_kernel<%d, %s in>" % (M, "int16" if i16 else "float32")
            w = worst.setdefault(inst, [0.0, 0.0, 0, None, None, 0.0, 0.0, M, i16])
            w[2] += 1
            if l2 > w[0]:
                w[0], w[3] = l2, (T, D)
            if mx > w[1]:
                w[1], w[4] = mx, (T, D)
            w[5], w[6] = max(w[5], ml2), max(w[6], mmx)
    lines = ["%-32s %5s  %-10s %-16s %-10s %-16s %-10s %s" % ("instantiation", "cases", "worst l2", "at (T, D)", "worst max", "at (T, D)", "model l2",
                                                             "model max")]
    for inst in sorted(worst, key=lambda k: (worst[k][7], worst[k][8])):
        w = worst[inst]
        lines.append("%-32s %5d  %-10.3g %-16s %-10.3g %-16s %-10.3g %.3g" % (inst, w[2], w[0], w[3], w[1], w[4], w[5], w[6]))
    lines.append("overall: l2 %.3g, max %.3g of the peak, bound 1e-6 (docs/SPEC.md §17); the float32 model: l2 %.3g, max %.3g"
                 % (max(w[0] for w in worst.values()), max(w[1] for w in worst.values()), max(w[5] for w in worst.values()),
                    max(w[6] for w in worst.values())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
