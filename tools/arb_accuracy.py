#!/usr/bin/env python3
"""arb_accuracy.py — the arbitrary-ratio resampler's error against the float64 definition over the two matrices of
tests/test_arb_gpu.py (designed low-pass taps; taps loud at both ends of every phase row), the rows of the segment and unroll
remainders included, on the streams of tests/arb_ref.py: the worst l2 and max figure per kernel instantiation and kind of
taps, and beside each the same figure of the float32 model of SPEC §12's order.  SPEC §3's bound is 1e-6 for both metrics."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import __graft_entry__ as g
    import arb_ref
    import test_arb_gpu as t
    fir = g.load_pkg().if_fir
    oracle = g.load_oracle()
    worst = {}
    for loud in (False, True):
        for b, T, R in t.MATRIX + t.REMAINDERS:
            for i16 in (False, True):
                n = arb_ref.stream_len(T, b, R)
                raw, x = t.signal(n, i16)
                taps = t.make_taps(T, b, R, loud)
                ref, _ = arb_ref.resample_f64(taps, x, b, R)
                with fir.IfFirArb(taps, b, R, max_samples=n) as f:
                    if i16:
                        f.set_input_format(fir.INPUT_I16)
                    l2, mx = oracle.err_metrics(f.process(raw), ref)
                ml2, mmx = oracle.err_metrics(arb_ref.resample_f32_order(taps, x, b, R), ref)
                inst = "fir_arb_kernel<%s in>, %s taps" % ("int16" if i16 else "float32", "loud" if loud else "designed")
                w = worst.setdefault(inst, [0.0, 0.0, 0, None, None, 0.0, 0.0])
                w[2] += 1
                if l2 > w[0]:
                    w[0], w[3] = l2, (b, T, R)
                if mx > w[1]:
                    w[1], w[4] = mx, (b, T, R)
                w[5], w[6] = max(w[5], ml2), max(w[6], mmx)
    print("%-42s %5s  %-10s %-24s %-10s %-24s %-10s %s" % ("instantiation, taps", "cases", "worst l2", "at (b, T, R)", "worst max", "at (b, T, R)",
                                                            "model l2", "model max"))
    for inst in sorted(worst):
        w = worst[inst]
        print("%-42s %5d  %-10.3g %-24s %-10.3g %-24s %-10.3g %.3g" % (inst, w[2], w[0], w[3], w[1], w[4], w[5], w[6]))
    print("overall: l2 %.3g, max %.3g of the peak, bound 1e-6 (docs/SPEC.md §3); the float32 model of the order: l2 %.3g, max %.3g"
          % (max(w[0] for w in worst.values()), max(w[1] for w in worst.values()), max(w[5] for w in worst.values()),
             max(w[6] for w in worst.values())))


if __name__ == "__main__":
    main()
