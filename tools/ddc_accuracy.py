#!/usr/bin/env python3
"""ddc_accuracy.py — the real-input down-converter's error against the float64 definition over the matrices of
tests/test_ddc_gpu.py (designed low-pass taps on 60 000 samples; taps loud at both ends of every phase row on the streams of
tests/ddc_ref.py), each row with the NCO off and at its own frequency: the worst l2 and max figure per kernel instantiation and
kind of taps.  SPEC §3's bound is 1e-6 for both."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import __graft_entry__ as g
    import ddc_ref
    import test_ddc_gpu as t
    from matrix_util import row_edge_taps
    fir, oracle = g.load_pkg().if_fir, g.load_oracle()
    worst = {}
    for loud, rows in ((False, t.MATRIX), (True, t.LOUD_MATRIX)):
        for T, D, ct, i16 in t.matrix_cases(rows):
            n = ddc_ref.stream_len(T, D) if loud else 60_000
            raw, x = t.signal(n, i16)
            taps = row_edge_taps(T, D, ct) if loud else t.taps_for(fir, T, D, ct)
            with fir.IfFirDdc(taps, D, max_samples=n, complex_taps=ct) as f:
                if i16:
                    f.set_input_format(fir.INPUT_I16)
                for freq in (0.0, t.FREQS[t.LOUD_MATRIX.index((T, D)) % len(t.FREQS)]):
                    f.set_nco(freq)
                    f.reset()
                    ref = ddc_ref.ddc_f64(taps, x, D, ddc_ref.phase_word(freq), ct)
                    l2, mx = oracle.err_metrics(f.process(raw), ref)
                    inst = "fir_ddc_kernel<%s>, %s %s taps, NCO %s" % ("int16" if i16 else "float32", "loud" if loud else "designed",
                                                                        "complex" if ct else "real", "on" if freq else "off")
                    w = worst.setdefault(inst, [0.0, 0.0, 0, None, None])
                    w[2] += 1
                    if l2 > w[0]:
                        w[0], w[3] = l2, (T, D)
                    if mx > w[1]:
                        w[1], w[4] = mx, (T, D)
    print("%-62s %5s  %-10s %-12s %-10s %-12s" % ("instantiation, taps, NCO", "cases", "worst l2", "at (T, D)", "worst max", "at (T, D)"))
    for inst in sorted(worst):
        w = worst[inst]
        print("%-62s %5d  %-10.3g %-12s %-10.3g %-12s" % (inst, w[2], w[0], w[3], w[1], w[4]))
    print("overall: l2 %.3g, max %.3g of the peak; bound 1e-6 (docs/SPEC.md §3)" % (max(w[0] for w in worst.values()),
                                                                                    max(w[1] for w in worst.values())))


if __name__ == "__main__":
    main()
