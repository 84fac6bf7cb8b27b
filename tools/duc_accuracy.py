#!/usr/bin/env python3
"""duc_accuracy.py — the real-output up-converter's error against the float64 definition over the two matrices of
tests/test_duc_gpu.py (designed image-rejection taps; taps loud at both ends of every phase row; both scaled to a float64 peak
of 0.9, on the streams of tests/duc_ref.py), each row with the NCO off and at its own frequency: the worst l2 and max figure of
the float32 output and the worst difference of the int16 output in LSB, per kernel instantiation and kind of taps.  SPEC §3's
bound is 1e-6 for both metrics; SPEC §11's is 1 LSB."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import __graft_entry__ as g
    import duc_ref
    import test_duc_gpu as t
    fir = g.load_pkg().if_fir
    worst = {}
    for loud in (False, True):
        for T, L, ct, i16 in t.CASES:
            n = duc_ref.stream_len(T, L)
            raw, _ = t.signal(n, i16)
            for freq in (0.0, t.FREQS[t.MATRIX.index((T, L))]):
                taps, ref = t.scaled_case(fir, T, L, ct, i16, n, duc_ref.phase_word(freq), loud)
                with fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct) as f:
                    if i16:
                        f.set_input_format(fir.INPUT_I16)
                    f.set_nco(freq)
                    l2, mx = duc_ref.metrics(f.process(raw), ref)
                    f.reset()
                    f.set_output_format(fir.OUTPUT_I16)
                    lsb = int(np.max(np.abs(f.process(raw).astype(np.int64) - duc_ref.to_i16(ref).astype(np.int64))))
                inst = "fir_duc_kernel<%s in>, %s %s taps, NCO %s" % ("int16" if i16 else "float32", "loud" if loud else "designed",
                                                                     "complex" if ct else "real", "on" if freq else "off")
                w = worst.setdefault(inst, [0.0, 0.0, 0, None, None, 0])
                w[2] += 1
                if l2 > w[0]:
                    w[0], w[3] = l2, (T, L)
                if mx > w[1]:
                    w[1], w[4] = mx, (T, L)
                w[5] = max(w[5], lsb)
    print("%-62s %5s  %-10s %-12s %-10s %-12s %s" % ("instantiation, taps, NCO", "cases", "worst l2", "at (T, L)", "worst max", "at (T, L)",
                                                     "int16 LSB"))
    for inst in sorted(worst):
        w = worst[inst]
        print("%-62s %5d  %-10.3g %-12s %-10.3g %-12s %d" % (inst, w[2], w[0], w[3], w[1], w[4], w[5]))
    print("overall: l2 %.3g, max %.3g of the peak, bound 1e-6 (docs/SPEC.md §3); int16 output %d LSB, bound 1 (docs/SPEC.md §11)"
          % (max(w[0] for w in worst.values()), max(w[1] for w in worst.values()), max(w[5] for w in worst.values())))


if __name__ == "__main__":
    main()
