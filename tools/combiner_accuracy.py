#!/usr/bin/env python3
"""combiner_accuracy.py — the channel combiner's error against the float64 definition over the matrix of
tests/test_combiner_gpu.py (tests/combiner_ref.py: cases, signals, centres, reference), the worst l2 and max figure per kernel
instantiation: overlap-save (overlap rows x input format) and generic (tap kind x input format).  SPEC §3's bound is 1e-6 for both.
Same calls as the test: one call per case, at most two workgroups."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import __graft_entry__ as g
    import combiner_ref as cr
    fir, oracle = g.load_pkg().if_fir, g.load_oracle()
    worst = {}
    for route in ("fft", "generic"):
        for L, C, T, ct, i16 in cr.cases(route):
            taps, raw, _, centres, _, ref = cr.case_reference(L, C, T, ct, i16)
            n = raw[0].size // 2
            with fir.IfFirCombiner(taps, L, centres, max_samples=n, complex_taps=ct, dev=True) as f:
                if route == "generic":
                    f.set_backend(fir.BACKEND_HIP_GENERIC)
                f.debug_config(grid_limit=2)
                if i16:
                    f.set_input_format(fir.INPUT_I16)
                l2, mx = oracle.err_metrics(f.process(raw), ref)
            inst = ("fir_combiner_kernel<rows=%d, %s>" % (cr.overlap_rows(T), "int16" if i16 else "float32") if route == "fft" else
                    "fir_combiner_generic_kernel<%s, %s taps>" % ("int16" if i16 else "float32", "complex" if ct else "real"))
            w = worst.setdefault(inst, [0.0, 0.0, 0, None, None])
            w[2] += 1
            if l2 > w[0]:
                w[0], w[3] = l2, (L, C, T)
            if mx > w[1]:
                w[1], w[4] = mx, (L, C, T)
    print("%-52s %5s  %-10s %-16s %-10s %-16s" % ("instantiation", "cases", "worst l2", "at (L, C, T)", "worst max", "at (L, C, T)"))
    for inst in sorted(worst):
        w = worst[inst]
        print("%-52s %5d  %-10.3g %-16s %-10.3g %-16s" % (inst, w[2], w[0], w[3], w[1], w[4]))
    print("overall: l2 %.3g, max %.3g of the peak; bound 1e-6 (docs/SPEC.md §3)" % (max(w[0] for w in worst.values()),
                                                                                    max(w[1] for w in worst.values())))


if __name__ == "__main__":
    main()
