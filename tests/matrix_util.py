"""Taps, streams and the comparison shared by the per-instantiation matrices (tests/test_interp_matrix_gpu.py,
tests/test_fft_matrix_gpu.py, tests/test_resamp_gpu.py).  Plain functions, like tests/bank_ref.py.

The taps are not a windowed design (whose end taps are zero, and the next ones 1e-6 of the peak): the first and the last tap
are the largest of the set, so one tap wrapped into the kept region or one sample missing from the history costs about
1/sqrt(T) of the output norm."""
import numpy as np

TOL = 1e-6   # docs/SPEC.md §3: relative, norm-wise and max-wise


def as_c(y):
    y = np.asarray(y, dtype=np.float64).reshape(-1, 2)
    return y[:, 0] + 1j * y[:, 1]


def as_iq(c):
    return np.stack([c.real, c.imag], axis=1).reshape(-1)


def edge_taps(T, L, complex_taps, seed=0):
    """seeded normal taps, |h| <= 0.5 inside, the first tap +1 and the last -1 (complex: -j), the whole set scaled to an
    output level of O(1): sum |h|^2 = L.  float32; complex taps interleaved (re, im)."""
    rng = np.random.default_rng([T, L, int(complex_taps), seed])
    h = rng.standard_normal(T).astype(np.float32).astype(np.complex128)
    if complex_taps:
        h = h + 1j * rng.standard_normal(T).astype(np.float32)
    h *= 0.5 / np.max(np.abs(h))
    h[0] = 1.0
    if T > 1:
        h[-1] = -1j if complex_taps else -1.0
    h *= np.sqrt(L / np.sum(np.abs(h) ** 2))
    if complex_taps:
        return as_iq(h).astype(np.float32)
    return h.real.astype(np.float32)


def row_edge_taps(T, L, complex_taps, seed=0):
    """edge_taps for a polyphase filter with rows g[p][j] = h[p + j L]: seeded normal taps, |h| <= 0.5 inside, every phase's
    first tap (the first min(L, T) taps) of magnitude 1 with alternating sign, every phase's highest tap (the last min(L, T)
    taps) the same negated (complex: times -j), the whole set scaled to sum |h|^2 = L.  With T <= L every phase has one tap,
    which is both ends and keeps the first form; L = 1 gives edge_taps' ends, first tap +, last tap - (complex: -j).
    float32; complex taps interleaved (re, im)."""
    rng = np.random.default_rng([T, L, int(complex_taps), seed, 77])
    h = rng.standard_normal(T).astype(np.complex128)
    if complex_taps:
        h = h + 1j * rng.standard_normal(T)
    h *= 0.5 / np.max(np.abs(h))
    e = min(L, T)
    sgn = np.where(np.arange(e) % 2 == 0, 1.0, -1.0).astype(np.complex128)
    h[:e] = sgn
    if T > e:
        h[T - e:] = (-1j if complex_taps else -1.0) * sgn[::-1]
    h *= np.sqrt(L / np.sum(np.abs(h) ** 2))
    if complex_taps:
        return as_iq(h).astype(np.float32)
    return h.real.astype(np.float32)


_signals = {}


def signal(oracle, n, i16):
    """(what the library is given, the same samples as float32).  int16: level 14000 with full-scale samples, 32767 and -32768
    on I and on Q, at the ends, scattered, and in a run"""
    if (n, i16) not in _signals:
        x = oracle.synth_iq(n, channel=3)
        if i16:
            xi = np.clip(np.round(x * 14000.0), -32768, 32767).astype(np.int16).reshape(-1, 2)
            full = np.array([[32767, -32768], [-32768, 32767], [32767, 32767], [-32768, -32768]], dtype=np.int16)
            at = np.unique(np.concatenate([[0, n - 1, n // 3, n // 3 + 1], np.arange(7, n, 97), np.arange(n // 2, min(n, n // 2 + 8))]))
            at = at[at < n]
            xi[at] = full[np.arange(at.size) % 4]
            xi = xi.reshape(-1)
            _signals[(n, i16)] = (xi, xi.astype(np.float32) * np.float32(2.0 ** -15))
        else:
            _signals[(n, i16)] = (x, x)
        if len(_signals) > 64:
            _signals.pop(next(iter(_signals)))
    return _signals[(n, i16)]


def check(oracle, y, ref, what, tag="interp-matrix"):
    l2, mx = oracle.err_metrics(y, ref)
    print(tag, what, "l2=%.3g max=%.3g" % (l2, mx))
    assert l2 <= TOL and mx <= TOL, (what, l2, mx)
