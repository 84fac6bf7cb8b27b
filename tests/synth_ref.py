"""Reference of the polyphase synthesis bank (docs/SPEC.md §14), plain numpy, like tests/pfb_ref.py:

    y[n] = sum_k e^{+j 2 pi k n / M} sum_m h[n - m L] X_k[m],   n = absolute output index,   X_k[m<0] = 0

* definition_f64: §14 defines the bank as the sum of M interpolators with their NCO at k / M, which is the channel combiner's
  definition with centres on the grid: tests/combiner_ref.reference with words[k] = (k << 32) // M.  O(channels) convolutions:
  for the small shapes.
* fold_f64: the fold form in float64 -- one inverse M-point transform per frame, then J = ceil(T / L) taps per output.  Equal to
  the definition to 1e-12 (tests/test_synth_host.py), and cheap enough for M = 4096 with 65536 taps.
* model_c64: the same in float32 / complex64 in the order the SPEC states (j = 0 .. J-1 onto a zero, newest frame first), the
  FORWARD scipy.fft on complex64 read at the mirrored bin.
* transfer_f64: what an analysis bank (tests/pfb_ref.py, prototype h, hop L) followed by this bank (prototype g) does to a stream.
* sample_count: the outputs of a call.

Frames are (frames, bins) complex arrays, element j = channel (first_bin + j) mod M, of a call whose first frame has absolute
index `first`, with zero frames before it; the results are complex arrays of frames * L outputs."""
import numpy as np
import scipy.fft

import combiner_ref
from pfb_ref import SIZES, channels

__all__ = ["SIZES", "channels", "sample_count", "terms", "definition_f64", "fold_f64", "model_c64", "transfer_f64", "iq"]


def sample_count(frames, L):
    return frames * L


def terms(T, L):
    """J = ceil(T / L)"""
    return -(-T // L)


def batch(M):
    """frames a workgroup transforms together"""
    return max(1, 1024 // M)


def lds_route_fits(M, T, L, groups=2):
    """`groups` workgroups of the one-kernel route's ring of ceil((J-1)/B) + 1 batches (8 bytes a point), the twiddles and the
    places fit the 160 KB of a CU's LDS: with two the route can be forced, with four it is the plan's choice"""
    B = batch(M)
    return groups * ((-(-(terms(T, L) - 1) // B) + 1) * B * M * 8 + 10 * M) <= 160 * 1024


def iq(y):
    """complex -> interleaved, for oracle.err_metrics"""
    y = np.asarray(y).reshape(-1)
    return np.stack([y.real, y.imag], axis=1).reshape(-1)


def as_frames(x, bins):
    """interleaved (I, Q) values -> (frames, bins) complex128"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    return (x[:, 0] + 1j * x[:, 1]).reshape(-1, bins)


def definition_f64(h, X, M, L, first_bin=0, bins=None, first=0):
    """the sum of interpolators: channel (first_bin + j) mod M through combiner_ref.reference at phase word k 2^32 / M"""
    X = np.asarray(X, dtype=np.complex128)
    ch = channels(M, first_bin, X.shape[1] if bins is None else bins)
    xs = [iq(X[:, j]) for j in range(ch.size)]
    words = [(int(k) << 32) // M for k in ch]
    y = combiner_ref.reference(h, xs, L, words, first_out=(first * L) % (1 << 32))
    return combiner_ref.as_c(y)


def _fold(h, X, M, L, first_bin, bins, first, dtype):
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    h = np.asarray(h, dtype=dtype).reshape(-1)
    T = h.size
    J = terms(T, L)
    X = np.asarray(X).astype(ctype)
    F = X.shape[0]
    full = np.zeros((F + J - 1, M), dtype=ctype)           # J - 1 zero frames before the call
    full[J - 1:, channels(M, first_bin, X.shape[1] if bins is None else bins)] = X
    fwd = scipy.fft.fft(full, axis=1)
    assert fwd.dtype == ctype
    v = fwd[:, (M - np.arange(M)) % M]                      # v_m[s] = F_m[(M - s) mod M]
    r = np.arange(F * L, dtype=np.int64)
    f, p = r // L, r % L
    s = (((first * L) % M) + r) % M
    hp = np.zeros(J * L, dtype=dtype)
    hp[:T] = h
    acc = np.zeros(F * L, dtype=ctype)
    for j in range(J):                                      # newest frame first
        t = p + j * L
        term = hp[t] * v[f + J - 1 - j, s]
        acc = np.where(t < T, acc + term, acc)
    assert acc.dtype == ctype
    return acc


def fold_f64(h, X, M, L, first_bin=0, bins=None, first=0):
    return _fold(h, X, M, L, first_bin, bins, first, np.float64)


def model_c64(h, X, M, L, first_bin=0, bins=None, first=0):
    return _fold(h, X, M, L, first_bin, bins, first, np.float32)


def transfer_f64(h, g, x, M, L):
    """y[n] = M sum_i x[n - i M] sum_m g[n - m L] h[i M - (n - m L)] for the frames m with 0 <= m L < len(x): what
    pfb_ref.fold_f64(h, x, M, L) followed by fold_f64(g, ., M, L) gives, from a stream that starts at index 0.
    x: complex samples; returns ceil(len(x) / L) L outputs"""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    n = x.size
    F = -(-n // L)
    y = np.zeros(F * L + g.size, dtype=np.complex128)
    u = np.arange(g.size)
    for m in range(F):
        w = np.zeros(g.size, dtype=np.complex128)
        for i in range((h.size + g.size) // M + 2):
            t = i * M - u                                   # the analysis tap
            at = m * L + u - i * M                          # = n - i M
            ok = (t >= 0) & (t < h.size) & (at >= 0) & (at < n)
            w[ok] += h[t[ok]] * x[at[ok]]
        y[m * L:m * L + g.size] += M * g * w
    return y[:F * L]
