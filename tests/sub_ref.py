"""Reference of the per-channel FIR stage over filter-bank frames (docs/SPEC.md §15), plain numpy, like tests/ddc_ref.py:

    x'_j[a] = x_j[a] exp(-j 2 pi ((P_j a) mod 2^32) / 2^32),   y_j[n] = sum_k h_r[k] x'_j[n R - k],   x_j[a] = in[a B + j]

definition_f64: every frame mixed, the convolution per bin, every R-th kept.  channel_f64: bin by bin through
oracle.fir_nco_f64, the decimator §15 defines the stage by.  model_c64: the float32 model of §15's arithmetic order.  X is always
a (frames, bins) complex array whose first frame has absolute index `first`, with zeros before it; taps are (rows, T) float32,
rows 1 or bins; words are the 32-bit phase words, one per bin."""
import numpy as np

from ddc_ref import _fma32

TWO32 = 1 << 32
SEG = 16


def ceil_div(a, b):
    return -((-a) // b)


def phase_word(freq):
    """P = round(f 2^32) mod 2^32"""
    return int(round(float(freq) * 4294967296.0)) % TWO32


def word_freq(word):
    """the quantised frequency a word stands for, in [-0.5, 0.5)"""
    return (word - TWO32 if word >= TWO32 // 2 else word) / 4294967296.0


def frame_count(c, F, R):
    """output frames of a call with F frames whose first frame has absolute index c: the a in [c, c + F) with a mod R == 0"""
    return ceil_div(c + F, R) - ceil_div(c, R)


def as_frames(iq, bins):
    """(frames, bins) complex128 of interleaved (re, im) values"""
    v = np.asarray(iq, dtype=np.float64).reshape(-1, 2)
    return (v[:, 0] + 1j * v[:, 1]).reshape(-1, bins)


def iq(frames):
    f = np.asarray(frames).reshape(-1)
    return np.stack([f.real, f.imag], axis=1).reshape(-1)


def rows_of(taps, bins):
    """(bins, T) float32 rows of a (T,), (1, T) or (bins, T) tap array"""
    h = np.asarray(taps, dtype=np.float32)
    h = h.reshape(1, -1) if h.ndim == 1 else h
    assert h.shape[0] in (1, bins)
    return np.broadcast_to(h, (bins, h.shape[1]))


def mixed_words(bins, seed=0):
    """the words of the tests: bin 0 at 0, then one at +0.5, one at -0.5 (the same word), one at 2^-32, the rest seeded"""
    rng = np.random.default_rng([bins, seed, 15])
    f = rng.uniform(-0.5, 0.5, bins)
    for j, v in enumerate((0.0, 0.5, -0.5, 2.0 ** -32)):
        if j < bins:
            f[j] = v
    return f


def _phase(words, first, F):
    """(P_j a) mod 2^32 for a = first .. first + F - 1, exact: (F, bins) uint64"""
    a = (np.arange(F, dtype=np.uint64) + np.uint64(first % TWO32)) & np.uint64(TWO32 - 1)
    return (a[:, None] * np.asarray(words, dtype=np.uint64)[None, :]) & np.uint64(TWO32 - 1)


def definition_f64(taps, X, R, words, first=0):
    X = np.asarray(X, dtype=np.complex128)
    F, B = X.shape
    h = rows_of(taps, B).astype(np.float64)
    xm = X * np.exp(-2j * np.pi * (_phase(words, first, F).astype(np.float64) / TWO32))
    y = np.empty((F, B), dtype=np.complex128)
    for j in range(B):
        y[:, j] = np.convolve(xm[:, j], h[j])[:F]
    return y[(-first) % R::R]


def channel_f64(oracle, taps, X, R, words, first=0):
    """bin by bin through oracle.fir_nco_f64(..., consumed=first); X must hold float32 values.  The oracle reads its position
    as a signed 64-bit integer (a negative one is "before the stream"); the definition depends on the position only through
    first mod R and first mod 2^32, so a position from 2^63 on is handed over as first mod (R 2^32) -- tests/test_sub_host.py
    holds that to definition_f64, which computes with Python's integers"""
    X = np.asarray(X)
    F, B = X.shape
    if first >= 1 << 63:
        first %= R << 32
    h = rows_of(taps, B)
    y = np.empty((frame_count(first, F, R), B), dtype=np.complex128)
    for j in range(B):
        xj = np.ascontiguousarray(iq(X[:, j]), dtype=np.float32)
        v = np.asarray(oracle.fir_nco_f64(np.ascontiguousarray(h[j]), xj, R, int(words[j]), consumed=first), dtype=np.float64).reshape(-1, 2)
        y[:, j] = v[:, 0] + 1j * v[:, 1]
    return y


def mixed_taps(taps, bins, words):
    """g_j[k] = h_r[k] e^{+j theta_j k} in float64, rounded once to float32; a word of 0 gives g = h: ((bins, T) re, the same im)"""
    h = rows_of(taps, bins).astype(np.float64)
    T = h.shape[1]
    w = np.asarray(words, dtype=np.uint64)
    ph = (np.arange(T, dtype=np.uint64)[None, :] * w[:, None]) & np.uint64(TWO32 - 1)
    ang = 2.0 * np.pi * (ph.astype(np.float64) / TWO32)
    on = (w != 0)[:, None]
    return np.where(on, h * np.cos(ang), h).astype(np.float32), np.where(on, h * np.sin(ang), 0.0).astype(np.float32)


def segments(T):
    """SPEC §15's order as a list of segments of tap indices: descending k, the highest segment takes what 16 does not divide"""
    top = T - ((T - 1) // SEG) * SEG
    segs, k = [], T - 1
    length = top
    while k >= 0:
        segs.append(list(range(k, k - length, -1)))
        k -= length
        length = SEG
    return segs


def model_c64(taps, X, R, words, first=0):
    """float32 model of SPEC §15's arithmetic: per output the segments of segments(), each from +0 with
    re = fma(-xi, gi, fma(xr, gr, re)), im = fma(xi, gr, fma(xr, gi, im)) per tap, joined by the compensated addition, its
    correction added once; then one rotation by the phasor of the output's absolute frame index (float64 cos / sin, rounded
    once), skipped where the word is 0.  X: complex64 values.  Returns (frames out, bins) complex64."""
    f32 = np.float32
    X = np.asarray(X, dtype=np.complex64)
    F, B = X.shape
    gr, gi = mixed_taps(taps, B, words)
    T = gr.shape[1]
    xr = np.concatenate([np.zeros((T - 1, B), f32), X.real.astype(f32)])
    xi = np.concatenate([np.zeros((T - 1, B), f32), X.imag.astype(f32)])
    at = np.arange((-first) % R, F, R, dtype=np.int64)   # the outputs' places in X
    n = at.size * B
    acc = [np.zeros(n, f32), np.zeros(n, f32)]
    lost = [np.zeros(n, f32), np.zeros(n, f32)]
    for seg in segments(T):
        sr, si = np.zeros(n, f32), np.zeros(n, f32)
        for k in seg:
            a, b = xr[at + T - 1 - k].reshape(-1), xi[at + T - 1 - k].reshape(-1)
            cr, ci = np.tile(gr[:, k], at.size), np.tile(gi[:, k], at.size)
            sr = _fma32(-b, ci, _fma32(a, cr, sr))
            si = _fma32(b, cr, _fma32(a, ci, si))
        for c, g in enumerate((sr, si)):
            t = acc[c] + g
            d = t - acc[c]
            lost[c] = lost[c] + ((acc[c] - (t - d)) + (g - d))
            acc[c] = t
    vr, vi = acc[0] + lost[0], acc[1] + lost[1]
    w = np.asarray(words, dtype=np.uint64)
    if np.any(w != 0):
        a = (at.astype(np.uint64) + np.uint64(first % TWO32)) & np.uint64(TWO32 - 1)
        phi = (np.uint64(TWO32) - ((a[:, None] * w[None, :]) & np.uint64(TWO32 - 1))) & np.uint64(TWO32 - 1)
        ang = 2.0 * np.pi * (phi.astype(np.float64) / TWO32).reshape(-1)
        wr, wi = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
        rr, ri = _fma32(vr, wr, -(vi * wi)), _fma32(vr, wi, vi * wr)
        on = np.tile(w != 0, at.size)
        vr, vi = np.where(on, rr, vr), np.where(on, ri, vi)
    y = np.empty(n, dtype=np.complex64)
    y.real, y.imag = vr, vi
    return y.reshape(at.size, B)
