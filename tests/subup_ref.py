"""Reference of the per-bin interpolating FIR stage over frames (docs/SPEC.md §16), plain numpy, on top of tests/combiner_ref.py
and tests/sub_ref.py as tests/sub_ref.py is on its neighbours:

    u_j[n] = x_j[n / R] if R | n else 0,   v_j[n] = sum_k h_r[k] u_j[n - k],   y_j[n] = exp(+j 2 pi ((P_j n) mod 2^32) / 2^32) v_j[n]
    x_j[m] = in[m B + j],   n = absolute OUTPUT frame index,   out[(n - c R) B + j] = y_j[n]

channel_f64: bin by bin through combiner_ref.reference, the interpolator §16 defines the stage by.  definition_f64: zero-stuff,
convolve, rotate.  phase_f64: the phase form v_j[m R + p] = sum_i h_r[p + i R] x_j[m - i].  reference_upfirdn: scipy, words 0.
model_c64: the float32 model of §16's arithmetic order.  X is always a (frames, bins) complex array whose first frame has absolute
INPUT index `first`, with zeros before it; taps are (rows, T) float32, rows 1 or bins; words are the 32-bit phase words, one per
bin.  Every function returns (frames R, bins)."""
import numpy as np

import combiner_ref
from ddc_ref import _fma32
from sub_ref import TWO32, as_frames, ceil_div, iq, mixed_words, phase_word, rows_of, word_freq  # noqa: F401 (the tests' names)

MAX_J = 32


def frame_count(c, F, R):
    """output frames of a call with F frames at input position c: F R, or 0 where (c + F) R would pass 2^64 - 1"""
    return F * R if (c + F) * R <= (1 << 64) - 1 else 0


def last_start(F, R):
    """the last position at which a call of F frames is accepted"""
    return ((1 << 64) - 1) // R - F


def _rotation(words, first_out, count):
    """exp(+j 2 pi ((P_j n) mod 2^32) / 2^32) for n = first_out .. first_out + count - 1, the phase in integers: (count, bins)"""
    n = (np.arange(count, dtype=np.uint64) + np.uint64(first_out % TWO32)) & np.uint64(TWO32 - 1)
    ph = (n[:, None] * np.asarray(words, dtype=np.uint64)[None, :]) & np.uint64(TWO32 - 1)
    return np.exp(2j * np.pi * (ph.astype(np.float64) / TWO32))


def channel_f64(taps, X, R, words, first=0):
    """THE definition: bin j is combiner_ref.reference(h_r, [x_j], R, [P_j], first_out=first R)"""
    X = np.asarray(X)
    F, B = X.shape
    h = rows_of(taps, B)
    y = np.empty((F * R, B), dtype=np.complex128)
    for j in range(B):
        xj = np.ascontiguousarray(iq(X[:, j]), dtype=np.float32)
        y[:, j] = combiner_ref.as_c(combiner_ref.reference(np.ascontiguousarray(h[j]), [xj], R, [int(words[j])], first_out=first * R))
    return y


def definition_f64(taps, X, R, words, first=0):
    """zero-stuff, convolve, rotate"""
    X = np.asarray(X, dtype=np.complex128)
    F, B = X.shape
    h = rows_of(taps, B).astype(np.float64)
    u = np.zeros((F * R, B), dtype=np.complex128)
    u[::R] = X
    v = np.empty_like(u)
    for j in range(B):
        v[:, j] = np.convolve(u[:, j], h[j])[:F * R]
    return v * _rotation(words, first * R, F * R)


def phase_f64(taps, X, R, words, first=0):
    """the phase form: v_j[m R + p] = sum_{i < J, p + i R < T} h_r[p + i R] x_j[m - i]"""
    X = np.asarray(X, dtype=np.complex128)
    F, B = X.shape
    h = rows_of(taps, B).astype(np.float64)
    T = h.shape[1]
    J = ceil_div(T, R)
    hp = np.zeros((B, J * R))
    hp[:, :T] = h
    hp = hp.reshape(B, J, R)
    xp = np.concatenate([np.zeros((J - 1, B), dtype=np.complex128), X])
    v = np.zeros((F, R, B), dtype=np.complex128)
    for i in range(J):
        v += hp[:, i, :].T[None, :, :] * xp[J - 1 - i:J - 1 - i + F][:, None, :]
    return v.reshape(F * R, B) * _rotation(words, first * R, F * R)


def reference_upfirdn(taps, X, R):
    """the third-party form (scipy.signal.upfirdn through combiner_ref.reference_upfirdn), words all 0, position 0"""
    X = np.asarray(X)
    F, B = X.shape
    h = rows_of(taps, B)
    y = np.empty((F * R, B), dtype=np.complex128)
    for j in range(B):
        xj = np.ascontiguousarray(iq(X[:, j]), dtype=np.float32)
        y[:, j] = combiner_ref.as_c(combiner_ref.reference_upfirdn(np.ascontiguousarray(h[j]), [xj], R, [0]))
    return y


def model_c64(taps, X, R, words, first=0):
    """float32 model of SPEC §16's arithmetic: the tap rows padded with zeros to J R taps; per output (m R + p, j) and component
    one chain from +0 over i = J - 1 .. 0 (oldest frame first) of fma(h_r[p + i R], x_j[m - i], acc); then one rotation by the
    phasor of the output's absolute index (float64 cos / sin, rounded once) as (fma(vr, wr, -(vi wi)), fma(vr, wi, vi wr)),
    skipped where the word is 0.  It depends on (T, R) alone.  (The kernel pads further, to its window's bucket: those terms
    come first in the chain, where fma(0, x, +0) = +0 for every finite x.)  X: complex64 values.  Returns (F R, bins) complex64."""
    f32 = np.float32
    X = np.asarray(X, dtype=np.complex64)
    F, B = X.shape
    h = rows_of(taps, B)
    T = h.shape[1]
    J = ceil_div(T, R)
    hp = np.zeros((B, J * R), f32)
    hp[:, :T] = h
    hp = hp.reshape(B, J, R)
    xr = np.concatenate([np.zeros((J - 1, B), f32), X.real.astype(f32)])
    xi = np.concatenate([np.zeros((J - 1, B), f32), X.imag.astype(f32)])
    n = F * R * B
    vr, vi = np.zeros(n, f32), np.zeros(n, f32)
    for i in range(J - 1, -1, -1):
        tap = np.broadcast_to(hp[:, i, :].T[None, :, :], (F, R, B)).reshape(-1)
        a = np.broadcast_to(xr[J - 1 - i:J - 1 - i + F][:, None, :], (F, R, B)).reshape(-1)
        b = np.broadcast_to(xi[J - 1 - i:J - 1 - i + F][:, None, :], (F, R, B)).reshape(-1)
        vr = _fma32(tap, a, vr)
        vi = _fma32(tap, b, vi)
    w = np.asarray(words, dtype=np.uint64)
    if np.any(w != 0):
        rot = _rotation(words, first * R, F * R).reshape(-1)
        wr, wi = rot.real.astype(f32), rot.imag.astype(f32)
        rr, ri = _fma32(vr, wr, -(vi * wi)), _fma32(vr, wi, vi * wr)
        on = np.tile(w != 0, F * R)
        vr, vi = np.where(on, rr, vr), np.where(on, ri, vi)
    y = np.empty(n, dtype=np.complex64)
    y.real, y.imag = vr, vi
    return y.reshape(F * R, B)
