"""Reference of the real-output polyphase synthesis bank (docs/SPEC.md §18), plain numpy, like tests/synth_ref.py:

    y[n] = sum_m h[n - m L] ( Re X_0[m] + (-1)^n Re X_H[m] + 2 sum_{0<k<H} Re( X_k[m] e^{+j 2 pi k n / M} ) ),   H = M / 2

* extend: the Hermitian extension of a frame of the span -- channel M - k = conj of channel k, the imaginary parts of channels
  0 and H dropped.
* definition_f64: §18 defines the bank as the real part of §14's bank fed the extended frame: synth_ref.definition_f64 (the
  sum of M interpolators) on extend(X), real part.  O(M) convolutions: for the small shapes.
* full_f64: the same through synth_ref.fold_f64 (one M-point transform per frame), which tests/test_synth_host.py holds to the
  definition at 1e-12: the float64 reference of the larger shapes.
* fold_f64: the half-size form in float64 -- the pre-tangle Z_k = (X_k + conj X_{H-k}) + j W^k (X_k - conj X_{H-k}), one inverse
  H-point transform per frame, z[n] = v[2n] + j v[2n+1], then J = ceil(T / L) taps per output.
* model_f32: the same in float32 / complex64 in the order SPEC §18 states: the pre-tangle with §13's twiddle product and
  W^k from float64 rounded once (k <= H/2; W^{H-k} = (-re, im) of entry k), the FORWARD scipy.fft on complex64 read at the
  mirrored bin, the chain j = 0 .. J-1 onto a zero, newest frame first.  (numpy float32 multiply-adds are not fused: a model of
  the error, not of the bits.)
* to_i16: SPEC §11's int16 rule.

Frames are (frames, bins) complex arrays, element j = channel first_bin + j (0 <= first_bin, first_bin + bins <= M/2 + 1), of a
call whose first frame has absolute index `first`, with zero frames before it; the results are REAL arrays of frames * L
outputs."""
import numpy as np
import scipy.fft

import synth_ref
from duc_ref import to_i16  # noqa: F401  (§18's int16 output is §11's)
from rpfb_ref import SIZES, channels  # noqa: F401  (the sizes and the span of §18 are §17's)
from synth_ref import terms

__all__ = ["SIZES", "channels", "terms", "batch", "extend", "definition_f64", "full_f64", "fold_f64", "model_f32", "to_i16",
           "pretangle_twiddles"]


def batch(M):
    """frames a workgroup transforms together: 1024 points of the M/2-point transform"""
    return max(1, 2048 // M)


def _half(X, M, first_bin, bins, ctype):
    """(frames, H + 1): channels 0 .. H of every frame, +0 outside the span, channels 0 and H real"""
    X = np.asarray(X).astype(ctype)
    H = M // 2
    half = np.zeros((X.shape[0], H + 1), dtype=ctype)
    half[:, channels(M, first_bin, X.shape[1] if bins is None else bins)] = X
    half[:, 0] = half[:, 0].real
    half[:, H] = half[:, H].real
    return half


def extend(X, M, first_bin=0, bins=None):
    """(frames, M) complex128: the Hermitian extension of the frames of a span"""
    H = M // 2
    half = _half(X, M, first_bin, bins, np.complex128)
    full = np.zeros((half.shape[0], M), dtype=np.complex128)
    full[:, :H + 1] = half
    full[:, H + 1:] = np.conj(half[:, H - 1:0:-1])
    return full


def definition_f64(h, X, M, L, first_bin=0, bins=None, first=0):
    return np.ascontiguousarray(synth_ref.definition_f64(h, extend(X, M, first_bin, bins), M, L, 0, M, first).real)


def full_f64(h, X, M, L, first_bin=0, bins=None, first=0):
    return np.ascontiguousarray(synth_ref.fold_f64(h, extend(X, M, first_bin, bins), M, L, 0, M, first).real)


def pretangle_twiddles(M):
    """W^k = e^{+j 2 pi k / M}, k = 0 .. H - 1, as the kernel has them: float64 cos and sin rounded once for k <= H/2, entry
    H - k negated in its real part for k > H/2"""
    H = M // 2
    k = np.arange(H // 2 + 1)
    w = np.exp(2j * np.pi * k / M).astype(np.complex64)
    out = np.empty(H, dtype=np.complex64)
    out[:H // 2 + 1] = w
    up = np.arange(H // 2 + 1, H)
    out[up] = -np.conj(w[H - up])
    return out


def _taps_chain(h, v, L, first, M, dtype):
    """outputs of the frames whose REAL slots are v[J - 1:] (the J - 1 rows before them: the frames before the call)"""
    T = h.size
    J = terms(T, L)
    F = v.shape[0] - (J - 1)
    r = np.arange(F * L, dtype=np.int64)
    f, p = r // L, r % L
    s = (((first * L) % M) + r) % M
    hp = np.zeros(J * L, dtype=dtype)
    hp[:T] = h
    acc = np.zeros(F * L, dtype=dtype)
    for j in range(J):                                      # newest frame first
        t = p + j * L
        acc = np.where(t < T, acc + hp[t] * v[f + J - 1 - j, s], acc)
    assert acc.dtype == dtype
    return acc


def fold_f64(h, X, M, L, first_bin=0, bins=None, first=0):
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    H, J = M // 2, terms(h.size, L)
    half = _half(X, M, first_bin, bins, np.complex128)
    half = np.concatenate([np.zeros((J - 1, H + 1), dtype=np.complex128), half])
    k = np.arange(H)
    A, Bc = half[:, k], np.conj(half[:, H - k])
    Z = (A + Bc) + 1j * np.exp(2j * np.pi * k / M) * (A - Bc)
    z = scipy.fft.ifft(Z, axis=1) * H
    v = np.empty((half.shape[0], M), dtype=np.float64)
    v[:, 0::2] = z.real
    v[:, 1::2] = z.imag
    return _taps_chain(h, v, L, first, M, np.float64)


def model_f32(h, X, M, L, first_bin=0, bins=None, first=0):
    f32 = np.float32
    h = np.asarray(h, dtype=f32).reshape(-1)
    H, J = M // 2, terms(h.size, L)
    half = _half(X, M, first_bin, bins, np.complex64)
    half = np.concatenate([np.zeros((J - 1, H + 1), dtype=np.complex64), half])
    k = np.arange(H)
    A, B = half[:, k], half[:, H - k]
    W = pretangle_twiddles(M)
    er, ei = A.real + B.real, A.imag - B.imag
    dr, di = A.real - B.real, A.imag + B.imag
    pr = dr * W.real - di * W.imag
    pi = dr * W.imag + di * W.real
    Z = np.empty((half.shape[0], H), dtype=np.complex64)
    Z.real = er - pi
    Z.imag = ei + pr
    Z[:, 0] = (half[:, 0].real + half[:, H].real) + 1j * (half[:, 0].real - half[:, H].real)
    assert er.dtype == f32 and pr.dtype == f32
    fwd = scipy.fft.fft(Z, axis=1)
    assert fwd.dtype == np.complex64
    z = fwd[:, (H - np.arange(H)) % H]                      # z[n] = F[(H - n) mod H]
    v = np.empty((half.shape[0], M), dtype=f32)
    v[:, 0::2] = z.real
    v[:, 1::2] = z.imag
    return _taps_chain(h, v, L, first, M, f32)
