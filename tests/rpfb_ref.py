"""Reference of the real-input polyphase filter bank (docs/SPEC.md §17), plain numpy, like tests/pfb_ref.py:

    y_k[m] = sum_{t<T} h[t] r[a-t] e^{-j 2 pi k (a-t) / M},   a = m D (absolute index),   r[i<0] = 0,   k = 0 .. M/2

* definition_f64: the restatement by the definition -- every product h[t] r[a-t] meets its own phase.  O(bins T) per frame: for
  the small shapes.
* channel_f64: one channel through the project's oracle (oracle.fir_nco_f64 at phase word k 2^32 / M on the stream widened to
  (r, 0)), which is what §17 defines the bank to be.
* fold_f64: the fold form in float64 -- slot (a-t) mod M collects h[t] r[a-t], one M-point real-input transform per frame.
* model_c64: the kernel's arithmetic restated in float32 / complex64 -- the fold in SPEC §13's order (rows r = 0 .. K-1 onto a
  zero), z[n] = u[2n] + j u[2n+1], scipy.fft on complex64 with M/2 points, then the untangling pass in SPEC §17's order with
  W_M^k from float64, rounded once.  (numpy float32 multiply-adds are not fused: a model of the error, not of the bits.)
* frame_count: the frames of a call.

Streams are float32 REAL samples of a call whose first sample has absolute index `first`, with zeros before it; the results
are (frames, bins) complex arrays, bin j = channel first_bin + j."""
import numpy as np
import scipy.fft

from pfb_ref import first_offset, frame_count, iq  # noqa: F401  (the calls of §17 are §13's)

SIZES = (128, 256, 512, 1024, 2048, 4096, 8192)


def channels(M, first_bin=0, bins=None):
    bins = M // 2 + 1 - first_bin if bins is None else bins
    assert 0 <= first_bin and bins >= 1 and first_bin + bins <= M // 2 + 1
    return first_bin + np.arange(bins)


def widen(r):
    """the real stream as interleaved (r, 0): what the complex bank and the oracle take"""
    r = np.asarray(r).reshape(-1)
    out = np.zeros(2 * r.size, dtype=r.dtype)
    out[0::2] = r
    return out


def _slots(h, r, M, D, first, dtype):
    """(frames, M) folded slots u[s] by absolute index: rows r = 0 .. K-1 summed in that order onto a zero"""
    h = np.asarray(h, dtype=dtype).reshape(-1)
    T = h.size
    K = -(-T // M)
    r = np.asarray(r, dtype=dtype).reshape(-1)
    F = frame_count(first, r.size, D)
    a_rel = first_offset(first, D) + D * np.arange(F, dtype=np.int64)
    hp = np.zeros(K * M, dtype=dtype)
    hp[:T] = h
    rp = np.concatenate([np.zeros(K * M - 1, dtype=dtype), r])
    win = np.lib.stride_tricks.sliding_window_view(rp, K * M)[a_rel] if F else np.zeros((0, K * M), dtype=dtype)
    v = (win * hp[::-1]).reshape(F, K, M)       # block K-1-r of the window holds the row r: t = M-1-q + r M
    w = np.zeros((F, M), dtype=dtype)
    for row in range(K):
        w = w + v[:, K - 1 - row, :]
    q = np.arange(M)
    u = np.empty_like(w)
    for f in range(F):
        u[f, ((first + int(a_rel[f])) % M + 1 + q) % M] = w[f]
    assert u.dtype == dtype
    return u


def fold_f64(h, r, M, D, first_bin=0, bins=None, first=0):
    u = _slots(h, r, M, D, first, np.float64)
    return np.ascontiguousarray(scipy.fft.rfft(u, axis=1)[:, channels(M, first_bin, bins)])


def untangle_twiddles(M):
    k = np.arange(M // 2 + 1)
    return np.exp(-2j * np.pi * k / M).astype(np.complex64)


def model_c64(h, r, M, D, first_bin=0, bins=None, first=0):
    f32 = np.float32
    H = M // 2
    u = _slots(h, r, M, D, first, f32)
    z = (u[:, 0::2] + 1j * u[:, 1::2]).astype(np.complex64)
    Z = scipy.fft.fft(z, axis=1)
    assert Z.dtype == np.complex64
    k = np.arange(H + 1)
    A, Bp = Z[:, k % H], Z[:, (H - k) % H]
    W = untangle_twiddles(M)
    er, ei = f32(0.5) * (A.real + Bp.real), f32(0.5) * (A.imag - Bp.imag)
    orr, oi = f32(0.5) * (A.imag + Bp.imag), f32(-0.5) * (A.real - Bp.real)
    pr = orr * W.real - oi * W.imag
    pi = orr * W.imag + oi * W.real
    y = np.empty((Z.shape[0], H + 1), dtype=np.complex64)
    y.real = er + pr
    y.imag = ei + pi
    # channels 0 and M/2 from Re Z[0] +- Im Z[0]
    y[:, 0] = Z[:, 0].real + Z[:, 0].imag
    y[:, H] = Z[:, 0].real - Z[:, 0].imag
    assert y.real.dtype == f32
    return np.ascontiguousarray(y[:, channels(M, first_bin, bins)])


def definition_f64(h, r, M, D, first_bin=0, bins=None, first=0):
    """mix, filter, pick -- nothing of the fold: every product h[t] r[a-t] meets its own phase e^{-j 2 pi k (a-t) / M}"""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    T = h.size
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    ch = channels(M, first_bin, bins)
    F = frame_count(first, r.size, D)
    out = np.zeros((F, ch.size), dtype=np.complex128)
    rp = np.concatenate([np.zeros(T - 1), r])
    t = np.arange(T)
    for f in range(F):
        a_rel = first_offset(first, D) + f * D
        a = first + a_rel
        seg = rp[a_rel:a_rel + T][::-1]        # r[a - t], t = 0 .. T-1
        idx = np.array([(a - int(tt)) % M for tt in t], dtype=np.int64)
        phase = np.exp(-2j * np.pi * ((ch[:, None] * idx[None, :]) % M) / M)
        out[f] = phase @ (h * seg)
    return out


def channel_f64(oracle, h, r, M, D, k, first=0):
    """channel k of every frame through the project's float64 oracle on the widened stream"""
    y = oracle.fir_nco_f64(np.asarray(h, dtype=np.float32), widen(np.asarray(r, dtype=np.float32)), D, (int(k) % M) * ((1 << 32) // M),
                           consumed=first)
    return y[0::2] + 1j * y[1::2]
