"""Reference of the polyphase filter bank (docs/SPEC.md §13), plain numpy, like tests/ddc_ref.py:

    y_k[m] = sum_{t<T} h[t] x[a-t] e^{-j 2 pi k (a-t) / M},   a = m D (absolute index),   x[i<0] = 0

* definition_f64: the restatement by the definition -- mix every sample by its channel's phase, filter, pick a = m D.  O(bins T)
  per frame: for the small shapes.
* channel_f64: one channel through the project's oracle (oracle.fir_nco_f64 at phase word k 2^32 / M), which is what §13 defines
  the bank to be.
* fold_f64: the fold form in float64 -- slot (a-t) mod M collects h[t] x[a-t], one M-point transform per frame.  Equal to the two
  above to 1e-12 (tests/test_pfb_host.py), and cheap enough for M = 4096 with 65536 taps.
* model_c64: the same in float32 / complex64 in the order the SPEC states (rows r = 0 .. K-1 onto a zero), scipy.fft on complex64.
* frame_count: the frames of a call.

Streams are interleaved float32 (I, Q) of a call whose first sample has absolute index `first`, with zeros before it; the
results are (frames, bins) complex arrays, bin j = channel (first_bin + j) mod M."""
import numpy as np
import scipy.fft

SIZES = (64, 128, 256, 512, 1024, 2048, 4096)


def frame_count(c, n, D):
    """frames m with c <= m D < c + n (Python integers: any position)"""
    return -(-(c + n) // D) - -(-c // D)


def first_offset(c, D):
    """offset in the call of the sample under its first frame"""
    return (-c) % D


def channels(M, first_bin, bins):
    return (first_bin + np.arange(bins)) % M


def _c(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    return x[:, 0] + 1j * x[:, 1]


def _windows(h, x, M, D, first, dtype):
    """(frames, K M) products h[t] x[a-t] laid out oldest sample first, and each frame's a mod M"""
    h = np.asarray(h, dtype=dtype).reshape(-1)
    T = h.size
    K = -(-T // M)
    xc = _c(x).astype(np.complex64 if dtype == np.float32 else np.complex128)
    n = xc.size
    F = frame_count(first, n, D)
    a_rel = first_offset(first, D) + D * np.arange(F, dtype=np.int64)
    hp = np.zeros(K * M, dtype=dtype)
    hp[:T] = h
    xp = np.concatenate([np.zeros(K * M - 1, dtype=xc.dtype), xc])
    # window of frame f: call samples a_rel - (K M - 1) .. a_rel
    win = np.lib.stride_tricks.sliding_window_view(xp, K * M)[a_rel] if F else np.zeros((0, K * M), dtype=xc.dtype)
    amod = np.array([(first + int(a)) % M for a in a_rel], dtype=np.int64)
    return win * hp[::-1], amod, K


def _fold(h, x, M, D, first_bin, bins, first, dtype):
    v, amod, K = _windows(h, x, M, D, first, dtype)
    F = v.shape[0]
    v = v.reshape(F, K, M)
    w = np.zeros((F, M), dtype=v.dtype)
    for r in range(K):          # row r holds t = M-1-q + r M: the block K-1-r of the window
        w = w + v[:, K - 1 - r, :]
    # slot (a + 1 + q) mod M
    q = np.arange(M)
    u = np.empty_like(w)
    for f in range(F):
        u[f, (amod[f] + 1 + q) % M] = w[f]
    y = scipy.fft.fft(u, axis=1)
    assert y.dtype == u.dtype
    return np.ascontiguousarray(y[:, channels(M, first_bin, M if bins is None else bins)])


def fold_f64(h, x, M, D, first_bin=0, bins=None, first=0):
    return _fold(h, x, M, D, first_bin, bins, first, np.float64)


def model_c64(h, x, M, D, first_bin=0, bins=None, first=0):
    return _fold(h, x, M, D, first_bin, bins, first, np.float32)


def definition_f64(h, x, M, D, first_bin=0, bins=None, first=0):
    """mix, filter, pick -- nothing of the fold: every product h[t] x[a-t] meets its own phase e^{-j 2 pi k (a-t) / M}"""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    T = h.size
    xc = _c(x)
    n = xc.size
    ch = channels(M, first_bin, M if bins is None else bins)
    F = frame_count(first, n, D)
    out = np.zeros((F, ch.size), dtype=np.complex128)
    xp = np.concatenate([np.zeros(T - 1, dtype=np.complex128), xc])
    t = np.arange(T)
    for f in range(F):
        a_rel = first_offset(first, D) + f * D
        a = first + a_rel
        seg = xp[a_rel:a_rel + T][::-1]        # x[a - t], t = 0 .. T-1
        idx = np.array([(a - int(tt)) % M for tt in t], dtype=np.int64) if a >= 1 << 62 else (a - t) % M
        phase = np.exp(-2j * np.pi * ((ch[:, None] * idx[None, :]) % M) / M)
        out[f] = phase @ (h * seg)
    return out


def channel_f64(oracle, h, x, M, D, k, first=0):
    """channel k of every frame through the project's float64 oracle"""
    y = oracle.fir_nco_f64(np.asarray(h, dtype=np.float32), x, D, (int(k) % M) * ((1 << 32) // M), consumed=first)
    return y[0::2] + 1j * y[1::2]


def iq(y):
    """(frames, bins) complex -> interleaved, for oracle.err_metrics"""
    y = np.asarray(y).reshape(-1)
    return np.stack([y.real, y.imag], axis=1).reshape(-1)
