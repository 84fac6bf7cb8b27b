"""Float64 reference of the arbitrary-ratio resampler's definition (docs/SPEC.md §12), with Python integers for the time tau,
for tests/test_arb_host.py, tests/test_arb_gpu.py and the tools; the plan's tile shape restated; the float32 model of §12's
arithmetic order.

    P = 2^b, K = ceil(T / P);  q = tau >> 32, f = tau mod 2^32, p = f >> (32 - b), mu = (f mod 2^(32 - b)) / 2^(32 - b)
    y = sum_{j<K} [(1 - mu) h[p + j P] + mu h[p + 1 + j P]] x[q - j];  tau += R

A call that brings the inputs [c, c + n) emits every output with tau >> 32 < c + n."""
import numpy as np

from resamp_ref import _fma32, as_c, as_iq, ceil_div

MIN_STEP, MAX_STEP = 1 << 26, 1 << 34
TILE_OUT = 1024


def out_count(c, tau, n, R):
    """outputs of a call with n inputs at position c with the next output at tau (Python integers)"""
    return max(0, ceil_div(((c + n) << 32) - tau, R))


def tile_shape(T, b, R):
    """(K, tile_out, x_len) restated from arb_shape (csrc/if_fir_arb_plan.h): K phase taps, tiles of 1024 consecutive outputs,
    and the window that holds the samples of a tile whatever the fraction of its first output.  tests/test_arb_host.py holds
    it to the header, tests/test_arb_gpu.py to the library."""
    K = ceil_div(T, 1 << b)
    return K, TILE_OUT, (((TILE_OUT - 1) * R + (1 << 32) - 1) >> 32) + K


def stream_len(T, b, R):
    """the shortest stream of the tests: three whole tiles and a ragged one, and never shorter than 2 K + 17 inputs (a stream
    shorter than K - 1 samples would put only the zeros of the start under every phase's highest tap); with more than 384
    phases eight whole tiles, so that a phase row is met by eight outputs or so and not by three (tests/test_arb_host.py:
    on three, zeroing a row's end can cost less than 1e-2 because the samples under it happen to be small)"""
    K, tile_out, _ = tile_shape(T, b, R)
    tiles = 3 if (1 << b) <= 384 else 8
    return max((((tiles * tile_out + 17) * R) >> 32) + 1, 2 * K + 17)


def rows(taps, b, dtype=np.float64):
    """g[p][j] = h[p + j P] for p = 0 .. P (row P is row 0 moved up by one tap), zero where the index reaches T"""
    h = np.asarray(taps, dtype=dtype)
    P = 1 << b
    K = ceil_div(h.size, P)
    g = np.zeros((K + 1) * P, dtype=dtype)
    g[:h.size] = h
    g = g.reshape(K + 1, P).T          # g[p][j] = h[p + j P], j = 0 .. K
    return np.concatenate([g[:, :K], g[:1, 1:]], axis=0)


def places(tau, count, R, b):
    """(q, p, mu as float64: exact, it has at most 28 bits) of `count` outputs from time tau on.  tau < 2^63 - count R."""
    t = np.uint64(tau) + np.arange(count, dtype=np.uint64) * np.uint64(R)
    assert tau + count * R < 1 << 63
    f = t & np.uint64(0xffffffff)
    low = f & np.uint64((1 << (32 - b)) - 1)
    return (t >> np.uint64(32)).astype(np.int64), (f >> np.uint64(32 - b)).astype(np.int64), low.astype(np.float64) / float(1 << (32 - b))


def _schedule(n, R):
    return [(n, R)] if np.isscalar(R) else list(R)


def resample_f64(taps, x_iq, b, R, offset=0):
    """taps: float32; x_iq: interleaved I/Q of a stream from index 0; R: the step, or a list of (inputs, step) pieces that
    covers the stream (a retune between calls); offset: tau at the start (< 2^34).  Returns (interleaved float64 outputs,
    the count of every piece)."""
    g = rows(taps, b)
    K = g.shape[1]
    x = as_c(x_iq)
    xp = np.concatenate([np.zeros(K - 1, dtype=np.complex128), x])
    win = np.lib.stride_tricks.sliding_window_view(xp, K)       # win[q][e] = x[q - (K - 1) + e]
    c, tau = 0, offset
    out, counts = [], []
    for n, step in _schedule(x.size, R):
        m = out_count(c, tau, n, step)
        q, p, mu = places(tau, m, step, b)
        assert m == 0 or q[-1] < c + n <= x.size
        coef = (1.0 - mu)[:, None] * g[p] + mu[:, None] * g[p + 1]   # [output][j]
        out.append(np.einsum("ij,ij->i", coef[:, ::-1], win[q]) if m else np.zeros(0, dtype=np.complex128))
        counts.append(m)
        c, tau = c + n, tau + m * step
        assert c << 32 <= tau < (c << 32) + MAX_STEP
    assert c == x.size
    return as_iq(np.concatenate(out)), counts


def _dot32(g, p, xr, xi, q, K, seg):
    """SPEC §7's order on one phase row per output: taps in descending j (e = K - 1 - j counts up from the oldest sample),
    segments of `seg` from +0 with the highest segment first, fused multiply-adds, compensated adds of the segments"""
    f32 = np.float32
    m = q.size
    acc = [np.zeros(m, f32), np.zeros(m, f32)]
    lost = [np.zeros(m, f32), np.zeros(m, f32)]
    e, length = 0, K - ((K - 1) // seg) * seg
    while e < K:
        sr, si = np.zeros(m, f32), np.zeros(m, f32)
        for ee in range(e, e + length):
            hr = g[p, K - 1 - ee]
            sr, si = _fma32(hr, xr[q + ee], sr), _fma32(hr, xi[q + ee], si)
        for c, s in enumerate((sr, si)):
            t = acc[c] + s
            d = t - acc[c]
            lost[c] = lost[c] + ((acc[c] - (t - d)) + (s - d))
            acc[c] = t
        e, length = e + length, seg
    return acc[0] + lost[0], acc[1] + lost[1]


def resample_f32_order(taps, x_iq, b, R, seg=16, offset=0):
    """float32 model of SPEC §12's arithmetic (order A): A = the dot product over row p, B = over row p + 1, each in §7's order;
    mu rounded once to float32; y = fma(mu, B - A, A).  x_iq: float32 interleaved, a stream from index 0; R and offset as
    resample_f64."""
    f32 = np.float32
    g = rows(taps, b, f32)
    K = g.shape[1]
    x = np.asarray(x_iq, dtype=f32)
    xr = np.concatenate([np.zeros(K - 1, f32), x[0::2]])
    xi = np.concatenate([np.zeros(K - 1, f32), x[1::2]])
    c, tau = 0, offset
    out = []
    for n, step in _schedule(x.size // 2, R):
        m = out_count(c, tau, n, step)
        q, p, mu = places(tau, m, step, b)
        mu = mu.astype(f32)
        ar, ai = _dot32(g, p, xr, xi, q, K, seg)
        br, bi = _dot32(g, p + 1, xr, xi, q, K, seg)
        out.append(np.stack([_fma32(mu, br - ar, ar), _fma32(mu, bi - ai, ai)], axis=1).reshape(-1))
        c, tau = c + n, tau + m * step
    return np.concatenate(out)
