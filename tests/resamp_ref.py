"""Float64 reference of the rational resampler's definition (docs/SPEC.md §7), for tests/test_resamp_gpu.py and the tools:

    u[n] = x[n/L] if n mod L == 0 else 0,   v[n] = sum_k h[k] u[n-k],   y[m] = v[m M]

evaluated in its polyphase form m M = q L + p, y[m] = sum_j h[p + j L] x[q - j], one numpy.convolve per phase.  Not a bare
scipy.signal.upfirdn call: that one returns fewer than ceil(N L / M) outputs when T < L."""
import numpy as np


def ceil_div(a, b):
    return -((-a) // b)


def out_count(c, n, L, M):
    """outputs of a call with n inputs whose first input has absolute index c"""
    return ceil_div((c + n) * L, M) - ceil_div(c * L, M)


def tile_shape(T, L, M):
    """(K, tile_out, tile_in) of the kernel's tile, restated from resamp_shape (csrc/if_fir_resamp_plan.h): K phase taps; the
    largest multiple of L within 256 lanes, 4 outputs per lane, capped to the periods whose inputs and K - 1 samples of overlap
    fit 8192 LDS samples.  tests/test_resamp_host.py holds it to the header, tests/test_resamp_gpu.py to the library."""
    K = ceil_div(T, L)
    B = min((256 // L) * 4, (8192 - (K - 1)) // M)
    return K, B * L, B * M


def stream_len(T, L, M):
    """the shortest stream of the loud-row-end tests: three whole tiles and a ragged part, and never shorter than two phase
    rows: a stream shorter than K - 1 samples (64/1 with 4096 taps: 49 samples against K = 64) would put only the zeros of
    the start under every phase's highest tap"""
    K, tile_out, _ = tile_shape(T, L, M)
    return max(((3 * tile_out + 17) * M) // L + 1, 2 * K + 17)


def as_c(iq):
    iq = np.asarray(iq, dtype=np.float64).reshape(-1, 2)
    return iq[:, 0] + 1j * iq[:, 1]


def as_iq(c):
    return np.stack([c.real, c.imag], axis=1).reshape(-1)


def resample_f64(taps, x_iq, L, M, complex_taps=False):
    """taps: float32 (interleaved (re, im) pairs with complex_taps); x_iq: interleaved I/Q of a stream from index 0.
    Returns the ceil(N L / M) outputs as interleaved float64."""
    h = np.asarray(taps, dtype=np.float64)
    if complex_taps:
        h = h[0::2] + 1j * h[1::2]
    x = as_c(x_iq)
    n = x.size
    m = np.arange(ceil_div(n * L, M), dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    y = np.zeros(m.size, dtype=np.complex128)
    for phase in range(L):
        g = h[phase::L]
        sel = p == phase
        if g.size and np.any(sel):
            y[sel] = np.convolve(x, g)[q[sel]]
    return as_iq(y)


def _fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum is rounded to float64, then to float32 (the double
    rounding differs from a true fma only on rare ties)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def resample_f32_order(taps, x_iq, L, M, complex_taps=False, seg=16, compensated=True):
    """float32 model of SPEC §7's arithmetic: phase taps in descending j in segments of `seg` from +0, fused multiply-adds, the
    segments added as they complete with the compensated addition.  x_iq: float32 interleaved, a stream from index 0.
    seg=32, compensated=False is SPEC §3's order (plain adds of 32-tap segments), which §7 compares against."""
    f32 = np.float32
    h = np.asarray(taps, dtype=f32)
    w = 2 if complex_taps else 1
    T = h.size // w
    K = ceil_div(T, L)
    x = np.asarray(x_iq, dtype=f32)
    n = x.size // 2
    xr = np.concatenate([np.zeros(K - 1, f32), x[0::2]])
    xi = np.concatenate([np.zeros(K - 1, f32), x[1::2]])
    m = np.arange(ceil_div(n * L, M), dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    gr, gi = np.zeros((L, K), f32), np.zeros((L, K), f32)
    k = np.arange(T)
    gr[k % L, k // L] = h[0::w]
    if complex_taps:
        gi[k % L, k // L] = h[1::2]
    acc = [np.zeros(m.size, f32), np.zeros(m.size, f32)]
    lost = [np.zeros(m.size, f32), np.zeros(m.size, f32)]
    e, length = 0, K - ((K - 1) // seg) * seg
    while e < K:
        sr, si = np.zeros(m.size, f32), np.zeros(m.size, f32)
        for ee in range(e, e + length):
            a, b, hr, hi = xr[q + ee], xi[q + ee], gr[p, K - 1 - ee], gi[p, K - 1 - ee]
            if complex_taps:
                sr, si = _fma32(-b, hi, _fma32(a, hr, sr)), _fma32(b, hr, _fma32(a, hi, si))
            else:
                sr, si = _fma32(hr, a, sr), _fma32(hr, b, si)
        for c, g in enumerate((sr, si)):
            t = acc[c] + g
            if compensated:
                d = t - acc[c]
                lost[c] = lost[c] + ((acc[c] - (t - d)) + (g - d))
            acc[c] = t
        e, length = e + length, seg
    return np.stack([acc[0] + lost[0], acc[1] + lost[1]], axis=1).reshape(-1)
