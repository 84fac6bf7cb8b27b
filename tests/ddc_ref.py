"""Float64 reference of the real-input down-converter's definition (docs/SPEC.md §10), for tests/test_ddc_gpu.py and the tools:

    x'[a] = r[a] exp(-j 2 pi ((P a) mod 2^32) / 2^32),   y[n] = sum_k h[k] x'[n-k],   y_D[m] = y[m D]

every input sample mixed, the convolution, every D-th kept (the definition, not the identity the kernel uses); the kernel's
tile shape restated from csrc/if_fir_ddc_plan.h; and the float32 model of §10's arithmetic order."""
import numpy as np

TWO32 = 1 << 32


def ceil_div(a, b):
    return -((-a) // b)


def phase_word(freq):
    """P = round(f 2^32) mod 2^32"""
    return int(round(float(freq) * 4294967296.0)) % TWO32


def out_count(c, n, D):
    """outputs of a call with n inputs whose first input has absolute index c: the n in [c, c + n) with n mod D == 0"""
    return ceil_div(c + n, D) - ceil_div(c, D)


def row_taps(T, D):
    return (ceil_div(T, D) + 3) // 4 * 4


def tile_shape(T, D):
    """(K, tile_out, tile_in) of the kernel's tile, restated from ddc_shape: K taps per phase row (a multiple of 4); the row
    stride that fits 16384 floats of LDS over D rows (a multiple of 4 whose quarter is odd) less K columns, at most 1024
    outputs.  tests/test_ddc_host.py holds it to the header, tests/test_ddc_gpu.py to the library."""
    K = row_taps(T, D)
    rs = (16384 // D) // 4 * 4
    if (rs // 4) % 2 == 0:
        rs -= 4
    tile_out = min(rs - K, 1024)
    return K, tile_out, tile_out * D


def stream_len(T, D):
    """three whole tiles and a ragged one, and never shorter than 2 T + 17 samples"""
    _, tile_out, tile_in = tile_shape(T, D)
    return max(3 * tile_in + 17 * D + 5, 2 * T + 17)


def as_iq(c):
    return np.stack([c.real, c.imag], axis=1).reshape(-1)


def as_c(iq):
    iq = np.asarray(iq, dtype=np.float64).reshape(-1, 2)
    return iq[:, 0] + 1j * iq[:, 1]


def taps_c(taps, complex_taps):
    h = np.asarray(taps, dtype=np.float64)
    return h[0::2] + 1j * h[1::2] if complex_taps else h.astype(np.complex128)


def _phase(word, first, n):
    """(P a) mod 2^32 for a = first .. first + n - 1, exact"""
    a = (np.arange(n, dtype=np.uint64) + np.uint64(first % TWO32)) & np.uint64(TWO32 - 1)
    return (a * np.uint64(word)) & np.uint64(TWO32 - 1)


def _convolve(x, h):
    """the first len(x) values of the convolution; long ones by overlap-add (its error, 1e-15 of the peak, is far below 1e-6)"""
    if x.size * h.size <= 1 << 26:
        return np.convolve(x, h)[:x.size]
    from scipy.signal import oaconvolve
    return oaconvolve(x, h)[:x.size]


def ddc_f64(taps, r, D, word=0, complex_taps=False, first=0):
    """taps: float32 (interleaved (re, im) pairs with complex_taps); r: the real samples of a stream whose first sample has
    absolute index `first`, with zeros before it.  Returns the outputs at the absolute n = 0 mod D as interleaved float64."""
    h = taps_c(taps, complex_taps)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    x = r * np.exp(-2j * np.pi * (_phase(word, first, r.size).astype(np.float64) / TWO32)) if word else r.astype(np.complex128)
    y = _convolve(x, h)
    return as_iq(y[(-first) % D::D])


def mixed_taps(taps, word, complex_taps=False):
    """g[k] = h[k] e^{+j theta k} in float64, rounded once to float32: (re, im) as two float32 arrays"""
    h = taps_c(taps, complex_taps)
    if word:
        k = np.arange(h.size, dtype=np.uint64)
        h = h * np.exp(2j * np.pi * (((k * np.uint64(word)) & np.uint64(TWO32 - 1)).astype(np.float64) / TWO32))
    return h.real.astype(np.float32), h.imag.astype(np.float32)


def _fma32(a, b, c):
    """float32 fma, exactly: the product of two float32 is exact in float64; its sum with c is taken in float64 together with
    what that addition lost (two-sum), and where the float64 sum lies exactly half way between two float32 values the lost part
    decides the direction, as the single rounding of a true fma does"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    r = s.astype(np.float32)
    odd = np.flatnonzero((err != 0.0) & (s != r.astype(np.float64)) & np.isfinite(s))
    if odd.size:
        so, ro = s[odd], r[odd]
        other = np.nextafter(ro, np.where(so > ro, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = np.abs(so - ro.astype(np.float64)) == np.abs(other.astype(np.float64) - so)
        away = tie & (np.sign(err[odd]) == np.sign(so - ro.astype(np.float64)))
        r[odd[away]] = other[away]
    return r


def segments(T, D):
    """SPEC §10's accumulation order as a list of segments, each a list of tap indices k in the order of their multiply-adds
    (k >= T: a zero tap of the padding).  Rows R = 0 .. D-1 hold the taps rho = D-1-R, j = K-1 .. 0; K <= 16: floor(16 / K)
    whole rows per segment; K > 16: a row is cut, its first segment holding the K - 16 floor((K-1)/16) oldest taps."""
    K = row_taps(T, D)
    row = lambda R, e0, e1: [(D - 1 - R) + (K - 1 - e) * D for e in range(e0, e1)]
    segs = []
    if K <= 16:
        G = 16 // K
        for r0 in range(0, D, G):
            segs.append([k for R in range(r0, min(r0 + G, D)) for k in row(R, 0, K)])
    else:
        top = K - ((K - 1) // 16) * 16
        for R in range(D):
            e, length = 0, top
            while e < K:
                segs.append(row(R, e, e + length))
                e, length = e + length, 16
    return segs


def ddc_f32_order(taps, r, D, word=0, complex_taps=False, first=0, drop=None):
    """float32 model of SPEC §10's arithmetic: per output the segments of segments(), each from +0 with one fused multiply-add
    per tap and component, joined by the compensated addition, then one rotation by the phasor of the output's absolute
    index (float64 cos / sin, rounded once).  r: float32 real samples.  drop: a tap index treated as zero."""
    f32 = np.float32
    gr, gi = mixed_taps(taps, word, complex_taps)
    T = gr.size
    if drop is not None:
        gr, gi = gr.copy(), gi.copy()
        gr[drop] = gi[drop] = 0.0
    K = row_taps(T, D)
    r = np.asarray(r, dtype=f32).reshape(-1)
    pad = K * D
    xp = np.concatenate([np.zeros(pad, f32), r])
    at = np.arange((-first) % D, r.size, D, dtype=np.int64)     # the outputs' places in r
    acc = [np.zeros(at.size, f32), np.zeros(at.size, f32)]
    lost = [np.zeros(at.size, f32), np.zeros(at.size, f32)]
    for seg in segments(T, D):
        sr, si = np.zeros(at.size, f32), np.zeros(at.size, f32)
        for k in seg:
            if k < T:   # (a zero tap adds +0 x: nothing)
                s = xp[at + pad - k]
                sr, si = _fma32(np.full(at.size, gr[k]), s, sr), _fma32(np.full(at.size, gi[k]), s, si)
        for c, g in enumerate((sr, si)):
            t = acc[c] + g
            d = t - acc[c]
            lost[c] = lost[c] + ((acc[c] - (t - d)) + (g - d))
            acc[c] = t
    vr, vi = acc[0] + lost[0], acc[1] + lost[1]
    if word:
        a = (at.astype(np.uint64) + np.uint64(first % TWO32)) & np.uint64(TWO32 - 1)
        phi = (np.uint64(TWO32) - ((a * np.uint64(word)) & np.uint64(TWO32 - 1))) & np.uint64(TWO32 - 1)
        ang = 2.0 * np.pi * (phi.astype(np.float64) / TWO32)
        wr, wi = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
        vr, vi = _fma32(vr, wr, -(vi * wi)), _fma32(vr, wi, vi * wr)
    return np.stack([vr, vi], axis=1).reshape(-1)


def real_signal(oracle, n, i16):
    """(what the library is given, the same samples as float32): the I, Q values of matrix_util.signal read as n real samples;
    int16 at level 14000 with full-scale samples at the ends, scattered, and in a run"""
    import matrix_util
    raw, x = matrix_util.signal(oracle, (n + 1) // 2, i16)
    return raw[:n], x[:n]
