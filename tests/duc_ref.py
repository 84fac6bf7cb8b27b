"""Float64 reference of the real-output up-converter's definition (docs/SPEC.md §11), for tests/test_duc_gpu.py and the tools:

    u[m] = x[m/L] if m mod L == 0 else 0,   v[m] = sum_k h[k] u[m-k],   y[m] = Re{ exp(+j 2 pi ((P m) mod 2^32) / 2^32) v[m] }

the interpolation, every OUTPUT mixed, the real part (the definition, not the identity the kernel uses); the kernel's tile
shape restated from csrc/if_fir_duc_plan.h; the float32 model of §11's arithmetic order; and the int16 output rule."""
import numpy as np

from ddc_ref import TWO32, _fma32, as_c, ceil_div, phase_word, taps_c  # noqa: F401  (phase_word, as_c: for the tests)

SEG = 16


def out_count(n, L):
    return n * L


def phase_taps(T, L):
    return ceil_div(T, L)


def tile_shape(T, L):
    """(K, KP, Q) of the kernel's tile, restated from duc_shape: K = ceil(T / L) phase taps, KP = K rounded up to even, Q input
    samples per tile = as many runs of 256 as keep L Q <= 16384, at most 4.  tests/test_duc_host.py holds it to the header,
    tests/test_duc_gpu.py to the library."""
    K = phase_taps(T, L)
    return K, (K + 1) // 2 * 2, 256 * min(16384 // (256 * L), 4)


def stream_len(T, L):
    """INPUT samples: three whole tiles and a ragged one, and never shorter than two phase rows"""
    K, _, Q = tile_shape(T, L)
    return max(3 * Q + 17, 2 * K + 17)


def _phase(word, first, n):
    """(P m) mod 2^32 for m = first .. first + n - 1, exact"""
    m = (np.arange(n, dtype=np.uint64) + np.uint64(first % TWO32)) & np.uint64(TWO32 - 1)
    return (m * np.uint64(word)) & np.uint64(TWO32 - 1)


def interpolate_f64(h, x, L):
    """v[m] for m = 0 .. len(x) L - 1, phase by phase: v[q L + p] = sum_j h[p + j L] x[q - j] (complex128)"""
    n = x.size
    v = np.zeros(n * L, dtype=np.complex128)
    for p in range(min(L, h.size)):
        hp = h[p::L]
        if n * hp.size <= 1 << 26:
            v[p::L] = np.convolve(x, hp)[:n]
        else:
            from scipy.signal import oaconvolve
            v[p::L] = oaconvolve(x, hp)[:n]
    return v


def duc_f64(taps, x_iq, L, word=0, complex_taps=False, first=0):
    """taps: float32 (interleaved (re, im) pairs with complex_taps); x_iq: interleaved I/Q of a stream whose first sample has
    absolute INPUT index `first`, with zeros before it.  Returns the N L real outputs as float64."""
    v = interpolate_f64(taps_c(taps, complex_taps), as_c(x_iq), L)
    if word:
        v = v * np.exp(2j * np.pi * (_phase(word, first * L, v.size).astype(np.float64) / TWO32))
    return np.ascontiguousarray(v.real)


def to_i16(y):
    """SPEC §11's int16 output of a float result: times 2^15, to nearest even, saturated"""
    return np.clip(np.rint(np.asarray(y) * 32768.0), -32768, 32767).astype(np.int16)


def mixed_taps(taps, word, complex_taps=False):
    """g[k] = h[k] e^{+j theta k} in float64, rounded once to float32, as the kernel's table holds it: (g_r, -g_i)"""
    h = taps_c(taps, complex_taps)
    if word:
        k = np.arange(h.size, dtype=np.uint64)
        h = h * np.exp(2j * np.pi * (((k * np.uint64(word)) & np.uint64(TWO32 - 1)).astype(np.float64) / TWO32))
    return h.real.astype(np.float32), -(h.imag.astype(np.float32))


def segments(T, L, p):
    """SPEC §11's accumulation order of phase p as a list of segments, each a list of tap indices k = p + j L in the order of
    their multiply-adds (k >= T: a zero tap of the padding): j = K-1 .. 0, the first segment holding the K - 16 floor((K-1)/16)
    oldest phase taps, the others 16."""
    K = phase_taps(T, L)
    js = list(range(K - 1, -1, -1))
    top = K - ((K - 1) // SEG) * SEG
    cuts = [0] + list(range(top, K + 1, SEG))
    return [[p + j * L for j in js[a:b]] for a, b in zip(cuts[:-1], cuts[1:])]


def rotated_f32(x_iq, L, word, first=0):
    """x'[n] = x[n] e^{+j theta L n} as the kernel forms it, with the phasor of the exact word (P L n) mod 2^32 from float64 cos /
    sin rounded once (the kernel's comes from nco_phasor: the two agree to the tolerance only): float32 (re, im)"""
    f32 = np.float32
    x = np.asarray(x_iq, dtype=f32).reshape(-1, 2)
    xr, xi = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])
    if not word:
        return xr, xi
    ang = 2.0 * np.pi * (_phase((word * L) % TWO32, first, xr.size).astype(np.float64) / TWO32)
    wr, wi = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
    return _fma32(xr, wr, -(xi * wi)), _fma32(xr, wi, xi * wr)


def duc_f32_order(taps, x_iq, L, word=0, complex_taps=False, first=0, drop=None):
    """float32 model of SPEC §11's arithmetic: per output two chains, sum g_r x'_r and sum (-g_i) x'_i, over the segments of
    segments(), each from +0 with one fused multiply-add per tap and chain, joined by the compensated addition with the
    correction added once; then y = a_r + a_i.  x_iq: float32 I/Q.  drop: a tap index treated as zero.  Returns float32."""
    f32 = np.float32
    gr, gi = mixed_taps(taps, word, complex_taps)
    T = gr.size
    if drop is not None:
        gr, gi = gr.copy(), gi.copy()
        gr[drop] = gi[drop] = 0.0
    K = phase_taps(T, L)
    xr, xi = rotated_f32(x_iq, L, word, first)
    n = xr.size
    xr, xi = np.concatenate([np.zeros(K, f32), xr]), np.concatenate([np.zeros(K, f32), xi])
    q = np.arange(n, dtype=np.int64) + K
    y = np.zeros(n * L, f32)
    for p in range(L):
        acc = [np.zeros(n, f32), np.zeros(n, f32)]
        lost = [np.zeros(n, f32), np.zeros(n, f32)]
        for seg in segments(T, L, p):
            s = [np.zeros(n, f32), np.zeros(n, f32)]
            for k in seg:
                if k < T:   # (a zero tap adds +0 x to a sum that is never -0: nothing)
                    at = q - k // L
                    s[0] = _fma32(np.full(n, gr[k]), xr[at], s[0])
                    s[1] = _fma32(np.full(n, gi[k]), xi[at], s[1])
            for c in range(2):
                t = acc[c] + s[c]
                d = t - acc[c]
                lost[c] = lost[c] + ((acc[c] - (t - d)) + (s[c] - d))
                acc[c] = t
        y[p::L] = (acc[0] + lost[0]) + (acc[1] + lost[1])
    return y


def metrics(y, ref):
    """SPEC §3's two metrics on real streams: (l2, max)"""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(y - ref) / np.linalg.norm(ref), np.max(np.abs(y - ref)) / np.max(np.abs(ref))


def signal(oracle, n, i16):
    """(what the library is given, the same samples as float32 I/Q): matrix_util.signal; int16 with full-scale samples"""
    import matrix_util
    return matrix_util.signal(oracle, n, i16)
