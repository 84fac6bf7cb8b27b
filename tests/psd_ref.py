"""docs/SPEC.md §8 restated in numpy, written from the spec text: the streaming power-spectrum estimator's segments, window,
power, bin selection, code mapping and streaming counts in float64 (the reference of tests/test_psd_gpu.py), and a plain
complex64 / float32 implementation in the §8 summation order (scipy.fft), whose error against the float64 reference sets the
tolerance of the GPU test."""
import numpy as np

CHUNK = 8
ZERO_DB, FULL_DB = -3.35, 16.7           # the detector's fft_zero_scale_power, fft_full_scale_power
SLOPE = (FULL_DB - ZERO_DB) / 65535      # dB per code


def as_c(iq):
    """interleaved (I, Q) -> complex128"""
    iq = np.asarray(iq, dtype=np.float64).reshape(-1, 2)
    return iq[:, 0] + 1j * iq[:, 1]


def hann(N):
    """the default window: periodic Hann in float64, rounded once to float32"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


def segments_complete(total, N, H):
    """segments [s H, s H + N) that lie wholly inside the first `total` samples"""
    return 0 if total < N else (total - N) // H + 1


def frame_count(pos, n, N, H, K):
    """frames a call of n samples at stream position pos emits: those whose last segment it completes"""
    return segments_complete(pos + n, N, H) // K - segments_complete(pos, N, H) // K


def bin_indices(N, first_bin, bins):
    assert -N // 2 <= first_bin and first_bin + bins <= N // 2 and bins >= 1
    return (first_bin + np.arange(bins)) % N


def _segments(x, N, H, count):
    return np.lib.stride_tricks.sliding_window_view(x, N)[::H][:count]


def power_f64(iq, N, H, K, window=None, first_bin=None, bins=None):
    """(frames, bins) float64 P of every whole frame of the stream iq (interleaved float32 I, Q)"""
    w = (hann(N) if window is None else np.asarray(window, dtype=np.float32)).astype(np.float64)
    x = as_c(iq)
    frames = segments_complete(x.size, N, H) // K
    sel = bin_indices(N, -N // 2 if first_bin is None else first_bin, N if bins is None else bins)
    out = np.zeros((frames, sel.size))
    if frames:
        seg = _segments(x, N, H, frames * K)
        for f in range(frames):
            S = np.abs(np.fft.fft(seg[f * K:(f + 1) * K] * w, axis=1)[:, sel]) ** 2
            out[f] = S.sum(axis=0) / (K * np.sum(w * w))
    return out


def power_c64(iq, N, H, K, window=None, first_bin=None, bins=None):
    """the same frames from a plain single-precision implementation: complex64 transform (scipy.fft), float32 sums in the §8
    order (segments of a chunk in order, chunk sums in order onto the accumulator, one float32 scale at the end)"""
    import scipy.fft
    w = hann(N) if window is None else np.asarray(window, dtype=np.float32)
    iq = np.asarray(iq, dtype=np.float32).reshape(-1, 2)
    x = (iq[:, 0] + 1j * iq[:, 1]).astype(np.complex64)
    frames = segments_complete(x.size, N, H) // K
    sel = bin_indices(N, -N // 2 if first_bin is None else first_bin, N if bins is None else bins)
    scale = np.float32(1.0 / (K * np.sum(w.astype(np.float64) ** 2)))
    out = np.zeros((frames, sel.size), dtype=np.float32)
    if frames:
        seg = _segments(x, N, H, frames * K)
        for f in range(frames):
            X = scipy.fft.fft((seg[f * K:(f + 1) * K] * w).astype(np.complex64), axis=1)[:, sel]
            assert X.dtype == np.complex64
            S = (X.real * X.real + X.imag * X.imag).astype(np.float32)
            acc = np.zeros(sel.size, dtype=np.float32)
            for c in range(0, K, CHUNK):
                part = np.zeros(sel.size, dtype=np.float32)
                for s in range(c, min(c + CHUNK, K)):
                    part = part + S[s]
                acc = acc + part
            out[f] = acc * scale
    return out


def db_of(power, ref_power):
    """power -> dB relative to ref_power, float64; P = 0 gives -inf"""
    p = np.asarray(power, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(p / float(ref_power))


def code_of_db(db):
    """dB -> the detector's uint16 code: rint (ties to even) of the position on the scale, clamped; -inf gives 0"""
    return np.clip(np.rint((np.asarray(db, dtype=np.float64) - ZERO_DB) / SLOPE), 0, 65535).astype(np.uint16)


def codes(power, ref_power):
    """the detector's dB-to-code scale in float64: P = 0 gives code 0"""
    return code_of_db(db_of(power, ref_power))


def plan(pos, carried, n, N, H, K):
    """(segments, chunks, frames, carried after) of a call: whole chunks only, counted segment by segment"""
    s0 = (pos - carried) // H
    avail = segments_complete(pos + n, N, H)
    s, chunks = s0, 0
    while True:
        left = K - s % K
        size = min(CHUNK, left)
        if s + size > avail:
            break
        s += size
        chunks += 1
    return s - s0, chunks, s // K - s0 // K, pos + n - s * H


# ---- the accuracy matrix of tests/test_psd_gpu.py, shared with the host test that measures its tolerance -------------------
MATRIX = ((256, 256), (256, 1), (512, 192), (1024, 512), (1024, 385), (2048, 2048), (4096, 1024), (4096, 4095))
SEGMENTS = (1, 3, 8, 9, 20)
# the complex64 implementation's worst max_k |P - P_ref| / max_k P_ref over the matrix (test_psd_host.py measures it and holds
# EPS to 4 times the figure, never above 1e-5)
C64_WORST = 3.2912e-7
EPS = 4 * C64_WORST


def matrix_samples(N, H, K):
    """two whole frames, the start of a third and an odd remainder"""
    return (2 * K + 3) * H + N + 17


def asymmetric_window(N):
    """a caller's window that is not symmetric: a rising ramp times a Hann window moved off the centre"""
    n = np.arange(N, dtype=np.float64)
    return ((0.25 + 0.75 * n / N) * (0.5 - 0.5 * np.cos(2.0 * np.pi * ((n + 0.3 * N) % N) / N)) + 0.01).astype(np.float32)


def matrix_signal(base, N, i16):
    """base = synth_iq of the length wanted (noise and two weak tones) plus one strong tone exactly on bin round(0.1 N) and
    one between bins at (-0.3 N + 0.5) / N.  Returns (what the context is fed, the same samples as float32)."""
    n = base.size // 2
    t = np.arange(n, dtype=np.float64)
    tone = 1.0 * np.exp(2j * np.pi * round(0.1 * N) / N * t) + 0.6 * np.exp(2j * np.pi * (-0.3 * N + 0.5) / N * t)
    x = np.asarray(base, dtype=np.float64).copy()
    x[0::2] += tone.real
    x[1::2] += tone.imag
    if i16:
        xi = np.clip(np.round(x * 10000.0), -32768, 32767).astype(np.int16)
        return xi, xi.astype(np.float32) * np.float32(2.0 ** -15)
    x = x.astype(np.float32)
    return x, x


# ---- long averages (tests/test_psd_long_gpu.py, measured on the host by tests/test_psd_host.py) -----------------------------
# (N, H, K): ceil(K / 8) from 126 to 8192 accumulator additions per frame
LONG = ((256, 1, 65535), (512, 2, 8200), (1024, 1, 4097), (1024, 385, 1003), (2048, 1, 8195), (4096, 1, 8209))
# the complex64 implementation's worst error over LONG x {float32, int16} x {Hann, asymmetric}, at (256, 1, 65535, int16, Hann)
C64_WORST_LONG = 3.226e-6


def eps_of(K):
    """SPEC §8's tolerance for a frame of K segments: EPS while the accumulator takes at most the 3 additions the matrix covers;
    beyond, every addition rounds once, by at most 2^-24 of a partial sum of non-negative terms that is at most the frame's
    peak.  Counting all ceil(K / 8) additions leaves three units for second order."""
    chunks = (K + CHUNK - 1) // CHUNK
    return EPS if chunks <= 3 else EPS + chunks * 2.0 ** -24


def long_samples(N, H, K):
    """one whole frame, 11 segments of the next and an odd remainder"""
    return (K + 11) * H + N + 5


def power_f64_segments(iq, N, H, K, seg_lo, seg_hi, window=None, first_bin=None, bins=None):
    """(bins,) float64: the sum of S over the stream's segments seg_lo .. seg_hi - 1 only, over K sum w^2: what a context whose
    stream starts inside a frame, at segment seg_lo of it, emits for that frame (seg_hi = K)"""
    w = (hann(N) if window is None else np.asarray(window, dtype=np.float32)).astype(np.float64)
    x = as_c(iq)
    assert 0 <= seg_lo < seg_hi <= segments_complete(x.size, N, H)
    sel = bin_indices(N, -N // 2 if first_bin is None else first_bin, N if bins is None else bins)
    seg = _segments(x, N, H, seg_hi)[seg_lo:]
    S = np.abs(np.fft.fft(seg * w, axis=1)[:, sel]) ** 2
    return S.sum(axis=0) / (K * np.sum(w * w))


def chunk_order_power(chunk_sums, K, N):
    """the frame a ones-window context of K segments makes of its float32 chunk sums ((chunks, bins), in chunk order): onto a
    float32 accumulator that starts at +0, one addition per chunk, then one float32 product by 1 / (K N) rounded once from
    float64 (sum w^2 = N exactly)"""
    chunk_sums = np.asarray(chunk_sums)
    assert chunk_sums.dtype == np.float32 and chunk_sums.shape[0] == (K + CHUNK - 1) // CHUNK
    acc = np.zeros(chunk_sums.shape[1], dtype=np.float32)
    for part in chunk_sums:
        acc = acc + part
    assert acc.dtype == np.float32
    return acc * np.float32(1.0 / (float(K) * float(N)))


def segment_order_sum(segment_powers):
    """a chunk sum from its segments' float32 powers ((segments, bins), in segment order): float32 additions onto +0"""
    segment_powers = np.asarray(segment_powers)
    assert segment_powers.dtype == np.float32 and 1 <= segment_powers.shape[0] <= CHUNK
    part = np.zeros(segment_powers.shape[1], dtype=np.float32)
    for s in segment_powers:
        part = part + s
    return part
