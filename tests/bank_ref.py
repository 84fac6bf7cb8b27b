"""Float64 reference of one channel of if_fir_channelizer_process_device_freq (docs/SPEC.md §3.3) on a WINDOW of a long stream, by the
definition:

    g = round(4096 f) / 4096;   hc[k] = h[k] exp(+j 2 pi g k)
    y[a] = exp(-j 2 pi ((P a) mod 2^32) / 2^32) * sum_k hc[k] x[a - k],    P = oracle.nco_phase_word(f),   a = 0 (mod d)

with `a` the ABSOLUTE sample index (64-bit: right past 2^32 samples).  Plain functions shared by tests/test_gpu_fullsize.py,
tests/test_gpu_parity.py and tests/test_oracle.py (which pins bank_window_ref to the C oracle for centres on the grid)."""
import numpy as np

GATHER = 1 << 22    # samples gathered per matrix product (rows of t samples each): 64 MiB of complex128


def shifted_taps(taps, centre):
    """hc[k] = h[k] exp(+j 2 pi g k) in float64, g = the multiple of 1/4096 nearest to `centre`.  (g k is an exact multiple
    of 1/4096 in binary64; it is reduced modulo 1 before the multiplication by 2 pi, so the angle is good to one rounding.)"""
    h = np.asarray(taps, dtype=np.float64)
    g = np.round(float(centre) * 4096.0) / 4096.0
    return h * np.exp(2j * np.pi * np.mod(g * np.arange(h.size), 1.0))


def mix_down(oracle, centre, a):
    """exp(-j 2 pi ((P a) mod 2^32) / 2^32) for absolute sample indices `a` (uint64 array), P = the 32-bit phase word of `centre`."""
    word = np.uint64(oracle.nco_phase_word(centre))
    lo = np.asarray(a, dtype=np.uint64) & np.uint64(0xFFFFFFFF)     # P a mod 2^32 needs a mod 2^32 only; P (a mod 2^32) < 2^64
    ph = ((word * lo) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0 ** 32
    return np.exp(-2j * np.pi * ph)


def interleave(y):
    out = np.empty(2 * y.size, dtype=np.float64)
    out[0::2], out[1::2] = y.real, y.imag
    return out


def bank_window_ref(oracle, taps, xs_with_history, t, d, centre, start):
    """Outputs of the channel at `centre` for the window's input samples a = 0 (mod d), in order (interleaved float64).
    xs_with_history: interleaved float32, the t - 1 samples of the stream before sample `start` (zeros where the stream has not begun)
    followed by the window's samples; start: absolute index of the window's first sample."""
    assert len(taps) == t
    xs = np.asarray(xs_with_history, dtype=np.float32).reshape(-1)
    xc = xs[0::2].astype(np.float64) + 1j * xs[1::2].astype(np.float64)
    w = xc.size - (t - 1)
    assert w >= 0
    first = (-start) % d            # the window's first sample with a = 0 (mod d)
    m = (w - first + d - 1) // d if w > first else 0
    rev = shifted_taps(taps, centre)[::-1].copy()
    # y[i] = sum_k hc[k] x[start + first + i d - k] = sum_j xc[first + i d + j] rev[j]: rows of t consecutive samples, d apart
    rows = np.lib.stride_tricks.as_strided(xc[first:], shape=(m, t), strides=(d * xc.strides[0], xc.strides[0]), writeable=False)
    y = np.empty(m, dtype=np.complex128)
    step = max(1, GATHER // t)
    for i in range(0, m, step):
        y[i:i + step] = rows[i:i + step] @ rev
    a = np.uint64(start + first) + np.uint64(d) * np.arange(m, dtype=np.uint64)
    return interleave(y * mix_down(oracle, centre, a))

