"""Reference of the polyphase synthesis bank (docs/SPEC.md §14), plain numpy, like tests/pfb_ref.py:

    y[n] = sum_k e^{+j 2 pi k n / M} sum_m h[n - m L] X_k[m],   n = absolute output index,   X_k[m<0] = 0

* definition_f64: §14 defines the bank as the sum of M interpolators with their NCO at k / M, which is the channel combiner's
  definition with centres on the grid: tests/combiner_ref.reference with words[k] = (k << 32) // M.  O(channels) convolutions:
  for the small shapes.
* fold_f64: the fold form in float64 -- one inverse M-point transform per frame, then J = ceil(T / L) taps per output.  Equal to
  the definition to 1e-12 (tests/test_synth_host.py), and cheap enough for M = 4096 with 65536 taps.
* model_c64: the same in float32 / complex64 in the order the SPEC states (j = 0 .. J-1 onto a zero, newest frame first), the
  FORWARD scipy.fft on complex64 read at the mirrored bin.
* transfer_f64: what an analysis bank (tests/pfb_ref.py, prototype h, hop L) followed by this bank (prototype g) does to a stream.
* sample_count: the outputs of a call.
* ring_model_c64: model_c64 walked as synth_ring_kernel walks a call (runs, ring slots, warm-up), with switchable faults of its
  index algebra; DEPTH_CASES: the (M, J) pairs at every step of the ring depth, the route switches and the sizes' limits, two
  shapes each (tests/test_synth_matrix_gpu.py; tests/test_synth_host.py shows that the faults move them).

Frames are (frames, bins) complex arrays, element j = channel (first_bin + j) mod M, of a call whose first frame has absolute
index `first`, with zero frames before it; the results are complex arrays of frames * L outputs."""
import numpy as np
import scipy.fft

import combiner_ref
from pfb_ref import SIZES, channels

__all__ = ["SIZES", "channels", "sample_count", "terms", "definition_f64", "fold_f64", "model_c64", "ring_model_c64", "transfer_f64", "iq",
           "DEPTH_J", "DEPTH_CASES", "depth_shapes", "RING_STEP_CASES", "RING_FAULTS"]


def sample_count(frames, L):
    return frames * L


def terms(T, L):
    """J = ceil(T / L)"""
    return -(-T // L)


def batch(M):
    """frames a workgroup transforms together"""
    return max(1, 1024 // M)


def lds_route_fits(M, T, L, groups=2):
    """`groups` workgroups of the one-kernel route's ring of ceil((J-1)/B) + 1 batches (8 bytes a point), the twiddles and the
    places fit the 160 KB of a CU's LDS: with two the route can be forced, with four it is the plan's choice"""
    B = batch(M)
    return groups * ((-(-(terms(T, L) - 1) // B) + 1) * B * M * 8 + 10 * M) <= 160 * 1024


def iq(y):
    """complex -> interleaved, for oracle.err_metrics"""
    y = np.asarray(y).reshape(-1)
    return np.stack([y.real, y.imag], axis=1).reshape(-1)


def as_frames(x, bins):
    """interleaved (I, Q) values -> (frames, bins) complex128"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    return (x[:, 0] + 1j * x[:, 1]).reshape(-1, bins)


def definition_f64(h, X, M, L, first_bin=0, bins=None, first=0):
    """the sum of interpolators: channel (first_bin + j) mod M through combiner_ref.reference at phase word k 2^32 / M"""
    X = np.asarray(X, dtype=np.complex128)
    ch = channels(M, first_bin, X.shape[1] if bins is None else bins)
    xs = [iq(X[:, j]) for j in range(ch.size)]
    words = [(int(k) << 32) // M for k in ch]
    y = combiner_ref.reference(h, xs, L, words, first_out=(first * L) % (1 << 32))
    return combiner_ref.as_c(y)


def _fold(h, X, M, L, first_bin, bins, first, dtype):
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    h = np.asarray(h, dtype=dtype).reshape(-1)
    T = h.size
    J = terms(T, L)
    X = np.asarray(X).astype(ctype)
    F = X.shape[0]
    full = np.zeros((F + J - 1, M), dtype=ctype)           # J - 1 zero frames before the call
    full[J - 1:, channels(M, first_bin, X.shape[1] if bins is None else bins)] = X
    fwd = scipy.fft.fft(full, axis=1)
    assert fwd.dtype == ctype
    v = fwd[:, (M - np.arange(M)) % M]                      # v_m[s] = F_m[(M - s) mod M]
    r = np.arange(F * L, dtype=np.int64)
    f, p = r // L, r % L
    s = (((first * L) % M) + r) % M
    hp = np.zeros(J * L, dtype=dtype)
    hp[:T] = h
    acc = np.zeros(F * L, dtype=ctype)
    for j in range(J):                                      # newest frame first
        t = p + j * L
        term = hp[t] * v[f + J - 1 - j, s]
        acc = np.where(t < T, acc + term, acc)
    assert acc.dtype == ctype
    return acc


def fold_f64(h, X, M, L, first_bin=0, bins=None, first=0):
    return _fold(h, X, M, L, first_bin, bins, first, np.float64)


def model_c64(h, X, M, L, first_bin=0, bins=None, first=0):
    return _fold(h, X, M, L, first_bin, bins, first, np.float32)


def transfer_f64(h, g, x, M, L):
    """y[n] = M sum_i x[n - i M] sum_m g[n - m L] h[i M - (n - m L)] for the frames m with 0 <= m L < len(x): what
    pfb_ref.fold_f64(h, x, M, L) followed by fold_f64(g, ., M, L) gives, from a stream that starts at index 0.
    x: complex samples; returns ceil(len(x) / L) L outputs"""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    n = x.size
    F = -(-n // L)
    y = np.zeros(F * L + g.size, dtype=np.complex128)
    u = np.arange(g.size)
    for m in range(F):
        w = np.zeros(g.size, dtype=np.complex128)
        for i in range((h.size + g.size) // M + 2):
            t = i * M - u                                   # the analysis tap
            at = m * L + u - i * M                          # = n - i M
            ok = (t >= 0) & (t < h.size) & (at >= 0) & (at < n)
            w[ok] += h[t[ok]] * x[at[ok]]
        y[m * L:m * L + g.size] += M * g * w
    return y[:F * L]


# ---- the one-kernel route's walk of a call ----

RING_FAULTS = ("back_on_multiple", "warmup_short", "last_term_dropped", "history_ignored")


def ring_model_c64(h, X, M, L, run_len, hist_frames=None, fault=None, first=0):
    """model_c64 of a full-width call, computed the way synth_ring_kernel<M> walks it: runs of `run_len` batches of B frames;
    a ring of NB = ceil((J-1)/B) + 1 transformed batches in natural slot order, which lives on from run to run as the LDS does;
    before a run the NB - 1 batches before it, from the call, then from `hist_frames` (the J - 1 frames before the call, zeros
    when None), then zeros; per output the kernel's back = j > fbi ? (j - fbi + B - 1) / B : 0, slot = cur - back (+ NB) and
    fb = (fbi - j) & (B - 1).  `first`: the absolute index of the call's first frame.  With fault=None the bits of model_c64.

    Test-only switches, each one fault of that algebra: "back_on_multiple": back = (j - fbi + B) / B for j > fbi (one more
    where j - fbi is a multiple of B); "warmup_short": the warm-up starts one batch late; "last_term_dropped": term J - 1 is
    skipped when T < J L; "history_ignored": the frames before the call read zero."""
    assert fault is None or fault in RING_FAULTS, fault
    h = np.asarray(h, dtype=np.float32).reshape(-1)
    T = h.size
    J, B = terms(T, L), batch(M)
    NB = -(-(J - 1) // B) + 1
    X = np.asarray(X).astype(np.complex64)
    F = X.shape[0]
    assert X.shape == (F, M) and run_len >= 1
    hist = np.zeros((J - 1, M), dtype=np.complex64)
    if hist_frames is not None and fault != "history_ignored":
        hist[:] = np.asarray(hist_frames).astype(np.complex64).reshape(J - 1, M)
    src = np.concatenate([hist, X])                             # frame f of the call in row f + J - 1
    hp = np.zeros(J * L, dtype=np.float32)
    hp[:T] = h
    mirror = (M - np.arange(M)) % M
    batches = -(-F // B)
    smod = (first * L) % M
    ring = np.zeros((NB, B, M), dtype=np.complex64)
    out = np.zeros(F * L, dtype=np.complex64)
    for q0 in range(0, batches, run_len):
        q1 = min(batches, q0 + run_len)
        cur = 0
        for q in range(q0 - (NB - 1) + (fault == "warmup_short" and NB > 1), q1):
            x = np.zeros((B, M), dtype=np.complex64)            # before the history and past the call: 0
            rows = np.arange(q * B, q * B + B) + J - 1
            ok = (rows >= 0) & (rows < F + J - 1)
            x[ok] = src[rows[ok]]
            fwd = scipy.fft.fft(x, axis=1)
            assert fwd.dtype == np.complex64
            ring[cur] = fwd[:, mirror]
            if q >= q0:
                f0 = q * B
                i = np.arange(min(B, F - f0) * L, dtype=np.int64)
                fbi, p = i // L, i % L
                s = (smod + f0 * L + i) % M
                acc = np.zeros(i.size, dtype=np.complex64)
                for j in range(J):
                    if fault == "last_term_dropped" and j == J - 1 and T < J * L:
                        continue
                    t = p + j * L
                    back = np.where(j > fbi, (j - fbi + (B if fault == "back_on_multiple" else B - 1)) // B, 0)
                    slot = np.where(cur - back < 0, cur - back + NB, cur - back)
                    fb = (fbi - j) & (B - 1)
                    acc = np.where(t < T, acc + hp[t] * ring[slot, fb, s], acc)
                assert acc.dtype == np.complex64
                out[f0 * L:f0 * L + i.size] = acc
            cur = 0 if cur + 1 == NB else cur + 1
    return out


# ---- the depth cases ----

def _largest_j(M, groups):
    """the largest J in 1 .. 32 whose ring fits `groups` times into a CU, 0 where none does"""
    return max([J for J in range(1, 33) if lds_route_fits(M, J, 1, groups)], default=0)


def depth_terms(M):
    """the J of a size: both ends, either side of every step of NB = ceil((J-1)/B) + 1 up to its third value, the most, and
    either side of the plan's switch (four workgroups a CU) and of the ring's limit (two)"""
    B, J4, J2 = batch(M), _largest_j(M, 4), _largest_j(M, 2)
    return tuple(sorted(J for J in {1, 2, B - 1, B, B + 1, B + 2, 2 * B, 2 * B + 1, 2 * B + 2, 32, J4, J4 + 1, J2, J2 + 1} if 1 <= J <= 32))


def depth_shapes(M, J):
    """the two (M, T, L) of a pair: A with J terms in every phase; B with a hop that divides nothing and the J-th term in phase 0
    only (T = L where J = 1).  L = M up to J = 16 and M / 2 beyond, so that T <= 16 M; less one in B"""
    top = M if J <= 16 else M // 2
    return (M, J * top, top), (M, (J - 1) * (top - 1) + 1 if J > 1 else top - 1, top - 1)


DEPTH_J = {M: depth_terms(M) for M in SIZES}
DEPTH_CASES = tuple(c for M in SIZES for J in DEPTH_J[M] for c in depth_shapes(M, J))
# one A shape per batch size, J on a step of NB, and the two sizes whose ring holds no more: runs and cuts through the ring
RING_STEP_CASES = tuple(depth_shapes(M, J)[0] for M, J in ((64, 17), (128, 9), (256, 5), (512, 17), (1024, 8), (2048, 3), (4096, 1)))

assert DEPTH_J == {64: (1, 2, 15, 16, 17, 18, 32), 128: (1, 2, 7, 8, 9, 10, 16, 17, 18, 25, 26, 32),
                   256: (1, 2, 3, 4, 5, 6, 8, 9, 10, 13, 14, 32), 512: (1, 2, 3, 4, 5, 6, 7, 8, 17, 18, 32), 1024: (1, 2, 3, 4, 8, 9, 32),
                   2048: (1, 2, 3, 4, 32), 4096: (1, 2, 3, 4, 32)}, DEPTH_J
assert len(DEPTH_CASES) == len(set(DEPTH_CASES)) == 118 and sum(lds_route_fits(*c) for c in DEPTH_CASES) == 98
assert all(terms(T, L) == J and T <= 16 * M for M in SIZES for J in DEPTH_J[M] for _, T, L in depth_shapes(M, J))
assert all(c in DEPTH_CASES and lds_route_fits(*c) for c in RING_STEP_CASES)
