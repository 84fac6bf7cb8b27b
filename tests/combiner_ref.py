"""The channel combiner (if_fir_combiner_t, docs/SPEC.md §9) in numpy: the definition in float64, the third-party form
(scipy.signal.upfirdn), a complex64 model of the overlap-save route, and the case matrices (cases, boundary_cases, move_cases),
signals and centres the CPU and GPU tests share.  Plain functions, like tests/bank_ref.py.

    u_c[n] = x_c[n/L] if n mod L == 0 else 0;   y[n] = sum_c exp(+j 2 pi P_c (n mod 2^32) / 2^32) sum_k h[k] u_c[n-k]"""
import functools

import numpy as np

TAPS = (31, 255, 1023, 3073)
FAST_L = (4, 8, 16, 64)
GENERIC_L = (1, 2, 3, 5, 16)
SPECIAL_CENTRES = (0.0, 0.5, -0.5, 37.0 / 4096, 100.5 / 4096, 0.2003, 0.2003, -0.3107)   # the C = 8 shape at L = 8 carries these


def as_c(y):
    y = np.asarray(y, dtype=np.float64).reshape(-1, 2)
    return y[:, 0] + 1j * y[:, 1]


def as_iq(c):
    return np.stack([c.real, c.imag], axis=1).reshape(-1)


def taps_c(taps, complex_taps):
    t = np.asarray(taps, dtype=np.float32).astype(np.float64)
    return t[0::2] + 1j * t[1::2] if complex_taps else t.astype(np.complex128)


def phase_word(f):
    """P = round(f 2^32) mod 2^32, as if_fir_interp_set_nco"""
    return int(round(float(f) * 4294967296.0)) % (1 << 32)


def split_word(P):
    """P = G 2^20 + r (mod 2^32): G = ((P + 2^19) mod 2^32) >> 20 in 0..4095, r the signed remainder in -2^19 .. 2^19 - 1"""
    G = ((P + (1 << 19)) % (1 << 32)) >> 20
    r = (P - (G << 20)) % (1 << 32)
    return G, r - (1 << 32) if r >= (1 << 31) else r


def rotation(P, first_out, count):
    """exp(+j 2 pi P (n mod 2^32) / 2^32), n = first_out .. first_out + count - 1, the phase reduced in integers"""
    n = (np.arange(count, dtype=np.uint64) + np.uint64(first_out % (1 << 32))) % np.uint64(1 << 32)
    ph = (n * np.uint64(P)) % np.uint64(1 << 32)     # (wraps mod 2^64, a multiple of 2^32)
    return np.exp(2j * np.pi * ph.astype(np.float64) / 4294967296.0)


def interpolate_f64(h, x, L):
    """sum_k h[k] u[n-k] for n = 0 .. len(x) L - 1, phase by phase: y[p + j L] = sum_i h[p + i L] x[j - i] (complex128)"""
    n = x.size
    y = np.zeros(n * L, dtype=np.complex128)
    for p in range(min(L, h.size)):
        y[p::L] = np.convolve(x, h[p::L])[:n]
    return y


def reference(taps, xs, L, words, complex_taps=False, first_out=0):
    """the definition in float64: xs = one interleaved float32 array per channel, words = the phase words P_c; interleaved"""
    h = taps_c(taps, complex_taps)
    y = 0
    for x, P in zip(xs, words):
        yc = interpolate_f64(h, as_c(x), L)
        y = y + yc * rotation(P, first_out, yc.size)
    return as_iq(y)


def reference_upfirdn(taps, xs, L, words, complex_taps=False):
    """the third-party form: a sum of scipy.signal.upfirdn(h, x_c, up=L)[:N L], rotated per channel"""
    import scipy.signal
    h = taps_c(taps, complex_taps)
    y = 0
    for x, P in zip(xs, words):
        x = as_c(x)
        yc = np.zeros(x.size * L, dtype=np.complex128)
        got = scipy.signal.upfirdn(h, x, up=L)[:x.size * L]   # (fewer than N L values when T < L: the rest are zero)
        yc[:got.size] = got
        y = y + yc * rotation(P, 0, yc.size)
    return as_iq(y)


def overlap_rows(T):
    return next((r for r in (4, 8, 16, 32, 48) if 64 * r >= T - 1), 48)


def table_f64(h, r):
    """the multiply table of residual r: FFT_4096(h[k] exp(j 2 pi r k / 2^32)) / 4096 in float64"""
    k = np.arange(h.size, dtype=np.float64)
    return np.fft.fft(h * np.exp(2j * np.pi * r * k / 4294967296.0), 4096) / 4096


def model_c64(taps, xs, L, words, complex_taps=False, first_out=0, move_extra=0, keep_early=0, table_of=None):
    """the overlap-save route in single precision: per block of 4096 output-rate points and per channel the 4096/L input
    samples rotated by the residual at their absolute index and by the block's scalar exp(j 2 pi G n0 / 4096) (float32
    phasors), a complex64 transform (scipy.fft), times the float32 table read modulo 4096/L, moved by G bins, summed over the
    channels in complex64; one complex64 inverse; positions overlap .. 4095 kept.  One call from a zero history.

    Test-only switches, each one fault of the index algebra (tests/test_combiner_host.py shows that the case lists notice them):
    move_extra = e: the bins are moved by G + e; keep_early = k: a block keeps positions overlap - k .. 4095 (its first k values
    replace the block before's last); table_of = (c, d): channel c is multiplied by the table of channel d's residual."""
    import scipy.fft
    h = taps_c(taps, complex_taps)
    T = h.size
    ovl = 64 * overlap_rows(T)
    A, nf = 4096 - ovl, 4096 // L
    n_in = as_c(xs[0]).size
    M = n_in * L
    y = np.zeros(M, dtype=np.complex64)
    chans = []
    for x, P in zip(xs, words):
        G, r = split_word(P)
        x = np.concatenate([np.zeros(ovl // L, dtype=np.complex64), as_c(x).astype(np.complex64), np.zeros(nf, dtype=np.complex64)])
        chans.append((x, G, r, table_f64(h, r).astype(np.complex64)))
    if table_of is not None:
        c, d = table_of
        chans[c] = chans[c][:3] + (chans[d][3],)
    tw =np.exp(2j * np.pi * np.arange(4096) / 4096).astype(np.complex64)
    bins = np.arange(4096)
    for b in range(-(-M // A)):
        n0 = first_out + b * A - ovl
        acc = np.zeros(4096, dtype=np.complex64)
        for x, G, r, H in chans:
            blk = x[b * (A // L):b * (A // L) + nf]
            w = np.full(nf, tw[(G * (n0 % 4096)) % 4096], dtype=np.complex64)
            if r:
                w = w * rotation(r % (1 << 32), n0 % (1 << 32), 4096)[::L].astype(np.complex64)
            X = scipy.fft.fft((blk * w).astype(np.complex64))
            k = (bins - G - move_extra) % 4096
            acc = acc + H[k] * X[k % nf]
        z = (scipy.fft.ifft(acc) * np.float32(4096)).astype(np.complex64)
        keep = min(4096, M - (b * A - ovl))
        early = keep_early if b else 0
        y[b * A - early:b * A - ovl + keep] = z[ovl - early:keep]
    return as_iq(y.astype(np.complex128))


# ---- the matrix of the tests ----

def cases(route):
    """(L, C, T, complex taps, int16 input) of a route ("fft" or "generic"): every L of the route x C in {1, 2, 3, 8} (+ 16 at
    L = 16, 64 at L = 64 on the overlap-save route) x real / complex taps x float32 / int16, T cycled over the matrix"""
    out = []
    for L in (FAST_L if route == "fft" else GENERIC_L):
        cs = [1, 2, 3, 8] + ([16] if L == 16 else []) + ([64] if L == 64 and route == "fft" else [])
        for ci, C in enumerate(cs):
            for ct in (False, True):
                for i16 in (False, True):
                    T = TAPS[(L + ci + 2 * ct + i16 + (route == "generic")) % 4]
                    out.append((L, C, T, ct, i16))
    return out


BOUNDARY_TAPS = (1, 2, 3, 256, 257, 258, 512, 513, 514, 1024, 1025, 1026, 2048, 2049, 2050, 3072, 3073)
BOUNDARY_L = (4, 8, 16, 32, 64)   # every L the overlap-save route takes
ROWS_TAPS = {4: 257, 8: 513, 16: 1025, 32: 2049, 48: 3073}   # T - 1 = overlap: the longest filter of each rows class


def boundary_cases():
    """(L, C, T, complex taps, int16 input) on the overlap-save route: every tap count either side of an overlap class x every
    L, the flags and the channel count cycled so that every compiled (rows, int16) unit, and complex taps in every rows class,
    come up (asserted below)"""
    out = []
    for ti, T in enumerate(BOUNDARY_TAPS):
        for li, L in enumerate(BOUNDARY_L):
            c = li + 3 * (ti % 3)
            out.append((L, (1, 2, 3, 8)[(ti + li) % 4], T, bool((c >> 1) & 1) ^ bool(ti % 2), bool(c & 1)))
    return out


def boundary_coverage():
    """of boundary_cases(): the (rows, int16) units, the L, the tap counts, the rows classes with complex taps"""
    cs = boundary_cases()
    return ({(overlap_rows(T), i16) for L, C, T, ct, i16 in cs}, {L for L, *_ in cs}, {T for L, C, T, ct, i16 in cs},
            {overlap_rows(T) for L, C, T, ct, i16 in cs if ct})


_ROWS = (4, 8, 16, 32, 48)
assert boundary_coverage() == ({(r, a) for r in _ROWS for a in (False, True)}, set(BOUNDARY_L), set(BOUNDARY_TAPS), set(_ROWS))
assert [overlap_rows(T) for T in (1, 257, 258, 513, 514, 1025, 1026, 2049, 2050, 3073)] == [4, 4, 8, 8, 16, 16, 32, 32, 48, 48]

# phase words at the edges of the split P = G 2^20 + r: G = 0, 1, 4095, 2048, 2047 on the grid; both sides of a half-way word
# (r = -2^19 with G = 101 and G = 100, r = 2^19 - 1); r = +-1; r = 12345 under G = 4095; r = -2^19 under G = 2048; two off the grid
MOVE_WORDS = (0, 1 << 20, 4095 << 20, 1 << 31, 2047 << 20, (100 << 20) + (1 << 19), (100 << 20) + (1 << 19) - 1,
              (100 << 20) - (1 << 19), 1, (1 << 32) - 1, (4095 << 20) + 12345, (2048 << 20) - (1 << 19),
              phase_word(0.2003), phase_word(-0.3107))
MOVE_SEEK = 12345    # input samples: the blocks' first points n0 are no multiples of 64 then, so G n0 takes every residue
assert sum(split_word(P)[1] == -(1 << 19) for P in MOVE_WORDS) == 3                       # three share one table
assert sum(split_word(P)[1] == 0 and split_word(P)[0] != 0 for P in MOVE_WORDS) == 4      # four use table 0 with G != 0


class Words(tuple):
    """the centres of a case given as phase words (in the place of a channel count); .seek = the input samples per channel the
    stream stands at when the call begins"""
    def __new__(cls, words, seek=0):
        self = super().__new__(cls, words)
        self.seek = int(seek)
        return self

    def __eq__(self, other):
        return isinstance(other, Words) and tuple(self) == tuple(other) and self.seek == other.seek

    def __hash__(self):
        return hash((tuple(self), self.seek))

    def __repr__(self):
        return "Words(%d at %d)" % (len(self), self.seek)


def word_centre(P):
    """the centre of a phase word in cycles per sample, signed(P) / 2^32: exact in a double"""
    return (P - (1 << 32) if P >= 1 << 31 else P) / 4294967296.0


def move_cases():
    """(L, Words, T, complex taps, int16 input): per L every word of MOVE_WORDS as a channel of one context (T = 513 or 2049,
    rows 8 or 32), from position 0 and from MOVE_SEEK; at L = 4 and 64 each word alone after the seek, where a wrong move of one
    channel cannot hide in a sum"""
    out = []
    for L in BOUNDARY_L:
        for seek in (0, MOVE_SEEK):
            out.append((L, Words(MOVE_WORDS, seek), 513 if L in (4, 16, 64) else 2049, True, False))
    for L in (4, 64):
        for P in MOVE_WORDS:
            out.append((L, Words((P,), MOVE_SEEK), 513, True, False))
    return out


def case_id(case):
    L, C, T, ct, i16 = case
    if isinstance(C, Words):
        return "L%d-%s@%d-T%d" % (L, "all" if len(C) > 1 else "%#x" % C[0], C.seek, T)
    return "%d-%d-%d-%s-%s" % case


def stream_samples(T, L):
    """M = 3 (4096 - 64 rows) + 517 outputs, N = ceil(M / L), at least 2 ceil(T / L) + 17 samples: a block loop, a ragged last
    block and a partly filled history all occur"""
    M = 3 * (4096 - 64 * overlap_rows(T)) + 517
    return max(-(-M // L), 2 * (-(-T // L)) + 17)


def centres_for(L, C):
    """spread over (-0.45, 0.45) and off the 1/4096 grid; the C = 8 shape at L = 8 carries the special centres"""
    if C == 8 and L == 8:
        return np.array(SPECIAL_CENTRES)
    c = np.arange(C)
    return -0.45 + 0.9 * (c + 0.5) / C + (0.3 + 0.005 * c) / 4096


_signals = {}


def signals(oracle, n, C, i16):
    """per channel c: (what the library is given, the same samples as float32) from synth_iq(channel=c).  int16: level 14000
    with the full-scale samples of matrix_util.signal at its positions (the ends, scattered, a run), rotated by the channel"""
    import matrix_util
    out = []
    for c in range(C):
        if (n, c, i16) not in _signals:
            x = oracle.synth_iq(n, channel=c)
            if i16:
                full = matrix_util.signal(oracle, n, True)[0].reshape(-1, 2)
                at = np.flatnonzero(np.any(np.abs(full.astype(np.int32)) >= 32767, axis=1))
                xi = np.clip(np.round(x * 14000.0), -32768, 32767).astype(np.int16).reshape(-1, 2)
                xi[at] = full[np.roll(at, c)]
                xi = xi.reshape(-1)
                _signals[(n, c, i16)] = (xi, xi.astype(np.float32) * np.float32(2.0 ** -15))
            else:
                _signals[(n, c, i16)] = (x, x)
        out.append(_signals[(n, c, i16)])
    return [o[0] for o in out], [o[1] for o in out]


@functools.lru_cache(maxsize=None)
def case_reference(L, C, T, ct, i16):
    """(taps, raw inputs, float32 inputs, centres, phase words, float64 reference) of a matrix case, computed once; C = a channel
    count (centres_for) or Words (the reference then begins at output index C.seek L)"""
    import __graft_entry__ as g
    import matrix_util
    oracle = g.load_oracle()
    taps = matrix_util.edge_taps(T, L, ct)
    if isinstance(C, Words):
        raw, xs = signals(oracle, stream_samples(T, L), len(C), i16)
        words = list(C)
        centres = np.array([word_centre(P) for P in words])
        return taps, raw, xs, centres, words, reference(taps, xs, L, words, ct, first_out=C.seek * L)
    raw, xs = signals(oracle, stream_samples(T, L), C, i16)
    centres = centres_for(L, C)
    words = [phase_word(f) for f in centres]
    return taps, raw, xs, centres, words, reference(taps, xs, L, words, ct)
