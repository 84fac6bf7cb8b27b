"""docs/SPEC.md §20 in numpy: the corner turn in both directions and all four format pairs, on raw arrays -- float32 elements as
(..., 2) float32, int16 elements as (..., 2) int16 -- so that every comparison is on bits.  Plus the selections, signals and
shape sets the host and GPU tests share.  Plain functions, like tests/fpow_ref.py."""
import numpy as np

TO_STREAMS, TO_FRAMES = 0, 1
FRAMES = (0, 1, 2, 63, 64, 65, 127, 129, 1000)          # the issue's edge sets
CHANNELS = (1, 2, 3, 63, 64, 65, 200)                   # ... and C = B
BINS = (1, 64, 65, 918, 4097, 8192)
SELECTIONS = ("span", "reversed", "scattered", "straddle")
FORMATS = ((False, False), (False, True), (True, False), (True, True))     # (int16 in, int16 out)


def to_i16(v):
    """one float32 component to int16, SPEC §11's rule with §20's own for a NaN, spelled out: the value times 2^15 (exact in
    float32 short of overflow, which gives the infinity that saturates), to nearest even, saturated at -32768 / 32767 (+-inf
    saturate); a NaN gives 0"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.rint(v * np.float32(32768.0))
    nan = np.isnan(v)
    s = np.where(nan, np.float32(0), s)
    s = np.where(s > 32767.0, np.float32(32767), np.where(s < -32768.0, np.float32(-32768), s))
    return s.astype(np.int16)


def conv(x, out_i16):
    """elements (..., 2), float32 or int16, to the output format"""
    if x.dtype == np.int16:
        return x.copy() if out_i16 else x.astype(np.float32) * np.float32(2.0 ** -15)
    assert x.dtype == np.float32
    return to_i16(x) if out_i16 else x.copy()


def to_streams(frames, sel, out_i16):
    """frames (F, B, 2) -> rows (C, F, 2): out[c][a] = conv(in[a][sel[c]])"""
    return np.ascontiguousarray(np.swapaxes(conv(frames[:, np.asarray(sel, dtype=np.int64)], out_i16), 0, 1))


def to_frames(rows, sel, B, out_i16):
    """rows (C, F, 2) -> frames (F, B, 2): out[a][sel[c]] = conv(in[c][a]), every other element all bits zero"""
    C, F = rows.shape[:2]
    out = np.zeros((F, B, 2), dtype=np.int16 if out_i16 else np.float32)
    out[:, np.asarray(sel, dtype=np.int64)] = np.swapaxes(conv(rows, out_i16), 0, 1)
    return out


def tile_cols(cols):
    """columns of the kernel's tile (csrc/if_fir_turn_plan.h, turn_tile_shift): the power of two at or above min(cols, 64)"""
    x = 1
    while x < 64 and x < cols:
        x *= 2
    return x


def selection(kind, B, C):
    """C distinct bins of a frame of B.  span: from the highest first bin that is not 0 where there is room; reversed: the same
    downwards; scattered: a seeded draw in its random order; straddle: pairs of bins on either side of every multiple of 64 (the
    widest tile's edges on the frame side), filled up from the top, rotated by one place so that a pair sits at an odd and the
    next even place of the list"""
    first = min(3, B - C)
    if kind == "span":
        return list(range(first, first + C))
    if kind == "reversed":
        return list(range(first + C - 1, first - 1, -1))
    rng = np.random.default_rng([B, C, 20])
    if kind == "scattered":
        return [int(v) for v in rng.permutation(B)[:C]]
    assert kind == "straddle"
    edge = [b for e in range(64, B, 64) for b in (e - 1, e)]
    taken = set(edge)
    rest = [b for b in range(B - 1, -1, -1) if b not in taken]
    pool = (edge + rest)[:C]
    return pool[-1:] + pool[:-1]


def special_f32():
    """float32 components that the int16 rule must get right and a bit copy must keep: NaNs with payloads, infinities, -0,
    denormals, the saturation edges +-(32767.5 * 2^-15) and their neighbours, ties to even, the largest finite value"""
    bits = np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0x7fffffff, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001,
                     0x80000001, 0x007fffff, 0x807fffff, 0x7f7fffff, 0xff7fffff], dtype=np.uint32).view(np.float32)
    q = np.float32(2.0 ** -15)
    edges = np.array([32767.5, -32767.5, 32767.49, 32766.5, 32767.0, -32768.0, -32768.5, -32768.51, 32768.0, 1e6, -1e6], dtype=np.float32) * q
    edges = np.concatenate([edges, np.nextafter(edges, np.float32(np.inf)), np.nextafter(edges, np.float32(-np.inf))]).astype(np.float32)
    ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, 0.50000006, 1000.5, 1001.5, -1000.5], dtype=np.float32) * q
    return np.concatenate([bits, edges, ties]).astype(np.float32)


def make_elements(shape, i16, seed):
    """seeded elements (*shape, 2): int16 over the whole range with the extremes present; float32 normal at level 0.3 (so that
    the int16 rule saturates some) with the special values strewn in"""
    rng = np.random.default_rng([seed, int(i16), 7])
    n = int(np.prod(shape)) * 2
    if i16:
        x = rng.integers(-32768, 32768, n, dtype=np.int64).astype(np.int16)
        if n >= 4:
            x[[0, 1, -2, -1]] = [32767, -32768, -32768, 32767]
    else:
        x = (0.3 * rng.standard_normal(n)).astype(np.float32)
        sp = special_f32()
        if n >= 8:
            at = rng.permutation(n)[:min(n // 4, 4 * sp.size)]
            x[at] = sp[np.arange(at.size) % sp.size]
    return x.reshape(tuple(shape) + (2,))


def same_bits(a, b):
    """bit equality of two raw arrays (NaN payloads and -0 count)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
