"""docs/SPEC.md §19 restated in numpy, written from the spec text: the frame power stage's output-frame count, its powers in
float64 (power_f64) and the float32 ORDER MODEL (model_f32), whose bits the GPU must give.

    p(a, i)  = fma(re, re, im*im)                              element i of input frame a (int16: the exact float32 value first)
    e_a[j]   = ((+0 + p(a, F0 + jG)) + p(a, F0 + jG + 1)) + ...   G terms in element order
    chunk    : a frame's e_a in chunks of 8 counted from a = fK, a chunk sum from +0 in frame order
    acc[j]   : from +0, the chunk sums in chunk order
    P[f][j]  = acc[j] * float32(1 / (K G fNorm))

The fma is a real one: tests/c/fpow_fma.c, compiled here into a small shared object and called through ctypes.  Every addition
is a numpy float32 addition, which rounds once.  A stream that starts at position c with nothing carried equals a stream from
the frame boundary below c whose first c mod K frames are zero: adding +0 changes no bit, so both references pad.

Frames are (F, B) arrays; the codes are psd_ref.codes (§8's mapping, stated once for both families)."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from psd_ref import codes  # noqa: F401  (the mapping of §8, unchanged)

CHUNK = 8
HERE = os.path.dirname(os.path.abspath(__file__))
_keep = []

# (B, first, G, Bo, K) of the GPU test: one element; Bo one short of a wave, K one short of a chunk; an odd B (every other row off
# the 16-byte grid) and an odd first element at a whole chunk; G = 2 with a chunk and a frame; G = 3 (no vector width divides it),
# two whole chunks and one frame; the detector's 918 bins at two chunks and a half; the real bank's 4097 elements in the
# widest group; the widest frame at K = 1 (every frame is an output frame); the longest average
MATRIX = ((1, 0, 1, 1, 1), (63, 0, 1, 63, 7), (65, 1, 1, 64, 8), (130, 2, 2, 64, 9), (200, 5, 3, 65, 17), (918, 0, 1, 918, 20),
          (4097, 1, 64, 64, 3), (8192, 0, 8, 1024, 1), (3, 0, 1, 3, 65535))
NORM = 0.8125                      # fNorm of the tests: not a power of two, exact in float32
# the chain IfFirPfb(taps = reversed window) -> IfFirFpow against the estimator (SPEC §19): the worst error of a plain complex64
# model (pfb_ref.model_c64 into model_f32) against float64 over CHAIN_SHAPES, relative to the frame's peak;
# tests/test_fpow_host.py re-measures it and holds CHAIN_EPS to 4 times the figure, never above 1e-5
CHAIN_SHAPES = ((256, 256, 3), (512, 192, 2))
CHAIN_C64_WORST = 1.2179e-7
CHAIN_EPS = 4 * CHAIN_C64_WORST


def frame_count(c, F, K):
    """output frames of a call with F frames at position c (Python integers: any position)"""
    return (c + F) // K - c // K


@functools.lru_cache(maxsize=None)
def _fma_lib():
    tmp = tempfile.TemporaryDirectory(prefix="fpow_fma")
    _keep.append(tmp)
    so = os.path.join(tmp.name, "libfpow_fma.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "c", "fpow_fma.c"), "-o", so, "-lm"])
    L = ctypes.CDLL(so)
    f32p = ctypes.POINTER(ctypes.c_float)
    L.fpow_p.argtypes = [f32p, f32p, f32p, ctypes.c_size_t]
    L.fpow_p.restype = None
    return L


def element_power_f32(re, im):
    """fma(re, re, im*im) per element, float32, one rounding for the product im*im and one for the fused operation"""
    re = np.ascontiguousarray(re, dtype=np.float32)
    im = np.ascontiguousarray(im, dtype=np.float32)
    out = np.empty(re.shape, dtype=np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    if re.size:
        _fma_lib().fpow_p(re.ctypes.data_as(f32p), im.ctypes.data_as(f32p), out.ctypes.data_as(f32p), re.size)
    return out


def values_f32(raw, i16, B):
    """what the stage is fed (interleaved float32, or int16 pairs) as (F, B, 2) float32: int16 * 2^-15 is exact"""
    raw = np.asarray(raw)
    v = raw.astype(np.float32) * np.float32(2.0 ** -15) if i16 else raw.astype(np.float32)
    return v.reshape(-1, B, 2)


def scale_f32(K, G, norm):
    return np.float32(1.0 / (K * G * float(np.float32(norm))))


def power_f64(v, first, G, Bo, K, norm, pos=0):
    """(frames, Bo) float64 P of every output frame the stream v ((F, B, 2) values) completes from position pos with nothing
    carried: the definition, the sums in float64 (norm is used as given: a caller who means the config's fNorm passes the
    float32 value)"""
    v = np.asarray(v, dtype=np.float64)
    r = pos % K
    v = np.concatenate([np.zeros((r,) + v.shape[1:]), v])
    n = v.shape[0] // K
    p = (v[:n * K, first:first + G * Bo, 0] ** 2 + v[:n * K, first:first + G * Bo, 1] ** 2).reshape(n, K, Bo, G)
    return p.sum(axis=(1, 3)) / (K * G * float(norm))


def model_f32(v, first, G, Bo, K, norm, pos=0):
    """the same frames in the float32 order of §19, bit for bit what the GPU gives"""
    v = np.asarray(v, dtype=np.float32)
    r = pos % K
    v = np.concatenate([np.zeros((r,) + v.shape[1:], dtype=np.float32), v])
    n = v.shape[0] // K
    used = v[:n * K, first:first + G * Bo]
    p = element_power_f32(used[..., 0], used[..., 1]).reshape(n * K, Bo, G)
    e = np.zeros((n * K, Bo), dtype=np.float32)
    for g in range(G):
        e = e + p[:, :, g]
    e = e.reshape(n, K, Bo)
    acc = np.zeros((n, Bo), dtype=np.float32)
    for c in range(0, K, CHUNK):
        part = np.zeros((n, Bo), dtype=np.float32)
        for s in range(c, min(c + CHUNK, K)):
            part = part + e[:, s]
        acc = acc + part
    assert acc.dtype == np.float32
    return acc * scale_f32(K, G, norm)


def bound_units(G, K):
    """SPEC §19's bound on the relative error of the float32 order against float64, in units of 2^-24: all terms are
    non-negative, so first-order analysis applies -- 2 for p, G - 1, 7, ceil(K / 8) - 1, 2 for the scale, slack for second order"""
    return G + -(-K // CHUNK) + 12


def special_bins(Bo):
    """output bins of the test signal: (loud: 60 dB above the noise, zero: exactly 0, clamp: 25 dB above the noise); None where
    Bo has no room"""
    loud = Bo // 2 if Bo >= 2 else None
    zero = Bo - 1 if Bo >= 3 else None
    clamp = 1 if Bo >= 5 else None
    return loud, zero, clamp


def make_signal(F, B, first, G, Bo, i16, seed=1):
    """noise in every element, no float32 denormal anywhere (no value below 2^-20 but the exact zeros); the elements of one
    output bin 60 dB above it, of one exactly zero, of one 25 dB above (with REF_POWER its code clamps at 65535).  Returns what
    the context is fed: interleaved float32 (F * B * 2,) or int16."""
    rng = np.random.default_rng(seed + 1000 * B + 7 * G + (1 if i16 else 0))
    x = rng.standard_normal((F, B, 2))
    x = np.where(np.abs(x) < 1e-3, 1e-3, x)
    gain = np.ones(B)
    loud, zero, clamp = special_bins(Bo)
    span = lambda j: slice(first + j * G, first + j * G + G)
    if loud is not None:
        gain[span(loud)] = 1000.0
    if clamp is not None:
        gain[span(clamp)] = 10.0 ** 1.25
    if zero is not None:
        gain[span(zero)] = 0.0
    x = x * gain[None, :, None]
    if i16:
        return np.clip(np.rint(x * 8.0), -32767, 32767).astype(np.int16).reshape(-1)
    return (x * 0.01).astype(np.float32).reshape(-1)


def ref_power_of(i16):
    """fRefPower of the tests: the noise bins read about +5 dB (mid-scale), the bin 25 dB above the noise clamps"""
    noise = 2.0 * (8.0 * 2.0 ** -15) ** 2 if i16 else 2.0 * 0.01 ** 2
    return float(np.float32(noise / NORM / 10.0 ** 0.5))


def chain_stream(N, H, K, frames=3):
    """the stream of the chain tests, interleaved float32: seeded white noise of variance 0.02 per complex sample and one tone
    exactly on bin round(0.1 N) that a Hann window reads 10 dB above the noise; `frames` whole estimator frames, the start of
    one more and an odd remainder"""
    n = (frames * K + 1) * H + N + 17
    rng = np.random.default_rng(19 + N + H + K)
    t = np.arange(n, dtype=np.float64)
    x = 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = x + np.sqrt(0.2 / (2.0 * N / 3.0)) * np.exp(2j * np.pi * round(0.1 * N) / N * t)
    iq = np.empty(2 * n, dtype=np.float32)
    iq[0::2], iq[1::2] = x.real, x.imag
    return iq


CHAIN_REF_POWER = float(np.float32(0.02 / 10.0 ** 0.5))   # the noise reads about +5 dB, the tone about +15 dB: nothing clamps at the top


def chain_align(N, H):
    """(d, q) of SPEC §19's identity: the stream delayed by d = (-(N-1)) mod H zeros, the bank's frame q + s is segment s"""
    d = (-(N - 1)) % H
    return d, (N - 1 + d) // H
