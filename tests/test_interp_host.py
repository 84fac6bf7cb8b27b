"""The interpolator's host side (no GPU): its C ABI in the header and the libraries, the index algebra of the overlap-save
kernel's two forms (tools/fft_model.py) against numpy.fft, the multiply table, and the compiled kernels' resources."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
INTERP_ABI = {"if_fir_interp_init", "if_fir_interp_init_complex", "if_fir_interp_destroy", "if_fir_interp_reset",
              "if_fir_interp_set_backend", "if_fir_interp_get_backend", "if_fir_interp_set_input_format", "if_fir_interp_set_nco",
              "if_fir_interp_get_nco", "if_fir_interp_set_stream", "if_fir_interp_synchronize", "if_fir_interp_last_error",
              "if_fir_interp_out_count", "if_fir_interp_process", "if_fir_interp_process_device"}
INTERP_DEV = {"if_fir_debug_interp_config", "if_fir_debug_interp_seek", "if_fir_debug_interp_tables", "if_fir_debug_interp_plan"}
OVERLAPS = (256, 512, 1024, 2048, 3072)  # docs/SPEC.md §6: the overlap-save kernel's overlaps, in outputs


def _fft_model():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fft_model
    return fft_model


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_declares_and_libraries_export_the_interpolator(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_interp_[a-z_]+)\s*\(", header))
    assert declared == INTERP_ABI, declared ^ INTERP_ABI
    assert "typedef struct if_fir_interp if_fir_interp_t;" in header
    assert INTERP_ABI <= set(fir.EXPORTS) and INTERP_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert INTERP_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert INTERP_ABI <= product and INTERP_ABI <= dev
    assert not (INTERP_DEV & product) and INTERP_DEV <= dev


@pytest.mark.parametrize("L", [1, 2, 4, 8, 16, 32, 64])
def test_model_small_form_is_fft_interpolation(L):
    """tools/fft_model.py's small form (the 4096/L-point Stockham transform read modulo 4096/L, times H, the 4096-point
    inverse), and the full form, against numpy.fft on the zero-stuffed block: zero-stuff, FFT, x H, IFFT; every L | 64 (odd
    log2(4096/L), L = 2, 8, 32, starts with the radix-2 pass)"""
    m = _fft_model()
    rng = np.random.default_rng(L)
    h = rng.standard_normal(255) + 1j * rng.standard_normal(255)
    xb = rng.standard_normal(4096 // L) + 1j * rng.standard_normal(4096 // L)
    u = np.zeros(4096, dtype=np.complex128)
    u[::L] = xb
    ref = np.fft.ifft(np.fft.fft(u) * np.fft.fft(h, 4096))
    scale = np.max(np.abs(ref))
    assert np.max(np.abs(m.interp_block(xb, h, L, small=True) - ref)) <= 1e-12 * scale
    assert np.max(np.abs(m.interp_block(xb, h, L, small=False) - ref)) <= 1e-12 * scale
    assert m.stockham_radices(4096 // L) == [2] * ((12 - (L.bit_length() - 1)) & 1) + [4] * ((12 - (L.bit_length() - 1)) // 2)


def end_weighted_taps(T, seed):
    """complex taps whose first and last are the largest: |h| <= 0.5 inside, h[0] = 1, h[T-1] = -1"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(T) + 1j * rng.standard_normal(T)
    h *= 0.5 / np.max(np.abs(h))
    h[0] = 1.0
    if T > 1:
        h[-1] = -1.0
    return h


@pytest.mark.parametrize("T", [1, 2, 3, 256, 257, 258, 512, 513, 514, 1024, 1025, 1026, 2048, 2049, 2050, 3072, 3073])
def test_model_keep_region_starts_at_the_overlap(T):
    """positions >= overlap (the smallest of 256 .. 3072 that is >= T - 1) of a block are the LINEAR convolution of the
    zero-stuffed block; when T - 1 = overlap the position before them that meets a wrapped input sample is not: overlap - 1
    for L = 1, overlap - L in general (positions 4096 - L + 1 .. 4095 of a zero-stuffed block are zero).  Taps with the
    largest weight at both ends: a boundary off by one costs O(1), not the 1e-6 of a windowed design's end taps."""
    m = _fft_model()
    ovl = min(o for o in OVERLAPS if o >= T - 1)
    h = end_weighted_taps(T, T)
    rng = np.random.default_rng(1000 + T)
    for L, small in ((1, False), (4, True)) + (((32, True),) if T - 1 == ovl else ()):
        xb = rng.standard_normal(4096 // L) + 1j * rng.standard_normal(4096 // L)
        u = np.zeros(4096, dtype=np.complex128)
        u[::L] = xb
        lin = np.convolve(u, h)[:4096]
        got = m.interp_block(xb, h, L, small=small)
        scale = np.max(np.abs(lin))
        assert np.max(np.abs(got[ovl:] - lin[ovl:])) <= 1e-12 * scale, (T, L)
        if T - 1 == ovl:
            assert abs(got[ovl - L] - lin[ovl - L]) >= 0.1 * abs(xb[-1]), (T, L)   # h[T-1] x (the block's last sample) wrapped in
            if T >= 2 + L:
                assert np.max(np.abs(got[T - 1 - L + 1:] - lin[T - 1 - L + 1:])) <= 1e-12 * scale, (T, L)


def test_plan_query_against_the_definitions(fir):
    """if_fir_debug_interp_plan (what interp_overlap_rows, interp_hist_len and interp_fft_supported decide) for every tap count
    and every interpolation, against the one-line definitions of docs/SPEC.md §6 and include/if_fir.h: 64 rows = the smallest
    overlap >= T - 1 (the largest beyond the overlap-save range); hist_len = the fewest input samples with
    hist_len L >= max(overlap, T - 1) (overlap-save range) or >= T - 1 (beyond it); overlap-save serves L | 64, T <= 3073"""
    for T in range(1, 4097):
        fits = [o for o in OVERLAPS if o >= T - 1]
        ovl = fits[0] if fits else OVERLAPS[-1]
        for L in range(1, 65):
            rows, hist, ok = fir.debug_interp_plan(T, L)
            assert rows * 64 == ovl, (T, L, rows)
            need = max(ovl, T - 1) if fits else T - 1
            assert hist * L >= need > (hist - 1) * L, (T, L, hist)
            assert ok == (bool(fits) and 64 % L == 0), (T, L, ok)
    for T, L in ((0, 1), (4097, 1), (255, 0), (255, 65)):
        with pytest.raises(fir.IfFirError):
            fir.debug_interp_plan(T, L)


@pytest.mark.parametrize("complex_taps", [False, True])
def test_host_multiply_table(fir, complex_taps):
    rng = np.random.default_rng(7)
    T = 1023
    if complex_taps:
        t = rng.standard_normal(2 * T).astype(np.float32)
        h = t[0::2].astype(np.float64) + 1j * t[1::2].astype(np.float64)
    else:
        t = rng.standard_normal(T).astype(np.float32)
        h = t.astype(np.float64)
    got = fir.debug_interp_tables(t, complex_taps)
    want = np.fft.fft(h, 4096) / 4096
    assert np.max(np.abs(got - want)) <= 1e-6 * np.max(np.abs(want))
    with pytest.raises(fir.IfFirError):
        fir.debug_interp_tables(np.ones(3074, dtype=np.float32))


def test_interp_kernels_do_not_spill():
    path = os.path.join(CSRC, "if_fir_interp.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_interp_r*.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # 5 overlap lengths x (int16, NCO, small form) = 40 instantiations
    assert len(names) == 40 and all("fir_interp_kernel" in n for n in names), names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 40
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 40


def test_interp_kernels_read_lds_without_pairing():
    """every fir_interp_kernel form reads LDS with single ds_read_b64 / ds_read_b32: no ds_read2 pairs (the single-read attribute)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_tools
    for r in (4, 8, 16, 32, 48):
        obj = os.path.join(CSRC, "if_fir_interp_r%d.o" % r)
        assert os.path.exists(obj), obj
        text = isa_tools.disassemble(obj)
        reads = re.findall(r"\b(ds_read\w*)", text)
        assert reads.count("ds_read_b64") > 0, r
        assert not [x for x in reads if x.startswith("ds_read2") or x == "ds_read_b128"], (r, sorted(set(reads)))
