"""The real-input down-converter's host side (no GPU): its C ABI in the header, the libraries and the binding; the tile shape,
the tap table and the call plan of qo-100-tools_amd/csrc/if_fir_ddc_plan.h through the stand-alone checker
tests/c/ddc_plan_check.cpp (built with the address and undefined-behaviour sanitizers); the float64 reference of
tests/ddc_ref.py against the decimator's oracle and scipy; the float32 model of SPEC §10's order; the compiled kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import ddc_ref
from matrix_util import TOL, row_edge_taps
from test_ddc_gpu import LOUD_MATRIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
DDC_ABI = {"if_fir_ddc_init", "if_fir_ddc_init_complex", "if_fir_ddc_destroy", "if_fir_ddc_reset", "if_fir_ddc_set_input_format",
           "if_fir_ddc_set_nco", "if_fir_ddc_get_nco", "if_fir_ddc_set_stream", "if_fir_ddc_synchronize", "if_fir_ddc_last_error",
           "if_fir_ddc_out_count", "if_fir_ddc_process", "if_fir_ddc_process_device"}
DDC_DEV = {"if_fir_debug_ddc_config"}


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ddc_plan_check") / "ddc_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "c", "ddc_plan_check.cpp"), "-o", exe])
    return exe


def ask(plan_check, *args):
    run = subprocess.run([plan_check] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    return run.stdout


def test_header_declares_and_libraries_export_the_down_converter(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_ddc_[a-z_]+)\s*\(", header))
    assert declared == DDC_ABI, declared ^ DDC_ABI
    assert "typedef struct if_fir_ddc if_fir_ddc_t;" in header
    assert DDC_ABI <= set(fir.EXPORTS) and DDC_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert DDC_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert DDC_ABI <= product and DDC_ABI <= dev
    assert not (DDC_DEV & product) and DDC_DEV <= dev
    for name in ("process", "process_device", "out_count", "reset", "set_input_format", "set_stream", "set_nco", "get_nco",
                 "debug_config", "tile_outputs", "__enter__", "__exit__"):
        assert hasattr(fir.IfFirDdc, name), name


def test_null_context_and_init_refusals_without_a_device(fir):
    """what answers before the device is asked for, in both libraries"""
    import ctypes
    taps = np.ones(4097, dtype=np.float32)
    for L in (fir.lib(), fir.dev_lib()):
        for name in ("reset", "synchronize"):
            assert getattr(L, "if_fir_ddc_" + name)(None) == 0
        assert L.if_fir_ddc_set_stream(None, None) == 0 and L.if_fir_ddc_set_input_format(None, 0) == 0
        assert L.if_fir_ddc_set_nco(None, 0.1) == 0 and L.if_fir_ddc_out_count(None, 1000) == 0
        for T, D, n, message in ((0, 4, 1024, "taps must be 1..4096 (got 0)"), (4097, 4, 1024, "taps must be 1..4096 (got 4097)"),
                                 (31, 0, 1024, "decimation must be 1..64 (got 0)"), (31, 65, 1024, "decimation must be 1..64 (got 65)"),
                                 (31, 4, 0, "ullMaxSamples must be 1..2^40 (got 0)")):
            ctx = ctypes.c_void_p()
            assert L.if_fir_ddc_init(ctypes.byref(ctx), taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), T, D, n, 0) == 0
            assert not ctx.value and L.if_fir_ddc_last_error(None).decode() == "if_fir_ddc_init: " + message


def test_plan_of_every_shape_and_stream_position(plan_check):
    """every D in 1..64 with T at the row and segment edges, stream positions around 2^32 and at 2^63 (the checker's header
    comment lists the properties), under the address and undefined-behaviour sanitizers"""
    out = ask(plan_check)
    assert out.strip().endswith("calls checked: OK"), out
    shapes = sum(1 for D in range(1, 65) for T in (1, D - 1, D, D + 1, 4 * D, 4 * D + 1, 16 * D, 16 * D + 1, 17 * D, 255, 1023, 4095, 4096)
                 if 1 <= T <= 4096)
    assert out.startswith("%d shapes, %d calls" % (shapes, shapes * 15 * 7)), out


def test_tile_shape_and_call_plan_are_the_python_restatement(plan_check):
    """ddc_ref.tile_shape and ddc_ref.out_count, from which the GPU tests size their streams, cuts and counts, against the header"""
    for T, D in LOUD_MATRIX + tuple((t, d) for d in (1, 2, 5, 16, 31, 32, 33, 63, 64) for t in (1, 17, 255, 1023, 4096)):
        K, G, tile_out, tile_in, cols, RS = (int(v) for v in ask(plan_check, "shape", T, D).split())
        assert (K, tile_out, tile_in) == ddc_ref.tile_shape(T, D), (T, D)
        n = ddc_ref.stream_len(T, D)
        outs = ddc_ref.out_count(0, n, D)
        assert outs > 3 * tile_out and outs % tile_out and n >= 2 * T + 17 and n <= 1 << 17, (T, D)
    for D in (1, 3, 64):
        for c in (0, 1, D - 1, (1 << 32) - 3, (1 << 32) - 1, 1 << 32, (1 << 32) + 2, (1 << 40) + 3, 1 << 63, (1 << 64) - 1001):
            for n in (0, 1, D - 1, D, D + 1, 1000):
                n0, count, first = (int(v) for v in ask(plan_check, "call", c, n, D).split())
                assert count == ddc_ref.out_count(c, n, D) and n0 == (-c) % D and (not count or first == c + n0), (c, n, D)
    assert ask(plan_check, "call", (1 << 64) - 5, 10, 3).strip() == "refused"


@pytest.mark.parametrize("T,D", [(24, 7), (3, 7), (7, 7), (5, 1), (4096, 64), (1, 5), (65, 4), (17, 1)])
def test_tap_table_is_phase_major(plan_check, T, D):
    """row R of the table holds the phase rho = D - 1 - R, its taps rho + j D with j descending (oldest sample first), zeros
    where rho + j D >= T and in the padding up to K: T < D (phases without a tap), T = D, T not a multiple of D"""
    K = ddc_ref.row_taps(T, D)
    got = np.array([[float(v) for v in row.split()] for row in ask(plan_check, "table", T, D).strip().splitlines()])
    assert got.shape == (D, 2 * K)
    want = np.zeros((D, K))
    for R in range(D):
        for e in range(K):
            k = (D - 1 - R) + (K - 1 - e) * D
            want[R, e] = k + 1 if k < T else 0.0
    assert np.array_equal(got[:, 0::2], want) and np.array_equal(got[:, 1::2], -want)
    # the order model walks the same taps in the same order
    flat = [k if k < T else None for seg in ddc_ref.segments(T, D) for k in seg]
    assert flat == [int(v) - 1 if v else None for v in want.reshape(-1)]
    assert all(len(seg) <= 16 and len(seg) % 4 == 0 for seg in ddc_ref.segments(T, D))


@pytest.mark.parametrize("word", [0, ddc_ref.phase_word(0.2), ddc_ref.phase_word(-0.37000001), ddc_ref.phase_word(1 / 4096), 1, (1 << 32) - 1])
def test_mixed_taps_are_rounded_once(plan_check, word):
    """g[k] = h[k] e^{+j theta k} with the exact phase (P k) mod 2^32: each component within half a float32 ulp (and the
    rounding of float64 cos / sin) of the float64 product, for real and for complex taps; P = 0 leaves the taps as they are"""
    T = 4096
    got = np.array([[float.fromhex(v) for v in line.split()] for line in ask(plan_check, "mix", T, word).strip().splitlines()])
    h = ((np.arange(T) + 1).astype(np.float32) / np.float32(T)).astype(np.float32)
    hc = np.stack([h, np.float32(-0.5) * h], axis=1).reshape(-1)
    for cols, taps, ct in ((got[:, 0:2], h, False), (got[:, 2:4], hc, True)):
        g = ddc_ref.taps_c(taps, ct)
        k = np.arange(T, dtype=np.uint64)
        g = g * np.exp(2j * np.pi * (((k * np.uint64(word)) & np.uint64(0xffffffff)).astype(np.float64) / 2 ** 32))
        for comp, want in ((cols[:, 0], g.real), (cols[:, 1], g.imag)):
            assert np.array_equal(comp, comp.astype(np.float32))
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(comp - want) <= 0.5 * ulp * (1 + 1e-6) + 1e-16), word
        if word == 0:
            assert np.array_equal(cols[:, 0], ddc_ref.taps_c(taps, ct).real) and np.array_equal(cols[:, 1], ddc_ref.taps_c(taps, ct).imag)
        wr, wi = ddc_ref.mixed_taps(taps, word, ct)
        assert np.max(np.abs(cols[:, 0] - wr)) <= 1.2e-7 and np.max(np.abs(cols[:, 1] - wi)) <= 1.2e-7


def test_reference_is_the_definition(oracle):
    """tests/ddc_ref.py equals the decimator's float64 oracle with an NCO fed (r, 0) -- SPEC §10 is §2 plus §3.2 on such a
    stream -- and, with the NCO off, scipy.signal.upfirdn(h, r, down=D); a stream that starts at an absolute index c equals
    the tail of the stream from 0 whose first c samples are zero"""
    from scipy.signal import upfirdn
    rng = np.random.default_rng(11)
    for T, D, n in ((31, 1, 300), (31, 4, 301), (255, 16, 5000), (7, 64, 1000), (100, 3, 997), (1, 5, 50)):
        r = rng.standard_normal(n).astype(np.float32)
        iq = np.stack([r, np.zeros(n, np.float32)], axis=1).reshape(-1)
        for ct in (False, True):
            taps = rng.standard_normal(T * (2 if ct else 1)).astype(np.float32)
            for f in (0.0, 0.2, -0.37000001, 0.4999, 1 / 4096):
                word = ddc_ref.phase_word(f)
                got = ddc_ref.ddc_f64(taps, r, D, word, ct)
                want = oracle.fir_nco_f64(taps, iq, D, word, complex_taps=ct)
                assert got.size == want.size == 2 * ddc_ref.out_count(0, n, D)
                assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (T, D, ct, f)
            got = ddc_ref.as_c(ddc_ref.ddc_f64(taps, r, D, 0, ct))
            want = upfirdn(ddc_ref.taps_c(taps, ct), r.astype(np.float64), down=D)[:got.size]
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (T, D, ct)
            c, word = 1003, ddc_ref.phase_word(0.2)
            whole = ddc_ref.ddc_f64(taps, np.concatenate([np.zeros(c, np.float32), r]), D, word, ct)
            tail = ddc_ref.ddc_f64(taps, r, D, word, ct, first=c)
            assert np.max(np.abs(tail - whole[2 * ddc_ref.out_count(0, c, D):])) <= 1e-12 * np.max(np.abs(whole))


def max_metric(y, ref):
    return np.max(np.abs(y - ref)) / np.max(np.abs(ref))


def row_end_costs(taps, r, D, word, ct, ref):
    """{(rho, which end): SPEC §3's max metric of leaving that tap out} for every phase row's first tap h[rho] and its last one
    h[rho + ((T-1-rho)//D) D]: without tap k the output m loses h[k] x'[m D - k]"""
    h = ddc_ref.taps_c(taps, ct)
    T, n = h.size, r.size
    x = r.astype(np.float64) * np.exp(-2j * np.pi * ((np.arange(n) * word) % (1 << 32)) / 2 ** 32)
    peak = np.max(np.abs(ref))
    costs = {}
    for rho in range(min(D, T)):
        for end, k in (("first", rho), ("last", rho + ((T - 1 - rho) // D) * D)):
            at = np.arange(0, n, D) - k
            lost = h[k] * x[at[at >= 0]]
            costs[rho, end] = max(np.max(np.abs(lost.real)), np.max(np.abs(lost.imag))) / peak
    return costs


@pytest.mark.parametrize("D", [1, 3, 4, 8, 16, 64])
def test_order_model_meets_the_bound_and_a_dropped_row_end_is_loud(oracle, D):
    """What tests/test_ddc_gpu.py rests on, at T = 4096 with row_edge_taps(T, D, ct), real and complex, float32 and full-scale
    int16 streams, a frequency off every grid: the float32 model of SPEC §10's order stays within 1e-6 of float64 in both
    metrics (the arithmetic can deliver what the GPU matrix asks), and leaving out the first or the last tap of any phase row
    moves the float64 reference by more than 1e-2, so that matrix sees such a bug.  The model with one such tap dropped is
    held to the same: it misses the bound by four orders."""
    T, word = 4096, ddc_ref.phase_word(-0.37000001)
    n = ddc_ref.stream_len(T, D)
    for ct in (False, True):
        taps = row_edge_taps(T, D, ct)
        for i16 in (False, True):
            r = ddc_ref.real_signal(oracle, n, i16)[1]
            ref = ddc_ref.ddc_f64(taps, r, D, word, ct)
            l2, mx = oracle.err_metrics(ddc_ref.ddc_f32_order(taps, r, D, word, ct), ref)
            print("model D=%d complex=%d i16=%d: l2=%.3g max=%.3g" % (D, ct, i16, l2, mx))
            assert l2 <= TOL and mx <= TOL, (D, ct, i16, l2, mx)
            costs = row_end_costs(taps, r, D, word, ct, ref)
            assert len(costs) == 2 * D and min(costs.values()) > 1e-2, (D, ct, i16, min(costs.items(), key=lambda kv: kv[1]))
    k = (D - 1) + ((T - 1 - (D - 1)) // D) * D   # (the last case: complex taps, int16)
    assert max_metric(ddc_ref.ddc_f32_order(taps, r, D, word, ct, drop=k), ref) > 1e-2


def test_ddc_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_ddc.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_ddc.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # float32 and int16 input
    assert len(names) == 2 and all("fir_ddc_kernel" in n for n in names), names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
