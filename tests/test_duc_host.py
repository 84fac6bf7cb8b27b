"""The real-output up-converter's host side (no GPU): its C ABI in the header, the libraries and the binding; the tile shape,
the tap table and the call plan of qo-100-tools_amd/csrc/if_fir_duc_plan.h through the stand-alone checker
tests/c/duc_plan_check.cpp (built with the address and undefined-behaviour sanitizers); the float64 reference of
tests/duc_ref.py against the interpolator's oracle path and scipy; the float32 model of SPEC §11's order; the int16 rule; the
compiled kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import duc_ref
from matrix_util import TOL, row_edge_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
DUC_ABI = {"if_fir_duc_init", "if_fir_duc_init_complex", "if_fir_duc_destroy", "if_fir_duc_reset", "if_fir_duc_set_input_format",
           "if_fir_duc_set_output_format", "if_fir_duc_set_nco", "if_fir_duc_get_nco", "if_fir_duc_set_stream", "if_fir_duc_synchronize",
           "if_fir_duc_last_error", "if_fir_duc_out_count", "if_fir_duc_process", "if_fir_duc_process_device"}
DUC_DEV = {"if_fir_debug_duc_config"}
# the (T, L) rows of tests/test_duc_gpu.py's matrix
MATRIX = ((1, 1), (5, 1), (17, 1), (3, 7), (24, 7), (255, 3), (255, 4), (1023, 8), (63, 64), (64, 64), (65, 64), (1537, 63), (4096, 64),
          (4096, 1))


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("duc_plan_check") / "duc_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "c", "duc_plan_check.cpp"), "-o", exe])
    return exe


def ask(plan_check, *args):
    run = subprocess.run([plan_check] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    return run.stdout


def test_header_declares_and_libraries_export_the_up_converter(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_duc_[a-z_]+)\s*\(", header))
    assert declared == DUC_ABI, declared ^ DUC_ABI
    assert "typedef struct if_fir_duc if_fir_duc_t;" in header
    assert re.search(r"IF_FIR_OUTPUT_F32 = 0,", header) and re.search(r"IF_FIR_OUTPUT_I16 = 1\b", header)
    assert (fir.OUTPUT_F32, fir.OUTPUT_I16) == (0, 1)
    assert DUC_ABI <= set(fir.EXPORTS) and DUC_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert DUC_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert DUC_ABI <= product and DUC_ABI <= dev
    assert not (DUC_DEV & product) and DUC_DEV <= dev
    for name in ("process", "process_device", "out_count", "reset", "set_input_format", "set_output_format", "set_stream", "set_nco",
                 "get_nco", "debug_config", "tile_inputs", "__enter__", "__exit__"):
        assert hasattr(fir.IfFirDuc, name), name


def test_null_context_and_init_refusals_without_a_device(fir):
    """what answers before the device is asked for, in both libraries"""
    import ctypes
    taps = np.ones(4097, dtype=np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    for L in (fir.lib(), fir.dev_lib()):
        for name in ("reset", "synchronize"):
            assert getattr(L, "if_fir_duc_" + name)(None) == 0
        assert L.if_fir_duc_set_stream(None, None) == 0 and L.if_fir_duc_set_input_format(None, 0) == 0
        assert L.if_fir_duc_set_output_format(None, 0) == 0
        assert L.if_fir_duc_set_nco(None, 0.1) == 0 and L.if_fir_duc_out_count(None, 1000) == 0
        assert L.if_fir_duc_process(None, None, None, 0, None) == 0 and L.if_fir_duc_process_device(None, None, None, 0, None) == 0
        for T, up, n, message in ((0, 4, 1024, "taps must be 1..4096 (got 0)"), (4097, 4, 1024, "taps must be 1..4096 (got 4097)"),
                                  (31, 0, 1024, "interpolation must be 1..64 (got 0)"), (31, 65, 1024, "interpolation must be 1..64 (got 65)"),
                                  (31, 4, 0, "ullMaxSamples must be 1..2^40 (got 0)")):
            for init in (L.if_fir_duc_init, L.if_fir_duc_init_complex):
                ctx = ctypes.c_void_p()
                assert init(ctypes.byref(ctx), taps.ctypes.data_as(f32p), T, up, n, 0) == 0
                assert not ctx.value and L.if_fir_duc_last_error(None).decode() == "if_fir_duc_init: " + message
        for bad in (np.nan, np.inf, -np.inf):
            h = np.ones(31, dtype=np.float32)
            h[7] = bad
            ctx = ctypes.c_void_p()
            assert L.if_fir_duc_init(ctypes.byref(ctx), h.ctypes.data_as(f32p), 31, 4, 1024, 0) == 0
            assert not ctx.value and L.if_fir_duc_last_error(None).decode() == "if_fir_duc_init: tap 7 is not finite"


def test_plan_of_every_shape_and_stream_position(plan_check):
    """every L in 1..64 with T at the row and segment edges, stream positions around 2^32 and near 2^64 / L (the checker's
    header comment lists the properties), under the address and undefined-behaviour sanitizers"""
    out = ask(plan_check)
    assert out.strip().endswith("calls checked: OK"), out
    shapes = sum(1 for L in range(1, 65)
                 for T in (1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 15 * L, 16 * L, 16 * L + 1, 17 * L, 33 * L, 255, 1023, 4095, 4096)
                 if 1 <= T <= 4096)
    assert out.startswith("%d shapes, %d calls" % (shapes, shapes * 12 * 5)), out


def test_tile_shape_and_call_plan_are_the_python_restatement(plan_check):
    """duc_ref.tile_shape, from which the GPU tests size their streams and cuts, against the header; the LDS of every shape
    leaves room for at least two workgroups on a CU"""
    for T, L in MATRIX + tuple((t, up) for up in (1, 2, 5, 16, 17, 31, 32, 33, 63, 64) for t in (1, 17, 255, 1023, 4096)):
        K, KP, top, Q, tile_out, RS, lds, per_cu = (int(v) for v in ask(plan_check, "shape", T, L).split())
        assert (K, KP, Q) == duc_ref.tile_shape(T, L), (T, L)
        assert tile_out == Q * L and lds <= 80 * 1024 and per_cu >= 2, (T, L, lds)
        assert top + 16 * ((KP - top) // 16) == KP and len(duc_ref.segments(T, L, 0)[0]) == top - (KP - K)
        n = duc_ref.stream_len(T, L)
        assert n > 3 * Q and n % Q and n >= 2 * K + 17 and n * L <= 1 << 18, (T, L)
    for L in (1, 3, 64):
        limit = ((1 << 64) - 1) // L
        for c in (0, 1, (1 << 32) - 3, 1 << 32, (1 << 40) + 3, limit - 1000, limit):
            for n in (0, 1, L, 1000):
                got = ask(plan_check, "call", c, n, L).strip()
                assert got == (str(n * L) if c + n <= limit else "refused"), (c, n, L)
    assert ask(plan_check, "call", (1 << 64) - 5, 10, 1).strip() == "refused"


@pytest.mark.parametrize("T,L", [(24, 7), (3, 7), (7, 7), (5, 1), (4096, 64), (1, 5), (65, 4), (17, 1), (33, 2)])
def test_tap_table_is_phase_major(plan_check, T, L):
    """row p of the table holds the phase p, its taps p + j L with j descending (oldest sample first) as (g_r, -g_i) -- the
    checker feeds g = (k + 1, -(k + 1)) -- zeros where p + j L >= T and in the pad entry in front of an odd K: T < L (phases
    without a tap), T = L, T not a multiple of L"""
    K, KP, _ = duc_ref.tile_shape(T, L)
    got = np.array([[float(v) for v in row.split()] for row in ask(plan_check, "table", T, L).strip().splitlines()])
    assert got.shape == (L, 2 * KP)
    want = np.zeros((L, KP))
    for p in range(L):
        for e in range(KP):
            k = p + (KP - 1 - e) * L
            want[p, e] = k + 1 if k < T else 0.0
    assert np.array_equal(got[:, 0::2], want) and np.array_equal(got[:, 1::2], -want)
    # the order model walks the same taps in the same order, in segments of at most 16
    for p in range(L):
        flat = [k if k < T else None for seg in duc_ref.segments(T, L, p) for k in seg]
        assert flat == [int(v) - 1 if v else None for v in want[p, KP - K:]]
        assert all(1 <= len(seg) <= 16 for seg in duc_ref.segments(T, L, p))
        assert all(len(seg) == 16 for seg in duc_ref.segments(T, L, p)[1:])


@pytest.mark.parametrize("word", [0, duc_ref.phase_word(0.2), duc_ref.phase_word(-0.37000001), duc_ref.phase_word(1 / 4096), 1, (1 << 32) - 1])
def test_mixed_taps_are_rounded_once(plan_check, word):
    """g[k] = h[k] e^{+j theta k} with the exact phase (P k) mod 2^32, stored as (g_r, -g_i): each component within half a
    float32 ulp (and the rounding of float64 cos / sin) of the float64 product, for real and for complex taps; P = 0 leaves the
    taps as they are"""
    T = 4096
    got = np.array([[float.fromhex(v) for v in line.split()] for line in ask(plan_check, "mix", T, word).strip().splitlines()])
    h = ((np.arange(T) + 1).astype(np.float32) / np.float32(T)).astype(np.float32)
    hc = np.stack([h, np.float32(-0.5) * h], axis=1).reshape(-1)
    for cols, taps, ct in ((got[:, 0:2], h, False), (got[:, 2:4], hc, True)):
        g = duc_ref.taps_c(taps, ct)
        k = np.arange(T, dtype=np.uint64)
        g = g * np.exp(2j * np.pi * (((k * np.uint64(word)) & np.uint64(0xffffffff)).astype(np.float64) / 2 ** 32))
        for comp, want in ((cols[:, 0], g.real), (cols[:, 1], -g.imag)):
            assert np.array_equal(comp, comp.astype(np.float32))
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(comp - want) <= 0.5 * ulp * (1 + 1e-6) + 1e-16), word
        if word == 0:
            assert np.array_equal(cols[:, 0], duc_ref.taps_c(taps, ct).real) and np.array_equal(cols[:, 1], -duc_ref.taps_c(taps, ct).imag)
        wr, wi = duc_ref.mixed_taps(taps, word, ct)
        assert np.max(np.abs(cols[:, 0] - wr)) <= 1.2e-7 and np.max(np.abs(cols[:, 1] - wi)) <= 1.2e-7


def chain_f64(oracle, taps, x_iq, L, word, ct):
    """SPEC §6 by the decimator's oracle, then the real part: the zero-stuffed stream through oracle.fir_f64 / fir_ctaps_f64 at
    decimation 1, every output times exp(+j 2 pi ((P m) mod 2^32) / 2^32) in float64"""
    n = len(x_iq) // 2
    u = np.zeros((n * L, 2), dtype=np.float32)
    u[::L] = np.asarray(x_iq, dtype=np.float32).reshape(-1, 2)
    v = duc_ref.as_c((oracle.fir_ctaps_f64 if ct else oracle.fir_f64)(taps, u.reshape(-1), 1))
    m = np.arange(n * L, dtype=np.uint64)
    return (v * np.exp(2j * np.pi * (((m * np.uint64(word)) & np.uint64(0xffffffff)).astype(np.float64) / 2 ** 32))).real


def test_reference_is_the_definition(oracle):
    """tests/duc_ref.py equals SPEC §6 evaluated by the float64 oracle followed by the real part and, with the NCO off and real
    taps, scipy.signal.upfirdn(h, x, up=L)[:N L].real; a stream that starts at an absolute input index c equals the tail of
    the stream from 0 whose first c samples are zero"""
    from scipy.signal import upfirdn
    rng = np.random.default_rng(11)
    for T, L, n in ((31, 1, 300), (31, 4, 301), (255, 16, 700), (7, 64, 100), (100, 3, 997), (1, 5, 50), (3, 7, 40)):
        x = rng.standard_normal(2 * n).astype(np.float32)
        for ct in (False, True):
            taps = rng.standard_normal(T * (2 if ct else 1)).astype(np.float32)
            for f in (0.0, 0.2, -0.37000001, 0.4999, 1 / 4096):
                word = duc_ref.phase_word(f)
                got = duc_ref.duc_f64(taps, x, L, word, ct)
                want = chain_f64(oracle, taps, x, L, word, ct)
                assert got.size == want.size == n * L
                assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (T, L, ct, f)
            if not ct:
                got = duc_ref.duc_f64(taps, x, L, 0, ct)
                want = np.zeros(n * L)
                full = upfirdn(taps.astype(np.float64), duc_ref.as_c(x), up=L)[:n * L].real   # (upfirdn stops early when T < L)
                want[:full.size] = full
                assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (T, L)
            c, word = 1003, duc_ref.phase_word(0.2)
            whole = duc_ref.duc_f64(taps, np.concatenate([np.zeros(2 * c, np.float32), x]), L, word, ct)
            tail = duc_ref.duc_f64(taps, x, L, word, ct, first=c)
            assert np.max(np.abs(tail - whole[c * L:])) <= 1e-12 * np.max(np.abs(whole))


def max_metric(y, ref):
    return np.max(np.abs(y - ref)) / np.max(np.abs(ref))


def row_end_costs(taps, x_iq, L, word, ct, ref):
    """{(p, which end): SPEC §3's max metric of leaving that tap out} for every reached phase row's first tap h[p] and its last
    one h[p + ((T-1-p)//L) L]: without tap k = p + j L the output q L + p loses Re{e^{j theta (q L + p)} h[k] x[q - j]}"""
    h = duc_ref.taps_c(taps, ct)
    x = duc_ref.as_c(x_iq)
    T, n = h.size, x.size
    peak = np.max(np.abs(ref))
    costs = {}
    for p in range(min(L, T)):
        for end, k in (("first", p), ("last", p + ((T - 1 - p) // L) * L)):
            j = k // L
            q = np.arange(j, n)
            ph = ((q * L + p) * word) % (1 << 32)
            lost = (np.exp(2j * np.pi * ph / 2 ** 32) * h[k] * x[q - j]).real
            costs[p, end] = np.max(np.abs(lost)) / peak
    return costs


@pytest.mark.parametrize("L", [1, 3, 4, 8, 16, 64])
def test_order_model_meets_the_bound_and_a_dropped_row_end_is_loud(oracle, L):
    """What tests/test_duc_gpu.py rests on, at T = 4096 with row_edge_taps(T, L, ct), real and complex, float32 and full-scale
    int16 streams, a frequency off every grid: the float32 model of SPEC §11's order stays within 1e-6 of float64 in both
    metrics (the arithmetic can deliver what the GPU matrix asks), and leaving out the first or the last tap of any phase row
    moves the float64 reference by more than 1e-2, so that matrix sees such a bug.  The model with one such tap dropped is
    held to the same: it misses the bound by four orders."""
    T, word = 4096, duc_ref.phase_word(-0.37000001)
    n = duc_ref.stream_len(T, L)
    for ct in (False, True):
        taps = row_edge_taps(T, L, ct)
        for i16 in (False, True):
            x = duc_ref.signal(oracle, n, i16)[1]
            ref = duc_ref.duc_f64(taps, x, L, word, ct)
            l2, mx = duc_ref.metrics(duc_ref.duc_f32_order(taps, x, L, word, ct), ref)
            print("model L=%d complex=%d i16=%d: l2=%.3g max=%.3g" % (L, ct, i16, l2, mx))
            assert l2 <= TOL and mx <= TOL, (L, ct, i16, l2, mx)
            costs = row_end_costs(taps, x, L, word, ct, ref)
            assert len(costs) == 2 * L and min(costs.values()) > 1e-2, (L, ct, i16, min(costs.items(), key=lambda kv: kv[1]))
    k = (L - 1) + ((T - 1 - (L - 1)) // L) * L   # (the last case: complex taps, int16)
    assert max_metric(duc_ref.duc_f32_order(taps, x, L, word, ct, drop=k), ref) > 1e-2


def test_int16_rule_is_clip_of_rint(plan_check):
    """duc_to_i16, which the kernel calls, against numpy's clip(rint(v 2^15)): ties go to the even code, +1.0 saturates to 32767,
    -1.0 is -32768 exactly, values beyond full scale stay at the rails"""
    vs = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 32766.5, 32767.5, -32767.5, -32768.5, 32767, -32768, 40000, -40000, 1e9, -1e9,
                   0.49999, -0.49999, 12345.5, -12344.5, 0.0], dtype=np.float32) / np.float32(32768)
    rng = np.random.default_rng(5)
    vs = np.concatenate([vs, rng.uniform(-1.2, 1.2, 400).astype(np.float32), ((rng.integers(-32768, 32767, 200) + 0.5) / 32768).astype(np.float32)])
    got = np.array([int(v) for v in ask(plan_check, "i16", *[float(v).hex() for v in vs]).split()])
    want = duc_ref.to_i16(vs)
    assert np.array_equal(got, want)
    assert want[0] == 0 and want[1] == 2 and want[2] == 2 and want[7] == 32766 and want[8] == 32767 and want[10] == -32768
    assert want.min() == -32768 and want.max() == 32767


def test_duc_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_duc.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_duc.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # float32 and int16 input x float32 and int16 output
    assert len(names) == 4 and len(set(names)) == 4 and all("fir_duc_kernel" in n for n in names), names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 4
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 4
