"""The rational resampler's host side (no GPU): its C ABI in the header, the libraries and the binding; the call planning
and the tap table of qo-100-tools_amd/csrc/if_fir_resamp_plan.h through the stand-alone checker tests/c/resamp_plan_check.cpp;
the float64 reference of tests/resamp_ref.py against a direct evaluation of the definition; the compiled kernels' resources."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import resamp_ref
from matrix_util import TOL, row_edge_taps, signal
from test_resamp_gpu import LOUD_MATRIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
RESAMP_ABI = {"if_fir_resamp_init", "if_fir_resamp_init_complex", "if_fir_resamp_destroy", "if_fir_resamp_reset",
              "if_fir_resamp_set_input_format", "if_fir_resamp_set_stream", "if_fir_resamp_synchronize", "if_fir_resamp_last_error",
              "if_fir_resamp_out_count", "if_fir_resamp_process", "if_fir_resamp_process_device"}
RESAMP_DEV = {"if_fir_debug_resamp_config"}


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resamp_plan_check") / "resamp_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "c", "resamp_plan_check.cpp"), "-o", exe])
    return exe


def test_header_declares_and_libraries_export_the_resampler(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_resamp_[a-z_]+)\s*\(", header))
    assert declared == RESAMP_ABI, declared ^ RESAMP_ABI
    assert "typedef struct if_fir_resamp if_fir_resamp_t;" in header
    assert RESAMP_ABI <= set(fir.EXPORTS) and RESAMP_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert RESAMP_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert RESAMP_ABI <= product and RESAMP_ABI <= dev
    assert not (RESAMP_DEV & product) and RESAMP_DEV <= dev
    for name in ("process", "process_device", "out_count", "reset", "set_input_format", "set_stream", "__enter__", "__exit__"):
        assert hasattr(fir.IfFirResamp, name), name


def test_plan_of_every_ratio_and_stream_position(plan_check):
    """every (L, M) in 1..64 x 1..64, T in {1, L-1, L, L+1, 255, 4096}, stream positions up to 2^40 + 7: count, t0, the period
    table, tap and input indices, tile windows (the checker's header comment lists the properties)"""
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("calls checked: OK"), run.stdout + run.stderr
    shapes = 64 * 5 + 63 * 64 * 6   # T = L - 1 = 0 is no filter
    assert run.stdout.startswith("%d shapes, %d calls" % (shapes, shapes * 36)), run.stdout


@pytest.mark.parametrize("L,T", [(7, 3), (7, 7), (7, 24), (1, 5), (64, 4096), (5, 1)])
def test_tap_table_is_phase_major(plan_check, L, T):
    """the table read back through the plan header's builder equals h[p + j L] exactly, zeros elsewhere: T < L (phases
    without a tap), T = L, T not a multiple of L"""
    run = subprocess.run([plan_check, "table", str(L), str(T)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    K, KP = (int(v) for v in lines[0].split())
    assert K == -(-T // L) and KP >= K and KP % 2 == 1
    got = np.array([[float(v) for v in row.split()] for row in lines[1:]])
    assert got.shape == (L, KP)
    h = np.arange(1, T + 1, dtype=np.float64)
    want = np.zeros((L, KP))
    for p in range(L):
        want[p, :len(h[p::L])] = h[p::L]
    assert np.array_equal(got, want)


def test_reference_is_the_definition():
    """tests/resamp_ref.py against the definition written out sample by sample (zero-stuff, filter, keep every M-th), with the
    output count of SPEC §7 -- including T < L, where scipy.signal.upfirdn returns fewer outputs than are defined"""
    rng = np.random.default_rng(5)
    for L, M, T, n in ((3, 2, 31, 101), (2, 3, 31, 100), (5, 7, 17, 99), (4, 6, 33, 64), (7, 5, 3, 257), (1, 4, 9, 50), (4, 1, 9, 50)):
        h = rng.standard_normal(2 * T).astype(np.float32)
        x = rng.standard_normal(2 * n).astype(np.float32)
        u = np.zeros(n * L, dtype=np.complex128)
        u[::L] = resamp_ref.as_c(x)
        for ct in (False, True):
            taps = h if ct else h[:T]
            hc = resamp_ref.as_c(h) if ct else h[:T].astype(np.float64)
            v = np.convolve(u, hc)[:n * L]
            want = resamp_ref.as_iq(v[::M])
            got = resamp_ref.resample_f64(taps, x, L, M, ct)
            assert got.size == want.size == 2 * -(-n * L // M), (L, M, T)
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (L, M, T, ct)
        for cut in (1, 2, 50):
            assert resamp_ref.out_count(0, cut, L, M) + resamp_ref.out_count(cut, n - cut, L, M) == -(-n * L // M)


def test_order_model_reproduces_the_figures_of_the_spec(fir, oracle):
    """docs/SPEC.md §7 gives the reason for its accumulation order in figures of the float32 model (tests/resamp_ref.py) on
    L/M = 1/3, 1023 complex taps, int16 input, 60 000 samples: §3's order (32-tap segments, plain adds) misses the bound, as
    does compensating its segment sums alone; 16-tap segments meet it, with the compensated sum by the widest margin.  This
    keeps those figures reproducible; the kernel itself is held to the bound by tests/test_resamp_gpu.py."""
    L, M, T, n = 1, 3, 1023, 60_000
    w = max(L, M)
    taps = (fir.bpf_design_complex(T, 0.1 / w, 0.8 / w) * np.float32(L)).astype(np.float32)
    xi = np.clip(np.round(oracle.synth_iq(n, channel=3) * 14000.0), -32768, 32767).astype(np.int16)
    x = xi.astype(np.float32) * np.float32(2.0 ** -15)
    ref = resamp_ref.resample_f64(taps, x, L, M, True)
    mx = {}
    for seg, comp in ((32, False), (32, True), (16, False), (16, True)):
        l2, mx[seg, comp] = oracle.err_metrics(resamp_ref.resample_f32_order(taps, x, L, M, True, seg, comp), ref)
        print("segments of %d, compensated=%d: l2=%.3g max=%.3g" % (seg, comp, l2, mx[seg, comp]))
    assert mx[32, False] == pytest.approx(1.008e-6, rel=2e-3) and mx[32, True] == pytest.approx(1.04e-6, rel=5e-3)
    assert mx[16, False] == pytest.approx(6.97e-7, rel=5e-3) and mx[16, True] == pytest.approx(5.39e-7, rel=5e-3)


def test_row_edge_taps_are_loud_where_the_rows_end():
    """the first and the last min(L, T) taps have one magnitude, the largest by a factor of 2, with the signs the docstring
    names; sum |h|^2 = L; T <= L and T = 1 keep the first form; L = 1 has edge_taps' ends"""
    for T, L in ((95, 3), (6, 3), (22, 3), (4096, 64), (100, 64), (3, 7), (7, 7), (8, 7), (1, 5), (1, 1), (31, 1), (2, 1)):
        for ct in (False, True):
            h = row_edge_taps(T, L, ct)
            assert h.dtype == np.float32 and h.size == T * (2 if ct else 1)
            c = resamp_ref.as_c(h) if ct else h.astype(np.complex128)
            assert abs(np.sum(np.abs(c) ** 2) - L) <= 1e-5 * L
            e, top = min(L, T), np.max(np.abs(c))
            sgn = np.where(np.arange(e) % 2 == 0, 1.0, -1.0)
            ends = np.zeros(T, dtype=bool)
            ends[:e] = ends[T - e:] = True
            assert np.all(np.abs(c[ends]) >= top * (1 - 1e-6)) and np.all(np.abs(c[~ends]) <= 0.5 * top * (1 + 1e-6))
            last = c[T - e:] / top
            if T > e:
                assert np.allclose(last, (-1j if ct else -1.0) * sgn[::-1], atol=1e-6)
                lead = min(e, T - e)   # T < 2 L: the last L taps reach into the first
                assert np.allclose(c[:lead] / top, sgn[:lead], atol=1e-6)
            else:
                assert np.allclose(c / top, sgn, atol=1e-6)


def test_tile_shape_is_the_plan_headers(plan_check):
    """resamp_ref.tile_shape, from which the loud-row-end tests size their streams and cuts, against resamp_shape itself"""
    for L, M, T in LOUD_MATRIX:
        run = subprocess.run([plan_check, "shape", str(L), str(M), str(T)], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, run.stdout + run.stderr
        K, W, B, tile_out, tile_in = (int(v) for v in run.stdout.split())
        assert (K, tile_out, tile_in) == resamp_ref.tile_shape(T, L, M), (L, M, T)
        n = resamp_ref.stream_len(T, L, M)
        outs = resamp_ref.out_count(0, n, L, M)
        assert outs > 3 * tile_out and outs % tile_out and n >= 2 * K, (L, M, T)


def max_metric(y, ref):
    return np.max(np.abs(y - ref)) / np.max(np.abs(ref))


def row_end_costs(taps, x, L, M, ct):
    """{(p, which end): SPEC §3's max metric between the float64 reference with and without that tap} over the phases the
    ratio reaches, p mod gcd(L, M) = 0: the others are never evaluated and their taps are dead by definition"""
    T = taps.size // (2 if ct else 1)
    full = resamp_ref.resample_f64(taps, x, L, M, ct)
    costs = {}
    for p in range(0, min(L, T), math.gcd(L, M)):
        for end, k in (("first", p), ("last", p + ((T - 1 - p) // L) * L)):
            h = taps.copy().reshape(T, -1)
            h[k] = 0.0
            costs[p, end] = max_metric(resamp_ref.resample_f64(h.reshape(-1), x, L, M, ct), full)
    return costs


def blackman_taps(fir, T, L, M):
    """the windowed design of tests/test_resamp_gpu.py::taps_for, real taps, odd T"""
    return (fir.bpf_design(T, 0.0, 0.45 / max(L, M)) * np.float32(L)).astype(np.float32)


def test_dropping_a_row_end_is_loud(fir, oracle):
    """The property tests/test_resamp_gpu.py::test_matrix_with_loud_row_ends rests on: with row_edge_taps, zeroing the first
    tap h[p] of a phase row, and zeroing its last one h[p + ((T-1-p)//L) L], moves the float64 reference by more than 1e-2
    in SPEC §3's max metric, 1e4 over the tolerance -- for every shape of that matrix, real and complex taps, every phase
    the ratio reaches, on the streams that matrix runs, float32 and int16.
    Measured over all of them: at least 0.107 (4/3 with 4096 complex taps, float32 stream, first tap of phase 2).
    With the Blackman design of taps_for on 1/4 with 255 taps both ends of the one row cost less than 1e-8 (the window's
    end taps are zero), which the last assertion holds: this test fails on such taps."""
    smallest = (np.inf, None)
    for L, M, T in LOUD_MATRIX:
        n = resamp_ref.stream_len(T, L, M)
        for ct in (False, True):
            for i16 in (False, True):
                costs = row_end_costs(row_edge_taps(T, L, ct), signal(oracle, n, i16)[1], L, M, ct)
                assert len(costs) == 2 * len(range(0, min(L, T), math.gcd(L, M)))
                for (p, end), cost in costs.items():
                    smallest = min(smallest, (cost, (L, M, T, ct, i16, p, end)))
                    assert cost > 1e-2, (L, M, T, ct, i16, p, end, cost)
    print("smallest row-end cost %.3g at (L, M, T, complex, i16, p, end) = %s" % smallest)
    L, M, T = 1, 4, 255
    quiet = row_end_costs(blackman_taps(fir, T, L, M), signal(oracle, resamp_ref.stream_len(T, L, M), False)[1], L, M, False)
    assert max(quiet.values()) < 1e-2 * TOL, quiet


def test_order_model_meets_the_bound_with_loud_taps(fir, oracle):
    """tests/test_resamp_gpu.py::test_matrix_with_loud_row_ends asks nothing the arithmetic cannot deliver: the float32 model
    of SPEC §7's order (resamp_ref.resample_f32_order) stays within half of SPEC §3's 1e-6 of float64, in both metrics, on
    every shape of that matrix with row_edge_taps, real and complex, float32 and int16 input.
    Measured: l2 at most 1.55e-7 (8/64, 1000 complex taps, float32), max at most 3.32e-7 (3/2, 95 complex taps, int16),
    which leaves the kernel a factor of 3.
    The bound says nothing about the row ends: the Blackman design on 1/4 with 255 taps meets it as well, and there zeroing
    both ends of the row costs less than 1e-8 (test_dropping_a_row_end_is_loud)."""
    worst = {"l2": (0.0, None), "max": (0.0, None)}

    def model_error(taps, x, L, M, ct):
        return oracle.err_metrics(resamp_ref.resample_f32_order(taps, x, L, M, ct), resamp_ref.resample_f64(taps, x, L, M, ct))

    for L, M, T in LOUD_MATRIX:
        n = resamp_ref.stream_len(T, L, M)
        for ct in (False, True):
            for i16 in (False, True):
                l2, mx = model_error(row_edge_taps(T, L, ct), signal(oracle, n, i16)[1], L, M, ct)
                for name, v in (("l2", l2), ("max", mx)):
                    worst[name] = max(worst[name], (v, (L, M, T, ct, i16)))
                assert l2 <= TOL / 2 and mx <= TOL / 2, (L, M, T, ct, i16, l2, mx)
    print("model worst l2=%.3g at %s, max=%.3g at %s" % (worst["l2"] + worst["max"]))
    L, M, T = 1, 4, 255
    x = signal(oracle, resamp_ref.stream_len(T, L, M), False)[1]
    quiet = blackman_taps(fir, T, L, M)
    l2, mx = model_error(quiet, x, L, M, False)
    assert l2 <= TOL / 2 and mx <= TOL / 2, (l2, mx)
    assert max(row_end_costs(quiet, x, L, M, False).values()) < 1e-2 * TOL


def test_resamp_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_resamp.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_resamp.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # (float32, int16 input) x (real, complex taps)
    assert len(names) == 4 and all("fir_resamp_kernel" in n for n in names), names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 4
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 4
