"""The arbitrary-ratio resampler's host side (no GPU): its C ABI in the header, the libraries and the binding; the call
planning, the tile bases and the tap table of qo-100-tools_amd/csrc/if_fir_arb_plan.h through the stand-alone checker
tests/c/arb_plan_check.cpp, against Python-integer arithmetic; the float64 reference of tests/arb_ref.py against the rational
resampler's on the phase grid; the float32 order model; the compiled kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import arb_ref
import resamp_ref
from matrix_util import TOL, row_edge_taps, signal
from test_arb_gpu import MATRIX, REMAINDERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
ARB_ABI = {"if_fir_arb_init", "if_fir_arb_destroy", "if_fir_arb_reset", "if_fir_arb_set_step", "if_fir_arb_set_input_format",
           "if_fir_arb_set_stream", "if_fir_arb_synchronize", "if_fir_arb_last_error", "if_fir_arb_out_count", "if_fir_arb_process",
           "if_fir_arb_process_device", "if_fir_arb_step_from_rates"}
ARB_DEV = {"if_fir_debug_arb_config"}
STEPS = [2 ** 26, 2 ** 26 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 34] + \
    [int(v) for v in np.random.default_rng(12).integers(2 ** 26, 2 ** 34, 200, endpoint=True)]
POSITIONS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 12345, 2 ** 63]
CHECKER = os.path.join(ROOT, "tests", "c", "arb_plan_check.cpp")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("arb_plan_check") / "arb_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, CHECKER, "-o", exe])
    return exe


def ask(exe, lines):
    """one answer (a list of words) per request line"""
    run = subprocess.run([exe, "query"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    out = run.stdout.splitlines()
    return [line.split() for line in out]


def test_header_declares_and_libraries_export_the_family(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_arb_[a-z_]+)\s*\(", header))
    assert declared == ARB_ABI, declared ^ ARB_ABI
    assert "typedef struct if_fir_arb if_fir_arb_t;" in header
    section = header[header.index("arbitrary-ratio resampler"):]
    assert "captured into a hipGraph are refused" in section
    assert ARB_ABI <= set(fir.EXPORTS) and ARB_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert ARB_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert ARB_ABI <= product and ARB_ABI <= dev
    assert not (ARB_DEV & product) and ARB_DEV <= dev
    for name in ("step", "set_step", "out_count", "process", "process_device", "reset", "set_input_format", "set_stream", "__enter__",
                 "__exit__"):
        assert hasattr(fir.IfFirArb, name), name
    assert callable(fir.step_from_rates)


def test_self_check_under_sanitizers(tmp_path):
    """tests/c/arb_plan_check.cpp with -fsanitize=address,undefined: every table into a heap buffer of exactly its size, the
    tile bases against 128-bit arithmetic, the places of a tile inside its window, a random walk of calls and retunes"""
    exe = str(tmp_path / "arb_plan_check_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, CHECKER, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("calls checked: OK"), run.stdout + run.stderr
    assert run.stdout.startswith("%d tables, %d tiles, %d calls" % (7 * 6, 7 * 6 * 27 * 4 * 5, 4 * 20000)), run.stdout


def test_out_count_and_tile_bases_equal_python_integers(plan_check):
    """arb_out_count at every step x position x time offset x call size, and arb_time at tiles up to the last one of the largest
    call, against Python's integers"""
    rng = np.random.default_rng(3)
    lines, wants = [], []
    for R in STEPS:
        for c in POSITIONS:
            for off in (0, 1, R - 1, int(rng.integers(0, 2 ** 34))):
                tau = (c << 32) + off
                for n in (0, 1, 2, 3, 5, 1000, int(rng.integers(0, 2 ** 36))):
                    lines.append("count %d %d %d %d" % (c, tau, n, R))
                    wants.append([str(arb_ref.out_count(c, tau, n, R)), "1"])
    base = len(lines)
    for R in STEPS:
        for off in (0, R - 1, 2 ** 34 - 1):
            for i in (0, 1024, 1024 * 4194303, 2 ** 32, 2 ** 42, 1024 * int(rng.integers(0, 2 ** 32))):
                t = off + i * R
                lines.append("time %d %d %d" % (off, i, R))
                wants.append([str(t >> 32), str(t & 0xffffffff)])
    got = ask(plan_check, lines)
    assert len(got) == len(wants)
    bad = [(lines[k], got[k], wants[k]) for k in range(len(wants)) if got[k] != wants[k]]
    assert not bad, (len(bad), bad[:5])
    assert base == len(STEPS) * 6 * 4 * 7
    # refused: a call that would carry the position past 2^64; a time outside the invariant is reported as such
    got = ask(plan_check, ["count %d %d 2 %d" % (2 ** 64 - 1, (2 ** 64 - 1) << 32, 2 ** 32), "count 5 %d 1 %d" % ((5 << 32) + 2 ** 34, 2 ** 32),
                           "count 5 %d 1 %d" % ((5 << 32) - 1, 2 ** 32)])
    assert got == [["-1", "1"], ["0", "0"], ["2", "0"]]


def test_places_of_a_tile(plan_check):
    """arb_place: the input index, the phase and the fraction of an output of a tile against Python integers; the fraction is
    the low bits rounded once to float32"""
    rng = np.random.default_rng(4)
    lines, wants = [], []
    for R in STEPS[:6] + STEPS[6::20]:
        for b in (4, 7, 10):
            for f0 in (0, 2 ** 32 - 1, int(rng.integers(0, 2 ** 32))):
                for l in (0, 1, 255, 256, 1023):
                    t = f0 + l * R
                    f = t & 0xffffffff
                    mu = np.float32(f & ((1 << (32 - b)) - 1)) / np.float32(1 << (32 - b))
                    lines.append("place %d %d %d %d" % (f0, l, R, b))
                    wants.append((t >> 32, f >> (32 - b), float(mu)))
    got = ask(plan_check, lines)
    assert [(int(g[0]), int(g[1]), float.fromhex(g[2])) for g in got] == wants


def test_walk_of_calls_and_retunes_keeps_the_invariant(plan_check):
    """a seeded random walk of call sizes -- none, a few, thousands -- with retunes between them: the checker's count equals
    Python's at every call, zero-output calls included, and c 2^32 <= tau < c 2^32 + 2^34 holds after each"""
    rng = np.random.default_rng(7)
    for start in (0, 2 ** 32 - 5, 2 ** 63):
        c, R = start, STEPS[int(rng.integers(len(STEPS)))]
        tau = c << 32
        lines, wants, zero = [], [], 0
        for k in range(3000):
            pick = int(rng.integers(8))
            n = 0 if pick == 0 else int(rng.integers(4)) if pick < 5 else int(rng.integers(5000))
            if rng.integers(3) == 0:
                R = STEPS[int(rng.integers(len(STEPS)))]
            m = arb_ref.out_count(c, tau, n, R)
            zero += (m == 0 and n > 0)
            lines.append("count %d %d %d %d" % (c, tau, n, R))
            wants.append([str(m), "1"])
            c, tau = c + n, tau + m * R
            assert c << 32 <= tau < (c << 32) + 2 ** 34
        assert zero > 100
        assert ask(plan_check, lines) == wants


def test_summed_counts_over_any_split_equal_the_one_call_count():
    rng = np.random.default_rng(8)
    for R in STEPS[:6] + STEPS[6::10]:
        n = int(rng.integers(1, 20000))
        off = int(rng.integers(0, R))
        whole = arb_ref.out_count(0, off, n, R)
        for _ in range(5):
            cuts = np.sort(rng.integers(0, n + 1, int(rng.integers(1, 6))))
            pieces = np.diff(np.concatenate([[0], cuts, [n]]))
            c, tau, total = 0, off, 0
            for s in pieces:
                m = arb_ref.out_count(c, tau, int(s), R)
                c, tau, total = c + int(s), tau + m * R, total + m
            assert total == whole, (R, n, off, pieces)


@pytest.mark.parametrize("b,T", [(4, 1), (4, 15), (4, 16), (4, 17), (6, 6), (5, 1000), (7, 2049), (10, 8192), (4, 8192)])
def test_tap_table_holds_both_neighbouring_phases(plan_check, b, T):
    """the table read back through the plan header's builder: entry (p, j) is the pair (h[p + j P], h[p + 1 + j P]), zeros where
    the index reaches T -- T < P (phases without a tap), a last row of one tap, the largest tables"""
    lines = ask(plan_check, ["table %d %d" % (b, T)])
    P = 1 << b
    K, KP = (int(v) for v in lines[0])
    assert K == -(-T // P) and KP >= K and KP % 2 == 1
    got = np.array([[[float(v) for v in pair.split(":")] for pair in row] for row in lines[1:]])
    assert got.shape == (P, KP, 2)
    h = np.zeros((KP + 1) * P + 1)
    h[:T] = np.arange(1, T + 1)
    want = np.zeros((P, KP, 2))
    for j in range(K):
        want[:, j, 0] = h[j * P:j * P + P]
        want[:, j, 1] = h[j * P + 1:j * P + P + 1]
    assert np.array_equal(got, want)
    # the same through the reference's rows: row p beside row p + 1
    g = arb_ref.rows(np.arange(1, T + 1, dtype=np.float32), b)
    assert np.array_equal(got[:, :K, 0], g[:P]) and np.array_equal(got[:, :K, 1], g[1:])


def test_tile_shape_is_the_plan_headers(plan_check):
    """arb_ref.tile_shape, from which the tests size their streams, against arb_shape itself"""
    for b, T, R in MATRIX + REMAINDERS:
        (K, KP, P, tile_out, x_len, entries, lds), = ([int(v) for v in row] for row in ask(plan_check, ["shape %d %d %d" % (T, b, R)]))
        assert (K, tile_out, x_len) == arb_ref.tile_shape(T, b, R), (b, T, R)
        assert P == 1 << b and entries == P * KP and lds == 8 * (entries + x_len) <= 160 * 1024
        n = arb_ref.stream_len(T, b, R)
        outs = arb_ref.out_count(0, 0, n, R)
        assert outs > 3 * tile_out and outs % tile_out and n >= 2 * K + 17, (b, T, R)


@pytest.mark.parametrize("b,M,T", [(6, 63, 1537), (4, 7, 255), (6, 64, 4096)])
def test_reference_is_the_rational_resamplers_on_the_phase_grid(oracle, b, M, T):
    """R = M 2^32 / P makes mu = 0 at every output: the reference equals resamp_ref.resample_f64(h, x, P, M) to 1e-12"""
    P = 1 << b
    R = M * 2 ** 32 // P
    assert R * P == M * 2 ** 32
    h = row_edge_taps(T, P, False)
    x = signal(oracle, arb_ref.stream_len(T, b, R), False)[1]
    got, counts = arb_ref.resample_f64(h, x, b, R)
    want = resamp_ref.resample_f64(h, x, P, M)
    assert got.size == want.size == 2 * counts[0]
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    # and in pieces with the step unchanged it is the same stream
    n = x.size // 2
    again, counts = arb_ref.resample_f64(h, x, b, [(n // 3, R), (0, R), (n - n // 3, R)])
    assert np.array_equal(again, got) and counts[1] == 0


def test_order_model_meets_half_the_bound_with_loud_taps(oracle):
    """tests/test_arb_gpu.py asks nothing the arithmetic cannot deliver: the float32 model of SPEC §12's order
    (arb_ref.resample_f32_order) stays within 5e-7 of float64, in both metrics, on every shape of that matrix with
    row_edge_taps, float32 and int16 input.
    Measured: l2 at most 1.59e-7 (b = 6, 1537 taps, R = 2^32 - 12345, float32), max at most 3.26e-7 (b = 5, 1000 taps,
    R = 2^34 - 1, float32)."""
    worst = {"l2": (0.0, None), "max": (0.0, None)}
    for b, T, R in MATRIX + REMAINDERS:
        n = arb_ref.stream_len(T, b, R)
        h = row_edge_taps(T, 1 << b, False)
        for i16 in (False, True):
            x = signal(oracle, n, i16)[1]
            l2, mx = oracle.err_metrics(arb_ref.resample_f32_order(h, x, b, R), arb_ref.resample_f64(h, x, b, R)[0])
            for name, v in (("l2", l2), ("max", mx)):
                worst[name] = max(worst[name], (v, (b, T, R, i16)))
            assert l2 <= TOL / 2 and mx <= TOL / 2, (b, T, R, i16, l2, mx)
    print("arb model worst l2=%.3g at %s, max=%.3g at %s" % (worst["l2"] + worst["max"]))


def max_metric(y, ref):
    return np.max(np.abs(y - ref)) / np.max(np.abs(ref))


def test_dropping_a_row_end_is_loud(oracle):
    """The property tests/test_arb_gpu.py's loud rows rest on: with row_edge_taps, zeroing the first tap h[p] of a phase row,
    and zeroing its last one h[p + ((T-1-p)//P) P], moves the float64 reference by more than 1e-2 in SPEC §3's max metric, 1e4
    over the tolerance -- for every shape of the matrix, float32 and int16, every phase row p < min(P, T) that an output of
    the stream reaches.  An output weights its row p by 1 - mu and its row p + 1 by mu; a row counts as reached when some
    output of the stream gives it a weight of at least 1/4 (R = 2^32 + 77 moves mu by 77 / 2^26 per output: in 3090 outputs
    row 1 gets no more than 0.0035, and a tap that enters with that weight cannot cost 1e-2 whatever its size)."""
    smallest = (np.inf, None)
    for b, T, R in MATRIX + REMAINDERS:
        P = 1 << b
        n = arb_ref.stream_len(T, b, R)
        h = row_edge_taps(T, P, False)
        _, p, mu = arb_ref.places(0, arb_ref.out_count(0, 0, n, R), R, b)
        reached = set(p[mu <= 0.75].tolist()) | set((p[mu >= 0.25] + 1).tolist())
        tested = 0
        for i16 in (False, True):
            x = signal(oracle, n, i16)[1]
            full = arb_ref.resample_f64(h, x, b, R)[0]
            # (every row of a short filter; of a long one the first, the last and a spread of the reached rows)
            phases = sorted(r for r in reached if r < min(P, T))
            if len(phases) > 12:
                phases = phases[:2] + phases[2:-2:max(1, len(phases) // 8)] + phases[-2:]
            for row in phases:
                for end, k in (("first", row), ("last", row + ((T - 1 - row) // P) * P)):
                    cut = h.copy()
                    cut[k] = 0.0
                    cost = max_metric(arb_ref.resample_f64(cut, x, b, R)[0], full)
                    smallest = min(smallest, (cost, (b, T, R, i16, row, end)))
                    assert cost > 1e-2, (b, T, R, i16, row, end, cost)
                    tested += 1
        assert tested >= 4 or T == 1, (b, T, R)
    print("smallest row-end cost %.3g at (b, T, R, i16, p, end) = %s" % smallest)


def test_step_from_rates(fir, plan_check):
    """exact ratios, ties (to even, as rint), and results outside 2^26 .. 2^34, from the library and from the plan header"""
    cases = [((64.0, 63.0), None), ((1.0, 1.0), 2 ** 32), ((63.0, 64.0), 63 * 2 ** 26), ((1.0, 64.0), 2 ** 26), ((4.0, 1.0), 2 ** 34),
             ((1.0e6, 2 * 333e3), None), ((48000.0, 48000.144), None),
             # ties: (2 k + 1) / 2^33 is k + 1/2 units: to the even neighbour
             ((2.0 ** 27 + 1, 2.0 ** 33), 2 ** 26), ((2.0 ** 27 + 3, 2.0 ** 33), 2 ** 26 + 2), ((2.0 ** 33 + 5, 2.0 ** 33), 2 ** 32 + 2),
             # just outside, either side; nonsense
             ((2.0 ** 27 - 1, 2.0 ** 33), 2 ** 26), ((2.0 ** 27 - 3, 2.0 ** 33), 0), ((2.0 ** 35 + 1, 2.0 ** 33), 2 ** 34), ((2.0 ** 35 + 3, 2.0 ** 33), 0), ((1.0, 65.0), 0),
             ((4.01, 1.0), 0), ((0.0, 1.0), 0), ((1.0, 0.0), 0), ((-1.0, 1.0), 0), ((float("nan"), 1.0), 0), ((float("inf"), 1.0), 0)]
    lines = []
    for (rate_in, rate_out), want in cases:
        if want is None:
            want = round(rate_in / rate_out * 2.0 ** 32)
            assert 2 ** 26 <= want <= 2 ** 34
        assert fir.step_from_rates(rate_in, rate_out) == want, (rate_in, rate_out)
        lines.append(("step %r %r" % (rate_in, rate_out), [str(want)]))
    assert ask(plan_check, [l for l, _ in lines]) == [w for _, w in lines]


def test_arb_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_arb.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_arb.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # float32 and int16 input
    assert len(names) == 2 and all("fir_arb_kernel" in n for n in names), names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
