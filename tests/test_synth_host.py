"""The polyphase synthesis bank's host side (no GPU): its C ABI in the header, the libraries and the binding; the size rules, the
call and chunk planning, the tap table and the mirrored places of qo-100-tools_amd/csrc/if_fir_synth_plan.h through the
stand-alone checker tests/c/synth_plan_check.cpp, against Python-integer arithmetic; the fold form of tests/synth_ref.py against
the definition (the channel combiner's, centres on the grid); the analysis-then-synthesis transfer formula against the two
fold forms in sequence; the complex64 model against half the GPU test's bound; the depth cases of
tests/test_synth_matrix_gpu.py against the plan, a model of the ring kernel's walk against the model, and that model's
switchable faults against those cases; the compiled kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_ref
import synth_ref
from matrix_util import TOL, row_edge_taps, signal
from test_synth_gpu import MATRIX, RING_CASES, stream_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
SYNTH_ABI = {"if_fir_synth_init", "if_fir_synth_destroy", "if_fir_synth_reset", "if_fir_synth_set_input_format", "if_fir_synth_set_stream",
             "if_fir_synth_synchronize", "if_fir_synth_last_error", "if_fir_synth_sample_count", "if_fir_synth_process",
             "if_fir_synth_process_device"}
SYNTH_DEV = {"if_fir_debug_synth_config", "if_fir_debug_synth_workspace"}
POSITIONS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 63, 2 ** 64 - 1001]
CHECKER = os.path.join(ROOT, "tests", "c", "synth_plan_check.cpp")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("synth_plan_check") / "synth_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, CHECKER, "-o", exe])
    return exe


def ask(exe, lines):
    """the answer lines (lists of words) to the request lines"""
    run = subprocess.run([exe, "query"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return [line.split() for line in run.stdout.splitlines()]


def test_header_declares_and_libraries_export_the_family(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    # (if_fir_synth_device, the test-signal generator of the decimator's context, is older than this family and none of it)
    declared = set(re.findall(r"\b(if_fir_synth_[a-z_]+)\s*\(", header)) - {"if_fir_synth_device"}
    assert declared == SYNTH_ABI, declared ^ SYNTH_ABI
    assert "typedef struct if_fir_synth if_fir_synth_t;" in header and "} if_fir_synth_config_t;" in header
    section = header[header.index("polyphase synthesis bank"):]
    assert "captured into a hipGraph are refused" in section
    for field in ("ulChannels", "ulHop", "lFirstBin", "ulBins"):
        assert field in section
    assert [name for name, _ in fir.SynthConfig._fields_] == ["ulChannels", "ulHop", "lFirstBin", "ulBins"]
    assert SYNTH_ABI <= set(fir.EXPORTS) and SYNTH_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert SYNTH_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert SYNTH_ABI <= product and SYNTH_ABI <= dev
    assert not (SYNTH_DEV & product) and SYNTH_DEV <= dev
    for name in ("sample_count", "process", "process_device", "reset", "set_input_format", "set_stream", "synchronize", "debug_config",
                 "debug_workspace", "__enter__", "__exit__"):
        assert hasattr(fir.IfFirSynth, name), name


def test_self_check(plan_check):
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("chunks checked: OK"), run.stdout + run.stderr
    shapes = int(run.stdout.split()[0])
    assert shapes > 7 * 6 * 5, run.stdout


def test_self_check_under_sanitizers(tmp_path):
    """tests/c/synth_plan_check.cpp with -fsanitize=address,undefined, run as a program: the tap table into a heap buffer of
    exactly its size, the calls, the chunks and the kernels' index algebra against 128-bit arithmetic"""
    exe = str(tmp_path / "synth_plan_check_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, CHECKER, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("chunks checked: OK"), run.stdout + run.stderr


def test_size_rules_and_routes(plan_check):
    """J = 32 is the most; T within 1 .. 16 M, L within 1 .. M; the LDS the one-kernel route would need against Python's
    integers; the plan's route is the LDS ring where four workgroups of it fit a CU and the workspace route elsewhere; route 2
    can be forced where two fit and is refused where they do not, and an unknown route everywhere"""
    lines, wants = [], []
    for M in synth_ref.SIZES:
        for T, L in ((32, 1), (33, 1), (1, 1), (0, 1), (16 * M, M), (16 * M + 1, M), (16 * M, M // 2), (16 * M, M // 2 - 1), (3 * M - 5, M // 2),
                     (M, 0), (M, M + 1), (32 * 17, 17), (32 * 17 + 1, 17)):
            lines.append("config %d %d %d" % (M, T, L))
            ok = 1 <= L <= M and 1 <= T <= 16 * M and -(-T // L) <= 32
            wants.append([str(-(-T // L))] if ok else ["refused"])
    lines += ["config 96 100 10", "config 32 100 10", "config 8192 100 10"]
    wants += [["refused"]] * 3
    assert ask(plan_check, lines) == wants
    seen = set()
    for M, T, L in MATRIX:
        J, B = -(-T // L), max(1, 1024 // M)
        ring = (-(-(J - 1) // B) + 1) * B * M * 8 + 10 * M
        (batch, lds, per_cu, ring_got, fits, route, ring_per_cu), = ([int(v) for v in row] for row in ask(plan_check, ["shape %d %d %d" % (M, T, L)]))
        assert batch == B and lds == 8 * B * M + 10 * M and 1 <= per_cu <= 8 and per_cu * lds <= 160 * 1024
        want = 2 * ring <= 160 * 1024
        assert ring_got == ring and fits == int(want) and route == (2 if 4 * ring <= 160 * 1024 else 1)
        assert ring_per_cu == min(8, 160 * 1024 // ring) and (not want or ring_per_cu >= 2)
        assert ask(plan_check, ["route %d %d %d %d" % (M, T, L, r) for r in (0, 1, 2, 3)]) == [
            ["2" if 4 * ring <= 160 * 1024 else "1"], ["1"], ["2" if want else "0"], ["0"]]
        seen.add((want, 4 * ring <= 160 * 1024))
    assert seen == {(True, True), (True, False), (False, False)}


def test_calls_equal_python_integers(plan_check):
    """outputs, (c L) mod M and the carry at every position x frame count x (M, T, L) of a spread, against Python's integers;
    the refusal when (c + F) L passes 2^64 - 1"""
    rng = np.random.default_rng(5)
    lines, wants = [], []
    for M, T, L in MATRIX[::3] + ((64, 187, 17), (256, 2047, 255), (64, 32, 1)):
        for c in POSITIONS + [(2 ** 64 - 1) // L - 1000, int(rng.integers(0, 2 ** 63)) // L]:
            for F in (0, 1, 2, 999, 1000, 1001, 2 ** 20 + 7, int(rng.integers(0, 2 ** 32))):
                lines.append("call %d %d %d %d %d" % (c, F, M, L, T))
                if (c + F) * L > 2 ** 64 - 1 or c + F >= 2 ** 64:
                    wants.append(["refused"])
                else:
                    wants.append([str(v) for v in (F * L, (c * L) % M, -(-T // L) - 1)])
    got = ask(plan_check, lines)
    bad = [(lines[k], got[k], wants[k]) for k in range(len(wants)) if got[k] != wants[k]]
    assert len(got) == len(wants) and not bad, (len(bad), bad[:5])
    assert ["refused"] in wants and any(w != ["refused"] and int(w[0]) > 2 ** 40 for w in wants)
    assert ask(plan_check, ["call %d 2 64 3 5" % (2 ** 64 - 1), "call 5 10 64 0 5"]) == [["refused"], ["refused"]]


def test_chunks_cover_every_frame_once(plan_check):
    """for workspace budgets from one byte up, the chunks of a call are consecutive, cover its frames exactly, fit the
    workspace with the J - 1 frames before them, and carry the absolute index of their first output modulo M"""
    for M, T, L in ((64, 187, 17), (1024, 8 * 1024 - 3, 385), (4096, 4096 + 9, 4096), (64, 32, 1), (256, 2047, 255)):
        J = -(-T // L)
        for nbytes in (1, 8 * M * J, 8 * M * (J + 1), 8 * M * (J + 4) + 5, 1 << 20, 32 << 20, 1 << 31):
            rows = max(J, min(nbytes, 1 << 30) // (8 * M))
            most = rows - (J - 1)
            for F, c in ((1, 0), (most, 3), (most + 1, 2 ** 40 + 12345), (3 * most + 2 if most < 500 else 1000, 2 ** 32 - 5)):
                smod = (c * L) % M
                (count, *rest), = ask(plan_check, ["chunks %d %d %d %d %d %d" % (F, nbytes, M, T, L, smod)])
                got = np.array([int(v) for v in rest], dtype=object).reshape(int(count), 3)
                assert int(count) == -(-F // most)
                per = -(-F // int(count))                  # the chunks are made equally long
                at = 0
                for first, frames, s in got:
                    assert first == at and 1 <= frames <= per <= most and per - frames < int(count) and s == ((c + first) * L) % M
                    at += frames
                assert at == F


@pytest.mark.parametrize("T,L", [(1, 1), (5, 5), (6, 5), (187, 17), (64, 2), (16 * 64, 64), (4097, 4096)])
def test_tap_table_is_the_prototype_padded_to_whole_rows(plan_check, T, L):
    (row,) = ask(plan_check, ["taps %d %d" % (T, L)])
    J = -(-T // L)
    want = np.zeros(J * L)
    want[:T] = np.arange(1, T + 1)
    assert np.array_equal(np.array([float(v) for v in row]), want)


def test_places_are_the_transforms_digit_order_mirrored(plan_check):
    """place of slot s: the radix-4 digits (a last radix-2 one where M is an odd power of two) of bin (M - s) mod M reversed"""
    for M in synth_ref.SIZES:
        slots = [0, 1, 2, 3, M // 2, M - 1, 77 % M]
        for s, (place,) in zip(slots, ask(plan_check, ["place %d %d" % (M, s) for s in slots])):
            pos, length, kk = 0, M, (M - s) % M
            while length > 1:
                r = 4 if length >= 4 else 2
                pos += (kk % r) * (length // r)
                kk //= r
                length //= r
            assert int(place) == pos, (M, s)


@pytest.mark.parametrize("M", [64, 128])
@pytest.mark.parametrize("case", range(4))
def test_fold_form_is_the_definition(oracle, M, case):
    """the sum of interpolators with their NCOs on the grid (combiner_ref.reference) against the fold form, 1e-12 of the
    largest output; full width from frame 0, and a span that wraps at a first frame past 2^40"""
    T, L = ((16 * M, M), (3 * M - 5, M // 2), (187, 17), (40, 1))[case]
    F = 2 * synth_ref.terms(T, L) + 9
    h = row_edge_taps(T, L, False)
    for first, first_bin, bins in ((0, 0, M), (2 ** 40 + 12345, -3, 7), (5, M - 2, 5)):
        X = synth_ref.as_frames(signal(oracle, F * bins, False)[1], bins)
        want = synth_ref.definition_f64(h, X, M, L, first_bin, bins, first)
        got = synth_ref.fold_f64(h, X, M, L, first_bin, bins, first)
        assert got.shape == want.shape == (synth_ref.sample_count(F, L),)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (first, np.max(np.abs(got - want)), np.max(np.abs(want)))


@pytest.mark.parametrize("M,L", [(64, 64), (64, 32), (64, 17)])
def test_transfer_formula_is_analysis_then_synthesis(oracle, M, L):
    """y[n] = M sum_i x[n - i M] sum_m g[n - m L] h[i M - (n - m L)] against pfb_ref.fold_f64 followed by the fold form, random
    prototypes h != g, 1e-12 of the largest output"""
    rng = np.random.default_rng([M, L])
    h, g = rng.standard_normal(4 * M + 3), rng.standard_normal(min(5 * M - 1, 32 * L))
    n = 31 * L + 5
    x = signal(oracle, n, False)[1]
    frames = pfb_ref.fold_f64(h, x, M, L)
    got = synth_ref.fold_f64(g, frames, M, L)
    xc = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    want = synth_ref.transfer_f64(h, g, xc[:, 0] + 1j * xc[:, 1], M, L)
    assert got.shape == want.shape == (32 * L,)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (np.max(np.abs(got - want)), np.max(np.abs(want)))


def test_model_meets_half_the_bound(oracle):
    """tests/test_synth_gpu.py asks nothing the arithmetic cannot deliver: the complex64 model (the forward scipy.fft on
    complex64 read at the mirrored bin, the taps in float32 in SPEC §14's order) stays within 5e-7 of float64, in both metrics
    over the whole output, on every shape of that matrix, float32 and int16 input."""
    worst = {"l2": (0.0, None), "max": (0.0, None)}
    for M, T, L in MATRIX:
        F = stream_frames(M, T, L)
        h = row_edge_taps(T, L, False)
        for i16 in (False, True):
            X = synth_ref.as_frames(signal(oracle, F * M, i16)[1], M)
            l2, mx = oracle.err_metrics(synth_ref.iq(synth_ref.model_c64(h, X, M, L)), synth_ref.iq(synth_ref.fold_f64(h, X, M, L)))
            for name, v in (("l2", l2), ("max", mx)):
                worst[name] = max(worst[name], (v, (M, T, L, i16)))
            assert l2 <= TOL / 2 and mx <= TOL / 2, (M, T, L, i16, l2, mx)
    print("synth model worst l2=%.3g at %s, max=%.3g at %s" % (worst["l2"] + worst["max"]))


def test_depth_cases_against_the_plan(plan_check):
    """tests/synth_ref.DEPTH_CASES against if_fir_synth_plan.h: every shape is legal with the J it is listed for, the ring's
    bytes and the two fits are synth_ref.lds_route_fits', and per size the list holds the largest J the plan itself sends
    through the ring with the one after it, the largest J the ring can be forced at with the one after it, J = 1 and J = 32 --
    so a change of the LDS rules cannot empty a class unnoticed"""
    cases = synth_ref.DEPTH_CASES
    assert len(cases) == 118 and {M for M, _, _ in cases} == set(synth_ref.SIZES)
    got = ask(plan_check, ["config %d %d %d" % c for c in cases] + ["shape %d %d %d" % c for c in cases] +
              ["route %d %d %d %d" % (c + (r,)) for c in cases for r in (0, 2)])
    configs, shapes, routes = got[:len(cases)], got[len(cases):2 * len(cases)], got[2 * len(cases):]
    assert len(routes) == 2 * len(cases)
    plan, forced = {}, {}
    for k, (M, T, L) in enumerate(cases):
        J, B = synth_ref.terms(T, L), synth_ref.batch(M)
        assert configs[k] == [str(J)] and J in synth_ref.DEPTH_J[M], (M, T, L)
        batch, _, _, ring, fits, route, per_cu = (int(v) for v in shapes[k])
        assert batch == B and ring == (-(-(J - 1) // B) + 1) * B * M * 8 + 10 * M
        assert fits == int(synth_ref.lds_route_fits(M, T, L)) and (route == 2) == synth_ref.lds_route_fits(M, T, L, 4) == (per_cu >= 4)
        assert routes[2 * k] == [str(route)] and routes[2 * k + 1] == ["2" if fits else "0"]
        assert plan.setdefault((M, J), route) == route and forced.setdefault((M, J), fits) == fits   # the two shapes of a pair agree
    assert sum(forced[M, J] for M, T, L in cases for J in [synth_ref.terms(T, L)]) == 98
    for M in synth_ref.SIZES:
        Js = synth_ref.DEPTH_J[M]
        assert {1, 2, 32} <= set(Js) and sorted(plan[M, J] for J in Js) == [plan[M, J] for J in Js][::-1]   # the ring first, then never again
        last4 = max([J for J in Js if plan[M, J] == 2], default=0)
        last2 = max(J for J in Js if forced[M, J])
        assert last4 == 32 or last4 + 1 in Js, M             # either side of the plan's switch (M = 64: the ring throughout)
        assert last2 == 32 or last2 + 1 in Js, M             # either side of the ring's limit
        assert (last4, last2) == {64: (32, 32), 128: (25, 32), 256: (13, 32), 512: (7, 17), 1024: (3, 8), 2048: (1, 3), 4096: (0, 1)}[M]
        B = synth_ref.batch(M)
        assert {J for J in (B, B + 1, 2 * B, 2 * B + 1) if J <= 32} <= set(Js)   # either side of the ring's second and third batch
    for M, T, L in synth_ref.RING_STEP_CASES:
        J, B = synth_ref.terms(T, L), synth_ref.batch(M)
        assert forced[M, J] and ((J - 1) % B == 0 or not forced[M, J + 1]), (M, J)   # J on a step of NB, or the most that fits
    assert sorted({synth_ref.batch(M) for M, _, _ in synth_ref.RING_STEP_CASES}) == [1, 2, 4, 8, 16]


def _depth_inputs(oracle, M, T, L, i16=False):
    F = stream_frames(M, T, L)
    return row_edge_taps(T, L, False), synth_ref.as_frames(signal(oracle, F * M, i16)[1], M)


def _max_metric(oracle, y, ref):
    return oracle.err_metrics(synth_ref.iq(y), synth_ref.iq(ref))[1]


def test_model_meets_half_the_bound_on_the_depth_cases(oracle):
    """test_model_meets_half_the_bound's loop over tests/synth_ref.DEPTH_CASES, with the frames tests/test_synth_matrix_gpu.py
    feeds: the complex64 model within 5e-7 of float64 in both metrics, float32 and int16 input."""
    worst = {"l2": (0.0, None), "max": (0.0, None)}
    for M, T, L in synth_ref.DEPTH_CASES:
        for i16 in (False, True):
            h, X = _depth_inputs(oracle, M, T, L, i16)
            l2, mx = oracle.err_metrics(synth_ref.iq(synth_ref.model_c64(h, X, M, L)), synth_ref.iq(synth_ref.fold_f64(h, X, M, L)))
            for name, v in (("l2", l2), ("max", mx)):
                worst[name] = max(worst[name], (v, (M, T, L, i16)))
            assert l2 <= TOL / 2 and mx <= TOL / 2, (M, T, L, i16, l2, mx)
    print("synth depth model worst l2=%.3g at %s, max=%.3g at %s" % (worst["l2"] + worst["max"]))


RING_DEPTH_CASES = tuple(c for c in synth_ref.DEPTH_CASES if synth_ref.lds_route_fits(*c))


def _two_calls(h, X, M, L, cut, fault=None):
    """the second of two calls, X[cut:], with the J - 1 frames before it as its history, in one run"""
    J = synth_ref.terms(h.size, L)
    assert cut >= J - 1
    return synth_ref.ring_model_c64(h, X[cut:], M, L, X.shape[0], hist_frames=X[cut - (J - 1):cut], fault=fault, first=cut)


def test_ring_model_is_the_model_bit_for_bit(oracle):
    """synth_ref.ring_model_c64 -- runs, ring slots, warm-up, back / slot / fb as synth_ring_kernel has them -- gives
    model_c64's bits on every depth case the ring takes: one batch a run, two, the whole call in one run, and a call that
    follows another with its last J - 1 frames as the history"""
    assert len(RING_DEPTH_CASES) == 98
    for M, T, L in RING_DEPTH_CASES:
        h, X = _depth_inputs(oracle, M, T, L)
        want = synth_ref.model_c64(h, X, M, L)
        batches = -(-X.shape[0] // synth_ref.batch(M))
        assert batches > 4
        for run_len in (1, 2, batches):
            assert np.array_equal(synth_ref.ring_model_c64(h, X, M, L, run_len).view(np.uint32), want.view(np.uint32)), (M, T, L, run_len)
        cut = X.shape[0] // 3 + 1
        assert np.array_equal(_two_calls(h, X, M, L, cut).view(np.uint32), want[cut * L:].view(np.uint32)), (M, T, L)


def test_ring_faults_move_the_named_cases(oracle):
    """one fault of the ring's index algebra at a time (synth_ref.RING_FAULTS), max metric against float64 over the walk's
    output: more than 100 x the GPU tests' bound on the cases named here, the model's own bits on the others.
    back_on_multiple: every shape with J >= B + 1, none with J <= B; last_term_dropped: the B shapes from J = 2 (T < J L);
    warmup_short: every walk of one batch a run from J = 2, and no walk of a zero-history call in one run; history_ignored: the
    second of two calls from J = 2.  J = 1 has no ring depth, no warm-up and no history: no fault touches it.
    The same for back_on_multiple on tests/test_synth_gpu.RING_CASES: its (M, J) from J = B + 1 -- (128, 16), (128, 30),
    (64, 32), every M >= 256 -- would have noticed that fault too; (64, 6), (64, 11), (64, 16) and (128, 6) could not."""
    loud = 100 * TOL
    moved = {f: 0 for f in synth_ref.RING_FAULTS}
    for M, T, L in RING_DEPTH_CASES:
        h, X = _depth_inputs(oracle, M, T, L)
        J, B = synth_ref.terms(T, L), synth_ref.batch(M)
        ref, clean = synth_ref.fold_f64(h, X, M, L), synth_ref.model_c64(h, X, M, L)
        F = X.shape[0]
        cut = F // 3 + 1
        walks = {"back_on_multiple": (lambda f: synth_ref.ring_model_c64(h, X, M, L, F, fault=f), J >= B + 1, 0),
                 "last_term_dropped": (lambda f: synth_ref.ring_model_c64(h, X, M, L, 2, fault=f), T < J * L, 0),
                 "warmup_short": (lambda f: synth_ref.ring_model_c64(h, X, M, L, 1, fault=f), J >= 2, 0),
                 "history_ignored": (lambda f: _two_calls(h, X, M, L, cut, f), J >= 2, cut * L)}
        for fault, (walk, moves, at) in walks.items():
            y = walk(fault)
            if moves:
                assert _max_metric(oracle, y, ref[at:]) > loud, (fault, M, T, L)
                moved[fault] += 1
            else:
                assert np.array_equal(y, clean[at:]), (fault, M, T, L)
        assert np.array_equal(synth_ref.ring_model_c64(h, X, M, L, F, fault="warmup_short"), clean), (M, T, L)
    assert moved == {"back_on_multiple": 64, "last_term_dropped": 42, "warmup_short": 84, "history_ignored": 84}, moved
    seen = set()
    for M, T, L in RING_CASES:
        h, X = _depth_inputs(oracle, M, T, L)
        J, B = synth_ref.terms(T, L), synth_ref.batch(M)
        y = synth_ref.ring_model_c64(h, X, M, L, X.shape[0], fault="back_on_multiple")
        if J >= B + 1:
            assert _max_metric(oracle, y, synth_ref.fold_f64(h, X, M, L)) > loud, (M, T, L)
        else:
            assert np.array_equal(y, synth_ref.model_c64(h, X, M, L)), (M, T, L)
        seen.add((M, J, J >= B + 1))
    assert {(64, 6, False), (64, 11, False), (64, 16, False), (128, 6, False), (64, 32, True), (128, 16, True), (128, 30, True),
            (512, 6, True), (1024, 6, True)} <= seen and not [c for c in seen if c[0] >= 256 and not c[2]]


def test_synth_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_synth.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_synth.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # seven sizes of the transform, of the ring kernel and the carry, float32 and int16 input; one kernel for the taps
    assert len(names) == 31 and sum("synth_transform_kernel" in n for n in names) == 14 and sum("synth_carry_kernel" in n for n in names) == 2
    assert sum("synth_ring_kernel" in n for n in names) == 14 and sum("synth_emit_kernel" in n for n in names) == 1, names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 31
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 31
