"""The polyphase synthesis bank's host side (no GPU): its C ABI in the header, the libraries and the binding; the size rules, the
call and chunk planning, the tap table and the mirrored places of qo-100-tools_amd/csrc/if_fir_synth_plan.h through the
stand-alone checker tests/c/synth_plan_check.cpp, against Python-integer arithmetic; the fold form of tests/synth_ref.py against
the definition (the channel combiner's, centres on the grid); the analysis-then-synthesis transfer formula against the two
fold forms in sequence; the complex64 model against half the GPU test's bound; the compiled kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_ref
import synth_ref
from matrix_util import TOL, row_edge_taps, signal
from test_synth_gpu import MATRIX, stream_frames

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
