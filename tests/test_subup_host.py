"""The host side of the per-bin interpolating FIR stage over frames (no GPU): its C ABI in the header, the libraries and the
binding; the call plan, the tile plan, the zero-padded tap table and the size rules of qo-100-tools_amd/csrc/if_fir_subup_plan.h
through the stand-alone checker tests/c/subup_plan_check.cpp (built with the address and undefined-behaviour sanitizers, run
directly) against Python-integer arithmetic; the refusals of init word for word; the float64 references of tests/subup_ref.py
against each other and against scipy; the complex64 model against half the GPU test's bound; the compiled kernels' resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import subup_ref
from matrix_util import TOL, signal
from test_subup_gpu import MATRIX, stream_frames, taps_of, words_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
SUBUP_ABI = {"if_fir_subup_init", "if_fir_subup_destroy", "if_fir_subup_reset", "if_fir_subup_set_input_format", "if_fir_subup_set_nco",
             "if_fir_subup_get_nco", "if_fir_subup_set_stream", "if_fir_subup_synchronize", "if_fir_subup_last_error",
             "if_fir_subup_frame_count", "if_fir_subup_process", "if_fir_subup_process_device"}
SUBUP_DEV = {"if_fir_debug_subup_config"}
CHECKER = os.path.join(ROOT, "tests", "c", "subup_plan_check.cpp")
LAST = 2 ** 64 - 1


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("subup_plan_check") / "subup_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, CHECKER, "-o", exe])
    return exe


def ask(exe, lines):
    """the answer lines to the request lines"""
    run = subprocess.run([exe, "query"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr
    return run.stdout.splitlines()


def test_header_declares_and_libraries_export_exactly_the_family(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_subup_[a-z_]+)\s*\(", header))
    assert declared == SUBUP_ABI, declared ^ SUBUP_ABI
    assert "typedef struct if_fir_subup if_fir_subup_t;" in header and "} if_fir_subup_config_t;" in header
    section = header[header.index("per-bin interpolating FIR stage"):]
    assert "captured into a hipGraph are refused" in section
    for field in ("ulBins", "ulTaps", "ulTapRows", "ulInterpolation"):
        assert field in section
    assert [name for name, _ in fir.SubUpConfig._fields_] == ["ulBins", "ulTaps", "ulTapRows", "ulInterpolation"]
    assert {n for n in fir.EXPORTS if n.startswith("if_fir_subup_")} == SUBUP_ABI
    assert {n for n in fir.DEV_EXPORTS if "_subup_" in n} == SUBUP_DEV
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert {n for n in re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M) if "_subup_" in n} == SUBUP_DEV
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    family = lambda names: {n for n in names if n.startswith(("if_fir_subup_", "if_fir_debug_subup_"))}
    assert family(product) == SUBUP_ABI and family(dev) == SUBUP_ABI | SUBUP_DEV
    for name in ("frame_count", "process", "process_device", "reset", "set_input_format", "set_nco", "get_nco", "set_stream", "synchronize",
                 "debug_config", "__enter__", "__exit__"):
        assert hasattr(fir.IfFirSubUp, name), name


def test_self_check_under_sanitizers(plan_check):
    """the checker's own walk: the call plan for every R at positions up to the refusal edge against 128-bit arithmetic, every
    (B, R, frames) edge of the tile plan and the kernel's index algebra, the table into a heap buffer of exactly its size, the
    size rules with their messages"""
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert run.stdout == "%d calls, %d tile plans, %d tables checked: OK\n" % (64 * 9 * 9, 6 * 3 * 12, 12), run.stdout


def test_calls_equal_python_integers(plan_check):
    """count and (c R) mod 2^32 at every position x frame count x R, against Python's integers; the refusal exactly when
    (c + F) R passes 2^64 - 1"""
    lines, wants = [], []
    for R in range(1, 65):
        E = LAST // R
        for c in (0, 1, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 63 // R, E - 1001, E - 1, E):
            for F in (0, 1, R, 701, 1000, 1001, 1002, 2 ** 32):
                lines.append("call %d %d %d" % (c, F, R))
                wants.append("refused" if (c + F) * R > LAST else "%d %d" % (F * R, (c * R) % 2 ** 32))
                assert (wants[-1] == "refused") == (subup_ref.frame_count(c, F, R) == 0 and F > 0)
    got = ask(plan_check, lines)
    bad = [(lines[k], got[k], wants[k]) for k in range(len(wants)) if got[k] != wants[k]]
    assert len(got) == len(wants) and not bad, (len(bad), bad[:5])
    assert "refused" in wants and "%d 0" % (64 * 2 ** 32) in wants
    for R in (1, 3, 64):
        F = 101
        c = subup_ref.last_start(F, R)
        assert ask(plan_check, ["call %d %d %d" % (c, F, R), "call %d %d %d" % (c + 1, F, R)]) == ["%d %d" % (F * R, c * R % 2 ** 32), "refused"]


def test_tiles_equal_python_integers(plan_check):
    """every (B, R, frames) edge: an item is one (bin, phase) over a run of 32 frames, a tile is 256 consecutive items, the bin
    runs fastest, then the phase"""
    lines, wants = [], []
    for B in (1, 63, 64, 65, 4095, 4096):
        for R in (1, 2, 7, 64):
            for F in (0, 1, 31, 32, 33, 97, 701, 2 ** 32):
                runs = -(-F // 32)
                lines.append("tiles %d %d %d" % (B, R, F))
                wants.append("%d %d %d" % (runs, runs * R * B, -(-runs * R * B // 256)))
            for item in (0, 1, B - 1, B, B + 1, 255, 256, 257, R * B - 1, R * B, 1000 * R * B + B // 2, 2 ** 27 * R * B - 1):
                lines.append("item %d %d %d" % (B, R, item))
                wants.append("%d %d %d" % (item // (R * B) * 32, item // B % R, item % B))
    assert ask(plan_check, lines) == wants


def test_table_is_tap_major_and_zero_padded(plan_check):
    for B, T, rows, R in ((1, 1, 1, 1), (3, 5, 1, 2), (3, 5, 3, 2), (65, 17, 65, 3), (64, 33, 64, 64), (4096, 2, 1, 1)):
        got = np.array([float(line) for line in ask(plan_check, ["table %d %d %d %d" % (B, T, rows, R)])])
        padded = -(-T // R) * R
        k, r = np.divmod(np.arange(padded * rows), rows)
        assert got.shape == (padded * rows,) and np.array_equal(got, np.where(k < T, 1000 * r + k + 1, 0))


INIT_REFUSALS = [
    (dict(bins=0), "bins must be 1..4096 (got 0)"),
    (dict(bins=4097), "bins must be 1..4096 (got 4097)"),
    (dict(taps=0), "taps must be 1..2048 (got 0)"),
    (dict(taps=2049, interpolation=64), "taps must be 1..2048 (got 2049)"),
    (dict(no_taps=True), "taps must be 1..2048 (got 33), pfTaps is NULL"),
    (dict(rows=0), "tap rows must be 1 or the 24 bins (got 0)"),
    (dict(rows=2), "tap rows must be 1 or the 24 bins (got 2)"),
    (dict(rows=25), "tap rows must be 1 or the 24 bins (got 25)"),
    (dict(interpolation=0), "interpolation must be 1..64 (got 0)"),
    (dict(interpolation=65), "interpolation must be 1..64 (got 65)"),
    (dict(interpolation=1), "taps per phase J = ceil(33 / 1) = 33 exceed 32"),
    (dict(taps=2048, interpolation=63), "taps per phase J = ceil(2048 / 63) = 33 exceed 32"),
    (dict(max_frames=0), "ullMaxFrames must be 1..2^32 (got 0)"),
    (dict(max_frames=2 ** 32 + 1), "ullMaxFrames must be 1..2^32 (got 4294967297)"),
    (dict(bins=0, taps=0, rows=7, interpolation=0, max_frames=0), "bins must be 1..4096 (got 0)"),   # the first rule broken speaks
]


def subup_init(fir, L, bins=24, taps=33, rows=1, interpolation=2, max_frames=4096, no_taps=False, no_cfg=False, no_ctx=False):
    h = np.linspace(-1.0, 1.0, 2049 * 25, dtype=np.float32)
    cfg = fir.SubUpConfig(bins, taps, rows, interpolation)
    ctx = ctypes.c_void_p(1)
    ok = L.if_fir_subup_init(None if no_ctx else ctypes.byref(ctx), None if no_cfg else ctypes.byref(cfg),
                             None if no_taps else h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), max_frames, 0)
    return ok, ctx


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("args,message", INIT_REFUSALS)
def test_init_refusals_word_for_word(fir, plan_check, dev, args, message):
    """in the product and in the development library, before the device is asked for; the same words from the plan header"""
    L = fir.dev_lib() if dev else fir.lib()
    ok, ctx = subup_init(fir, L, **args)
    assert ok == 0 and ctx.value is None
    assert L.if_fir_subup_last_error(None).decode() == "if_fir_subup_init: " + message
    a = dict(bins=24, taps=33, rows=1, interpolation=2, max_frames=4096, no_taps=False)
    a.update(args)
    assert ask(plan_check, ["config %d %d %d %d %d %d" % (a["bins"], a["taps"], a["rows"], a["interpolation"], a["max_frames"],
                                                          not a["no_taps"])]) == [message]


@pytest.mark.parametrize("dev", [False, True])
def test_missing_pointers_and_null_contexts(fir, plan_check, dev):
    L = fir.dev_lib() if dev else fir.lib()
    ok, _ = subup_init(fir, L, no_ctx=True, bins=0)
    assert ok == 0 and L.if_fir_subup_last_error(None).decode() == "if_fir_subup_init: ppCtx is NULL"
    ok, ctx = subup_init(fir, L, no_cfg=True)
    assert ok == 0 and ctx.value is None and L.if_fir_subup_last_error(None).decode() == "if_fir_subup_init: pCfg is NULL"
    # with nothing to refuse an init fails only where there is no device, and then says so
    ok, ctx = subup_init(fir, L)
    if ok:
        L.if_fir_subup_destroy(ctx)
    else:
        assert ctx.value is None and L.if_fir_subup_last_error(None).decode() == "if_fir_subup_init: no HIP device"
    assert ask(plan_check, ["config 24 33 1 2 4096 1", "config 4096 2048 4096 64 %d 1" % 2 ** 32, "config 1 32 1 1 1 1"]) == ["ok"] * 3
    # every entry point that takes a context returns 0 for none: set_nco with frequencies in and out of range, and with NULL
    for f in (0.1, 0.5000001, float("nan")):
        assert L.if_fir_subup_set_nco(None, (ctypes.c_double * 1)(f)) == 0
    two = (ctypes.c_double * 2)(0.0, 0.0)
    assert L.if_fir_subup_set_nco(None, None) == 0 and L.if_fir_subup_get_nco(None, two) == 0
    assert L.if_fir_subup_reset(None) == 0 and L.if_fir_subup_synchronize(None) == 0 and L.if_fir_subup_set_stream(None, None) == 0
    assert L.if_fir_subup_set_input_format(None, 0) == 0 and L.if_fir_subup_frame_count(None, 1000) == 0
    assert L.if_fir_subup_process(None, None, None, 0, None) == 0 and L.if_fir_subup_process_device(None, None, None, 0, None) == 0
    L.if_fir_subup_destroy(None)
    if dev:
        assert L.if_fir_debug_subup_config(None, 0, None, 0) == 0


def test_binding_refuses_what_c_cannot_hold(fir):
    with pytest.raises(fir.IfFirError, match="if_fir_subup_init: bins, taps, tap rows and interpolation must be unsigned"):
        fir.IfFirSubUp(np.ones(4, dtype=np.float32), -1)
    with pytest.raises(fir.IfFirError, match=r"if_fir_subup_init: tap rows must be 1 or the 5 bins \(got 2\)"):
        fir.IfFirSubUp(np.ones((2, 4), dtype=np.float32), 5)
    with pytest.raises(fir.IfFirError, match=r"if_fir_subup_init: taps per phase J = ceil\(70 / 2\) = 35 exceed 32"):
        fir.IfFirSubUp(np.ones(70, dtype=np.float32), 5, 2)


@pytest.mark.parametrize("B,T,rows,R", MATRIX)
def test_definitions_are_the_interpolator_per_bin(oracle, B, T, rows, R):
    """zero-stuff, convolve, rotate and the phase form (Python integers for the phase) against combiner_ref.reference per bin,
    1e-12 of the largest output, words all 0 and mixed, at position 0, past 2^32 and at the last position a call accepts;
    scipy's upfirdn for words 0"""
    J = -(-T // R)
    F = min(stream_frames(B, R), 2 * J + 9)
    X = subup_ref.as_frames(signal(oracle, stream_frames(B, R) * B, False)[1], B)[:F]
    taps = taps_of(B, T, rows, R)
    for mixed in (False, True):
        for first in (0, 2 ** 33 + 5, subup_ref.last_start(F, R)):
            want = subup_ref.channel_f64(taps, X, R, words_of(B, mixed), first)
            assert want.shape == (subup_ref.frame_count(first, F, R), B) == (F * R, B)
            for form in (subup_ref.definition_f64, subup_ref.phase_f64):
                got = form(taps, X, R, words_of(B, mixed), first)
                assert got.shape == want.shape
                assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (form.__name__, mixed, first, np.max(np.abs(got - want)))
            if mixed and first and B > 1:   # (bin 0's word is 0)
                assert not np.allclose(want, subup_ref.channel_f64(taps, X, R, words_of(B, mixed), 0))
    want = subup_ref.channel_f64(taps, X, R, words_of(B, False))
    assert np.max(np.abs(subup_ref.reference_upfirdn(taps, X, R) - want)) <= 1e-12 * np.max(np.abs(want))
    assert subup_ref.frame_count(subup_ref.last_start(F, R) + 1, F, R) == 0


def test_model_meets_half_the_bound(oracle):
    """tests/test_subup_gpu.py asks nothing the arithmetic cannot deliver: the complex64 model of SPEC §16's order stays within
    5e-7 of float64, in both metrics over the whole output, on every shape of that matrix, float32 and int16 input, words all 0
    and mixed, at position 0 and at 2^33 + 5"""
    worst = {"l2": (0.0, ()), "max": (0.0, ())}
    for B, T, rows, R in MATRIX:
        F = stream_frames(B, R)
        taps = taps_of(B, T, rows, R)
        for i16 in (False, True):
            xf = signal(oracle, F * B, i16)[1]
            for mixed in (False, True):
                for first in (0, 2 ** 33 + 5):
                    ref = subup_ref.phase_f64(taps, subup_ref.as_frames(xf, B), R, words_of(B, mixed), first)
                    model = subup_ref.model_c64(taps, xf.view(np.complex64).reshape(F, B), R, words_of(B, mixed), first)
                    l2, mx = oracle.err_metrics(subup_ref.iq(model), subup_ref.iq(ref))
                    for name, v in (("l2", l2), ("max", mx)):
                        worst[name] = max(worst[name], (v, (B, T, rows, R, i16, mixed, first)))
                    assert l2 <= TOL / 2 and mx <= TOL / 2, (B, T, rows, R, i16, mixed, first, l2, mx)
    print("subup model worst l2=%.3g at %s, max=%.3g at %s" % (worst["l2"] + worst["max"]))


def test_model_depends_on_taps_and_factor_alone():
    """the model of a stream cut in two (the second piece with the first one's tail as its history) has the bits of one run:
    nothing in the order knows the call"""
    rng = np.random.default_rng(16)
    B, T, R, F = 5, 17, 3, 40
    J = -(-T // R)
    taps = rng.standard_normal((B, T)).astype(np.float32)
    X = (rng.standard_normal((F, B)) + 1j * rng.standard_normal((F, B))).astype(np.complex64)
    words = [0, 1, 2 ** 31, 12345678, 2 ** 32 - 1]
    one = subup_ref.model_c64(taps, X, R, words, first=7)
    for cut in (1, J - 2, J, 23):
        tail = subup_ref.model_c64(taps, X[cut - min(cut, J - 1):], R, words, first=7 + cut - min(cut, J - 1))[min(cut, J - 1) * R:]
        assert np.array_equal(tail.view(np.uint32), one[cut * R:].view(np.uint32)), cut


def test_subup_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_subup.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_subup.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # the stage per window bucket (1, 2, 4, 8, 16, 32) and the carry, float32 and int16 input
    assert len(names) == 14 and sum("fir_subup_kernel" in n for n in names) == 12 and sum("subup_carry_kernel" in n for n in names) == 2, names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 14
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 14
    assert re.findall(r"LDS Size \[bytes/block\]: (\d+)", text) == ["0"] * 14
