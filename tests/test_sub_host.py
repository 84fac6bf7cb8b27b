"""The host side of the per-channel FIR stage over filter-bank frames (no GPU): its C ABI in the header, the libraries and the
binding; the call plan, the tile plan, the tap-major table and the size rules of qo-100-tools_amd/csrc/if_fir_sub_plan.h through
the stand-alone checker tests/c/sub_plan_check.cpp (built with the address and undefined-behaviour sanitizers, run directly)
against Python-integer arithmetic; the refusals of init word for word; the two float64 references of tests/sub_ref.py against
each other; the complex64 model against half the GPU test's bound; the compiled kernels' resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sub_ref
from matrix_util import TOL, signal
from test_sub_gpu import MATRIX, stream_frames, taps_of, words_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
SUB_ABI = {"if_fir_sub_init", "if_fir_sub_destroy", "if_fir_sub_reset", "if_fir_sub_set_input_format", "if_fir_sub_set_nco",
           "if_fir_sub_get_nco", "if_fir_sub_set_stream", "if_fir_sub_synchronize", "if_fir_sub_last_error", "if_fir_sub_frame_count",
           "if_fir_sub_process", "if_fir_sub_process_device"}
SUB_DEV = {"if_fir_debug_sub_config"}
POSITIONS = [0, 1, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1001]
CHECKER = os.path.join(ROOT, "tests", "c", "sub_plan_check.cpp")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sub_plan_check") / "sub_plan_check")
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
    declared = set(re.findall(r"\b(if_fir_sub_[a-z_]+)\s*\(", header))
    assert declared == SUB_ABI, declared ^ SUB_ABI
    assert "typedef struct if_fir_sub if_fir_sub_t;" in header and "} if_fir_sub_config_t;" in header
    section = header[header.index("per-channel FIR stage"):]
    assert "captured into a hipGraph are refused" in section
    for field in ("ulBins", "ulTaps", "ulTapRows", "ulDecimation"):
        assert field in section
    assert [name for name, _ in fir.SubConfig._fields_] == ["ulBins", "ulTaps", "ulTapRows", "ulDecimation"]
    assert {n for n in fir.EXPORTS if n.startswith("if_fir_sub_")} == SUB_ABI
    assert {n for n in fir.DEV_EXPORTS if "_sub_" in n} == SUB_DEV
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert {n for n in re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M) if "_sub_" in n} == SUB_DEV
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    family = lambda names: {n for n in names if n.startswith(("if_fir_sub_", "if_fir_debug_sub_"))}
    assert family(product) == SUB_ABI and family(dev) == SUB_ABI | SUB_DEV
    for name in ("frame_count", "process", "process_device", "reset", "set_input_format", "set_nco", "get_nco", "set_stream", "synchronize",
                 "debug_config", "__enter__", "__exit__"):
        assert hasattr(fir.IfFirSub, name), name


def test_self_check_under_sanitizers(plan_check):
    """the checker's own walk: the call plan for every R at positions up to 2^64 - 1001 against 128-bit arithmetic, every (B,
    outputs) edge of the tile plan and the kernel's index algebra, the table into a heap buffer of exactly its size, the size
    rules with their messages"""
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert run.stdout == "%d calls, %d tile plans, %d tables checked: OK\n" % (64 * 9 * 9, 6 * 14, 10), run.stdout


def test_calls_equal_python_integers(plan_check):
    """count, n0 and the low 32 bits of the first output's index at every position x frame count x R, against Python's
    integers; the refusal when c + F passes 2^64"""
    lines, wants = [], []
    for R in range(1, 65):
        for c in POSITIONS:
            for F in (0, 1, R - 1, R, R + 1, 701, 1000, 1001, 2 ** 32):
                lines.append("call %d %d %d" % (c, F, R))
                if c + F >= 2 ** 64:
                    wants.append("refused")
                else:
                    n0 = (-c) % R
                    wants.append("%d %d %d" % (sub_ref.frame_count(c, F, R), n0, (c + n0) % 2 ** 32))
    got = ask(plan_check, lines)
    bad = [(lines[k], got[k], wants[k]) for k in range(len(wants)) if got[k] != wants[k]]
    assert len(got) == len(wants) and not bad, (len(bad), bad[:5])
    assert "refused" in wants and any(w != "refused" and int(w.split()[0]) == 2 ** 32 for w in wants)
    assert ask(plan_check, ["call %d 1 1" % (2 ** 64 - 1), "call %d 1 1" % (2 ** 64 - 2)]) == ["refused", "1 0 %d" % (2 ** 32 - 2)]


def test_tiles_equal_python_integers(plan_check):
    """every (B, outputs) edge: the items are runs of 4 outputs x B bins, a tile is 256 consecutive items, the bin runs fastest"""
    lines, wants = [], []
    for B in (1, 63, 64, 65, 4095, 4096):
        edge = -(-1024 // B)
        for count in (0, 1, 3, 4, 5, 8, edge - 1, edge, edge + 1, 4 * edge, 176, 2 ** 32):
            count = max(count, 0)
            runs = -(-count // 4)
            lines.append("tiles %d %d" % (B, count))
            wants.append("%d %d %d" % (runs, runs * B, -(-runs * B // 256)))
        for item in (0, 1, B - 1, B, B + 1, 255, 256, 257, 1000 * B + B // 2, 2 ** 30 * B - 1):
            lines.append("item %d %d" % (B, item))
            wants.append("%d %d" % (item // B * 4, item % B))
    assert ask(plan_check, lines) == wants


def test_table_is_tap_major(plan_check):
    for B, T, rows in ((1, 1, 1), (3, 5, 1), (3, 5, 3), (65, 17, 65), (4096, 2, 1)):
        got = np.array([[float(v) for v in line.split()] for line in ask(plan_check, ["table %d %d %d" % (B, T, rows)])])
        k, j = np.divmod(np.arange(T * B), B)
        assert got.shape == (T * B, 2) and np.array_equal(got[:, 0], 1000 * (j if rows == B else 0) + k + 1) and not np.any(got[:, 1])


INIT_REFUSALS = [
    (dict(bins=0), "bins must be 1..4096 (got 0)"),
    (dict(bins=4097), "bins must be 1..4096 (got 4097)"),
    (dict(taps=0), "taps must be 1..128 (got 0)"),
    (dict(taps=129), "taps must be 1..128 (got 129)"),
    (dict(no_taps=True), "taps must be 1..128 (got 33), pfTaps is NULL"),
    (dict(rows=0), "tap rows must be 1 or the 24 bins (got 0)"),
    (dict(rows=2), "tap rows must be 1 or the 24 bins (got 2)"),
    (dict(rows=25), "tap rows must be 1 or the 24 bins (got 25)"),
    (dict(decimation=0), "decimation must be 1..64 (got 0)"),
    (dict(decimation=65), "decimation must be 1..64 (got 65)"),
    (dict(max_frames=0), "ullMaxFrames must be 1..2^32 (got 0)"),
    (dict(max_frames=2 ** 32 + 1), "ullMaxFrames must be 1..2^32 (got 4294967297)"),
    (dict(bins=0, taps=0, rows=7, decimation=0, max_frames=0), "bins must be 1..4096 (got 0)"),   # the first rule broken speaks
]


def sub_init(fir, L, bins=24, taps=33, rows=1, decimation=2, max_frames=4096, no_taps=False, no_cfg=False, no_ctx=False):
    h = np.linspace(-1.0, 1.0, 130 * 24, dtype=np.float32)
    cfg = fir.SubConfig(bins, taps, rows, decimation)
    ctx = ctypes.c_void_p(1)
    ok = L.if_fir_sub_init(None if no_ctx else ctypes.byref(ctx), None if no_cfg else ctypes.byref(cfg),
                           None if no_taps else h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), max_frames, 0)
    return ok, ctx


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("args,message", INIT_REFUSALS)
def test_init_refusals_word_for_word(fir, plan_check, dev, args, message):
    """in the product and in the development library, before the device is asked for; the same words from the plan header"""
    L = fir.dev_lib() if dev else fir.lib()
    ok, ctx = sub_init(fir, L, **args)
    assert ok == 0 and ctx.value is None
    assert L.if_fir_sub_last_error(None).decode() == "if_fir_sub_init: " + message
    a = dict(bins=24, taps=33, rows=1, decimation=2, max_frames=4096, no_taps=False)
    a.update(args)
    assert ask(plan_check, ["config %d %d %d %d %d %d" % (a["bins"], a["taps"], a["rows"], a["decimation"], a["max_frames"], not a["no_taps"])]) == [message]


@pytest.mark.parametrize("dev", [False, True])
def test_missing_pointers_and_null_contexts(fir, plan_check, dev):
    L = fir.dev_lib() if dev else fir.lib()
    ok, _ = sub_init(fir, L, no_ctx=True, bins=0)
    assert ok == 0 and L.if_fir_sub_last_error(None).decode() == "if_fir_sub_init: ppCtx is NULL"
    ok, ctx = sub_init(fir, L, no_cfg=True)
    assert ok == 0 and ctx.value is None and L.if_fir_sub_last_error(None).decode() == "if_fir_sub_init: pCfg is NULL"
    # with nothing to refuse an init fails only where there is no device, and then says so
    ok, ctx = sub_init(fir, L)
    if ok:
        L.if_fir_sub_destroy(ctx)
    else:
        assert ctx.value is None and L.if_fir_sub_last_error(None).decode() == "if_fir_sub_init: no HIP device"
    assert ask(plan_check, ["config 24 33 1 2 4096 1", "config 4096 128 4096 64 %d 1" % 2 ** 32]) == ["ok", "ok"]
    # every entry point that takes a context returns 0 for none: set_nco with frequencies in and out of range, and with NULL
    for f in (0.1, 0.5000001, float("nan")):
        assert L.if_fir_sub_set_nco(None, (ctypes.c_double * 1)(f)) == 0
    two = (ctypes.c_double * 2)(0.0, 0.0)
    assert L.if_fir_sub_set_nco(None, None) == 0 and L.if_fir_sub_get_nco(None, two) == 0
    assert L.if_fir_sub_reset(None) == 0 and L.if_fir_sub_synchronize(None) == 0 and L.if_fir_sub_set_stream(None, None) == 0
    assert L.if_fir_sub_set_input_format(None, 0) == 0 and L.if_fir_sub_frame_count(None, 1000) == 0
    assert L.if_fir_sub_process(None, None, None, 0, None) == 0 and L.if_fir_sub_process_device(None, None, None, 0, None) == 0
    L.if_fir_sub_destroy(None)
    if dev:
        assert L.if_fir_debug_sub_config(None, 0, None, 0) == 0


def test_binding_refuses_what_c_cannot_hold(fir):
    with pytest.raises(fir.IfFirError, match="if_fir_sub_init: bins, taps, tap rows and decimation must be unsigned"):
        fir.IfFirSub(np.ones(4, dtype=np.float32), -1)
    with pytest.raises(fir.IfFirError, match=r"if_fir_sub_init: tap rows must be 1 or the 5 bins \(got 2\)"):
        fir.IfFirSub(np.ones((2, 4), dtype=np.float32), 5)


@pytest.mark.parametrize("B,T,rows,R", MATRIX)
def test_definition_is_the_decimator_per_bin(oracle, B, T, rows, R):
    """mix every frame, filter, pick (Python integers for the phase and the offsets) against oracle.fir_nco_f64 per bin, 1e-12
    of the largest output, words all 0 and mixed, at position 0, past 2^32, at 2^63 and at the last position a stream has"""
    F = min(stream_frames(B), 4 * T + 3 * R + 40)
    X = sub_ref.as_frames(signal(oracle, stream_frames(B) * B, False)[1], B)[:F]
    for mixed in (False, True):
        for first in (0, 2 ** 33 + 5, 2 ** 63, 2 ** 64 - F - 1):
            want = sub_ref.channel_f64(oracle, taps_of(B, T, rows), X, R, words_of(B, mixed), first)
            got = sub_ref.definition_f64(taps_of(B, T, rows), X, R, words_of(B, mixed), first)
            assert got.shape == want.shape == (sub_ref.frame_count(first, F, R), B)
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (mixed, first, np.max(np.abs(got - want)))


def test_model_meets_half_the_bound(oracle):
    """tests/test_sub_gpu.py asks nothing the arithmetic cannot deliver: the complex64 model of SPEC §15's order stays within
    5e-7 of float64, in both metrics over the whole output, on every shape of that matrix, float32 and int16 input, words all 0
    and mixed, at position 0 and at 2^33 + 5"""
    worst = {"l2": (0.0, ()), "max": (0.0, ())}
    for B, T, rows, R in MATRIX:
        F = stream_frames(B)
        for i16 in (False, True):
            xf = signal(oracle, F * B, i16)[1]
            for mixed in (False, True):
                for first in (0, 2 ** 33 + 5):
                    ref = sub_ref.channel_f64(oracle, taps_of(B, T, rows), sub_ref.as_frames(xf, B), R, words_of(B, mixed), first)
                    model = sub_ref.model_c64(taps_of(B, T, rows), xf.view(np.complex64).reshape(F, B), R, words_of(B, mixed), first)
                    l2, mx = oracle.err_metrics(sub_ref.iq(model), sub_ref.iq(ref))
                    for name, v in (("l2", l2), ("max", mx)):
                        worst[name] = max(worst[name], (v, (B, T, rows, R, i16, mixed, first)))
                    assert l2 <= TOL / 2 and mx <= TOL / 2, (B, T, rows, R, i16, mixed, first, l2, mx)
    print("sub model worst l2=%.3g at %s, max=%.3g at %s" % (worst["l2"] + worst["max"]))


def test_model_segments_are_the_spec_order():
    for T in range(1, 129):
        segs = sub_ref.segments(T)
        assert [k for s in segs for k in s] == list(range(T - 1, -1, -1))
        assert all(len(s) == 16 for s in segs[1:]) and 1 <= len(segs[0]) <= 16 and len(segs) == -(-T // 16)


def test_sub_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_sub.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_sub.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # the stage and the carry, float32 and int16 input
    assert len(names) == 4 and sum("fir_sub_kernel" in n for n in names) == 2 and sum("sub_carry_kernel" in n for n in names) == 2, names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 4
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 4
    assert re.findall(r"LDS Size \[bytes/block\]: (\d+)", text) == ["0"] * 4
