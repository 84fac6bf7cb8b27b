"""The host side of the corner turn (no GPU): its C ABI in the header, the libraries and the binding; the tile map, the offsets
and the rules of qo-100-tools_amd/csrc/if_fir_turn_plan.h through the stand-alone checker tests/c/turn_plan_check.cpp (built
with the address and undefined-behaviour sanitizers, run directly) and against Python's integers; the refusals of init word
for word; the numpy reference tests/turn_ref.py against a definition written element by element and against the up-converter's
int16 rule; the compiled kernels' resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import duc_ref
import turn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
TURN_ABI = {"if_fir_turn_init", "if_fir_turn_destroy", "if_fir_turn_set_input_format", "if_fir_turn_set_output_format",
            "if_fir_turn_set_stream", "if_fir_turn_synchronize", "if_fir_turn_last_error", "if_fir_turn_process",
            "if_fir_turn_process_device"}
TURN_DEV = {"if_fir_debug_turn_config"}
FIELDS = ["ulDirection", "ulBins", "ulChannels", "ulFirst", "ulInputFormat", "ulOutputFormat"]
CHECKER = os.path.join(ROOT, "tests", "c", "turn_plan_check.cpp")
NO_LIST = 2 ** 64 - 1


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("turn_plan_check") / "turn_plan_check")
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
    declared = set(re.findall(r"\b(if_fir_turn_[a-z_]+)\s*\(", header))
    assert declared == TURN_ABI, declared ^ TURN_ABI
    assert "typedef struct if_fir_turn if_fir_turn_t;" in header and "} if_fir_turn_config_t;" in header
    section = header[header.index("corner turn"):]
    assert "captured into a hipGraph are refused" in section
    assert "IF_FIR_TURN_TO_STREAMS = 0" in section and "IF_FIR_TURN_TO_FRAMES = 1" in section
    for field in FIELDS:
        assert field in section
    assert "if_fir_turn_reset" not in header
    assert [name for name, _ in fir.TurnConfig._fields_] == FIELDS
    assert ctypes.sizeof(fir.TurnConfig) == 24
    assert (fir.TURN_TO_STREAMS, fir.TURN_TO_FRAMES) == (turn_ref.TO_STREAMS, turn_ref.TO_FRAMES) == (0, 1)
    assert {n for n in fir.EXPORTS if n.startswith("if_fir_turn_")} == TURN_ABI
    assert {n for n in fir.DEV_EXPORTS if "_turn_" in n} == TURN_DEV
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert {n for n in re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M) if "_turn_" in n} == TURN_DEV
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    family = lambda names: {n for n in names if n.startswith(("if_fir_turn_", "if_fir_debug_turn_"))}
    assert family(product) == TURN_ABI and family(dev) == TURN_ABI | TURN_DEV
    for name in ("process", "process_device", "set_input_format", "set_output_format", "set_stream", "synchronize", "debug_config",
                 "__enter__", "__exit__"):
        assert hasattr(fir.IfFirTurn, name), name


def test_self_check_under_sanitizers(plan_check):
    """the checker's own walk: the tile map played as the kernel runs it over the issue's F, C, B and four selections on 1 and
    on 3 workgroups, both directions, with an LDS tile of exactly the planned size; the offsets of the first and last tiles at
    P = 2^32 and F = 2^32 against 128-bit arithmetic; the rules and their messages in order"""
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    m = re.fullmatch(r"(\d+) cases of (\d+), (\d+) tiles, (\d+) offsets, (\d+) rules checked: OK\n", run.stdout)
    assert m and int(m.group(1)) > 1900 and int(m.group(2)) == 2808 and int(m.group(3)) > 90000 and int(m.group(4)) > 700000 \
        and int(m.group(5)) == 22, run.stdout


def test_tiles_equal_python_integers(plan_check):
    """columns and frames of a tile, the LDS pitch (odd: a column access is conflict-free) and size, and the tile counts"""
    lines, wants = [], []
    for cols in list(range(1, 70)) + [127, 128, 129, 200, 918, 4097, 8192]:
        for F in (0, 1, 63, 64, 65, 4095, 4096, 4097, 2 ** 32 - 1, 2 ** 32):
            X = turn_ref.tile_cols(cols)
            TF = 4096 // X
            tx = -(-cols // X)
            lines.append("tile %d %d" % (cols, F))
            wants.append("%d %d %d %d %d %d" % (X, TF, X | 1, TF * (X | 1), tx, tx * -(-F // TF)))
            assert (X | 1) % 2 == 1 and TF >= 64 and TF * (X | 1) * 8 <= 49152
    assert ask(plan_check, lines) == wants


# (arguments, message): each breaks its rule and, in the last line, every rule at once
INIT_REFUSALS = [
    (dict(direction=2), "unknown direction 2"),
    (dict(bins=0), "bins must be 1..8192 (got 0)"),
    (dict(bins=8193), "bins must be 1..8192 (got 8193)"),
    (dict(channels=0, sel=None), "channels must be 1..130, the frame's bins (got 0)"),
    (dict(channels=131, sel=None), "channels must be 1..130, the frame's bins (got 131)"),
    (dict(sel=None, first=128), "bins [128, 131) of the span are outside the frame's 130"),
    (dict(sel=None, first=2 ** 32 - 1), "bins [4294967295, 4294967298) of the span are outside the frame's 130"),
    (dict(in_fmt=2), "unknown input format 2"),
    (dict(out_fmt=2), "unknown output format 2"),
    (dict(first=1), "ulFirst must be 0 beside a list of bins (got 1)"),
    (dict(sel=[5, 130, 7]), "bin 130 at place 1 of the list is outside the frame's 130"),
    (dict(sel=[5, 129, 2 ** 32 - 1]), "bin 4294967295 at place 2 of the list is outside the frame's 130"),
    (dict(sel=[5, 9, 5]), "bin 5 is listed twice (places 0 and 2)"),
    (dict(max_frames=0), "ullMaxFrames must be 1..2^32 (got 0)"),
    (dict(max_frames=2 ** 32 + 1), "ullMaxFrames must be 1..2^32 (got 4294967297)"),
    (dict(direction=7, bins=0, channels=0, first=9, in_fmt=9, out_fmt=9, sel=[9, 9, 9], max_frames=0), "unknown direction 7"),
    (dict(bins=8, channels=3, first=9, in_fmt=9, out_fmt=9, sel=[9, 9, 9], max_frames=0), "bins [9, 12) of the span are outside the frame's 8"),
    (dict(bins=8, channels=3, first=5, out_fmt=9, sel=[9, 9, 9], max_frames=0), "unknown output format 9"),
    (dict(bins=8, channels=3, first=0, sel=[7, 7, 9], max_frames=0), "bin 7 is listed twice (places 0 and 1)"),
]


def turn_init(fir, L, direction=0, bins=130, channels=3, first=0, in_fmt=0, out_fmt=0, sel=(5, 129, 7), max_frames=4096, no_cfg=False,
              no_ctx=False):
    cfg = fir.TurnConfig(direction, bins, channels, first, in_fmt, out_fmt)
    ctx = ctypes.c_void_p(1)
    arr = (ctypes.c_uint32 * len(sel))(*sel) if sel is not None else None
    ok = L.if_fir_turn_init(None if no_ctx else ctypes.byref(ctx), None if no_cfg else ctypes.byref(cfg), arr, max_frames, 0)
    return ok, ctx


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("args,message", INIT_REFUSALS)
def test_init_refusals_word_for_word(fir, plan_check, dev, args, message):
    """in the product and in the development library, before the device is asked for; the same words from the plan header"""
    L = fir.dev_lib() if dev else fir.lib()
    ok, ctx = turn_init(fir, L, **args)
    assert ok == 0 and ctx.value is None
    assert L.if_fir_turn_last_error(None).decode() == "if_fir_turn_init: " + message
    a = dict(direction=0, bins=130, channels=3, first=0, in_fmt=0, out_fmt=0, sel=(5, 129, 7), max_frames=4096)
    a.update(args)
    sel = a["sel"]
    line = "config %d %d %d %d %d %d %d %d" % (a["direction"], a["bins"], a["channels"], a["first"], a["in_fmt"], a["out_fmt"], a["max_frames"],
                                              NO_LIST if sel is None else len(sel))
    assert ask(plan_check, [line + "".join(" %d" % v for v in (sel or ()))]) == [message]


@pytest.mark.parametrize("dev", [False, True])
def test_missing_pointers_and_null_contexts(fir, plan_check, dev):
    L = fir.dev_lib() if dev else fir.lib()
    ok, _ = turn_init(fir, L, no_ctx=True, bins=0)
    assert ok == 0 and L.if_fir_turn_last_error(None).decode() == "if_fir_turn_init: ppCtx is NULL"
    ok, ctx = turn_init(fir, L, no_cfg=True)
    assert ok == 0 and ctx.value is None and L.if_fir_turn_last_error(None).decode() == "if_fir_turn_init: pCfg is NULL"
    # with nothing to refuse an init fails only where there is no device, and then says so
    ok, ctx = turn_init(fir, L)
    if ok:
        L.if_fir_turn_destroy(ctx)
    else:
        assert ctx.value is None and L.if_fir_turn_last_error(None).decode() == "if_fir_turn_init: no HIP device"
    assert ask(plan_check, ["config 0 130 3 0 0 0 4096 3 5 129 7", "config 1 8192 8192 0 1 1 %d %d" % (2 ** 32, NO_LIST),
                            "config 0 130 3 127 0 1 1 %d" % NO_LIST]) == ["ok", "ok", "ok"]
    # every entry point that takes a context returns 0 for none
    assert L.if_fir_turn_synchronize(None) == 0 and L.if_fir_turn_set_stream(None, None) == 0
    assert L.if_fir_turn_set_input_format(None, 0) == 0 and L.if_fir_turn_set_output_format(None, 0) == 0
    assert L.if_fir_turn_process(None, None, None, 0, 0) == 0 and L.if_fir_turn_process_device(None, None, None, 0, 0) == 0
    L.if_fir_turn_destroy(None)
    if dev:
        assert L.if_fir_debug_turn_config(None, 0) == 0


def test_call_rules_word_for_word(plan_check):
    """pitch below the frames, pitch above 2^40, frames above init's, in that order"""
    assert ask(plan_check, ["call 0 0 1", "call 100 100 100", "call 100 %d 100" % 2 ** 40, "call 8 7 4", "call 8 %d 4" % (2 ** 40 + 1),
                            "call 8 8 7", "call 9 8 7"]) == [
        "ok", "ok", "ok", "a row pitch of 7 elements is below the call's 8 frames", "a row pitch of 1099511627777 elements is above 2^40",
        "8 frames exceed ullMaxFrames 7 of init", "a row pitch of 8 elements is below the call's 9 frames"]


def test_binding_refuses_what_c_cannot_hold(fir):
    with pytest.raises(fir.IfFirError, match="if_fir_turn_init: direction, bins, channels, first and the formats must be unsigned"):
        fir.IfFirTurn(0, -1, channels=1)
    with pytest.raises(fir.IfFirError, match="if_fir_turn_init: listed bins must be unsigned 32-bit integers"):
        fir.IfFirTurn(0, 8, sel=[1, -2])
    with pytest.raises(fir.IfFirError, match="if_fir_turn_init: 2 listed bins for 3 channels"):
        fir.IfFirTurn(0, 8, sel=[1, 2], channels=3)
    with pytest.raises(fir.IfFirError, match=r"if_fir_turn_init: bins must be 1..8192 \(got 8193\)"):
        fir.IfFirTurn(1, 8193, channels=1)


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def test_int16_rule_is_spelled_out():
    """the special values one by one; equal to duc_ref.to_i16 on every finite value"""
    q = 2.0 ** -15
    cases = [(float("nan"), 0), (-float("nan"), 0), (float("inf"), 32767), (-float("inf"), -32768), (0.0, 0), (-0.0, 0),
             (1e-45, 0), (-1e-45, 0), (3.4e38, 32767), (-3.4e38, -32768), (32767.5 * q, 32767), (-32767.5 * q, -32768),
             (32766.5 * q, 32766), (-32768.5 * q, -32768), (1.0, 32767), (-1.0, -32768), (0.5 * q, 0), (1.5 * q, 2), (2.5 * q, 2),
             (-0.5 * q, 0), (-1.5 * q, -2), (-2.5 * q, -2), (1000.5 * q, 1000), (1001.5 * q, 1002), (0.75 * q, 1)]
    for v, want in cases:
        assert int(turn_ref.to_i16(np.float32(v))) == want, (v, want)
    payload = np.array([0x7f800001, 0xffc12345], dtype=np.uint32).view(np.float32)
    assert np.array_equal(turn_ref.to_i16(payload), np.array([0, 0], dtype=np.int16))
    rng = np.random.default_rng(20)
    finite = np.concatenate([rng.standard_normal(20000).astype(np.float32), (rng.integers(-40000, 40000, 20000) + 0.5).astype(np.float32) * np.float32(q),
                             turn_ref.special_f32()])
    finite = finite[np.isfinite(finite)]
    got = turn_ref.to_i16(finite)
    assert got.dtype == np.int16 and np.array_equal(got, duc_ref.to_i16(finite.astype(np.float64)))
    assert np.any(got == 32767) and np.any(got == -32768)


@pytest.mark.parametrize("i16,o16", turn_ref.FORMATS)
@pytest.mark.parametrize("kind", turn_ref.SELECTIONS)
def test_reference_against_the_definition_element_by_element(kind, i16, o16):
    """SPEC §20 written as loops: both directions, every format pair, a pitch with a tail"""
    B, C, F = 70, 9, 5
    sel = turn_ref.selection(kind, B, C)
    assert len(set(sel)) == C and all(0 <= s < B for s in sel)
    frames = turn_ref.make_elements((F, B), i16, 1)
    rows = turn_ref.to_streams(frames, sel, o16)
    assert rows.shape == (C, F, 2) and rows.dtype == (np.int16 if o16 else np.float32)
    for c in range(C):
        for a in range(F):
            assert turn_ref.same_bits(rows[c, a], turn_ref.conv(frames[a, sel[c]], o16))
    rin = turn_ref.make_elements((C, F), i16, 2)
    out = turn_ref.to_frames(rin, sel, B, o16)
    assert out.shape == (F, B, 2)
    listed = {s: c for c, s in enumerate(sel)}
    for a in range(F):
        for i in range(B):
            want = turn_ref.conv(rin[listed[i], a], o16) if i in listed else np.zeros(2, dtype=out.dtype)
            assert turn_ref.same_bits(out[a, i], want)
    assert out[:, [i for i in range(B) if i not in listed]].tobytes() == bytes(out.itemsize * 2 * F * (B - C))
    if not i16 and not o16:
        assert turn_ref.same_bits(rows, np.ascontiguousarray(np.swapaxes(frames[:, sel], 0, 1)))   # the bits, NaN payloads included
    if i16 and not o16:
        assert np.array_equal(rows.astype(np.float64) * 32768.0, np.swapaxes(frames[:, sel], 0, 1).astype(np.float64))   # exact


def test_selections_are_what_they_say():
    for B in turn_ref.BINS:
        for C in [c for c in turn_ref.CHANNELS if c <= B] + [B]:
            for kind in turn_ref.SELECTIONS:
                sel = turn_ref.selection(kind, B, C)
                assert len(sel) == C and len(set(sel)) == C and min(sel) >= 0 and max(sel) < B, (kind, B, C)
    s = turn_ref.selection("straddle", 918, 200)
    for e in range(64, 918, 64):
        assert e - 1 in s and e in s                       # both sides of every tile edge of the frame side
    assert (s[1], s[2]) == (63, 64) and s[0] not in (63, 64)     # rotated by one: a pair sits at an odd and the next even place
    assert turn_ref.selection("reversed", 918, 200) == turn_ref.selection("span", 918, 200)[::-1]
    sc = turn_ref.selection("scattered", 918, 200)
    assert sc != sorted(sc) and sc != sorted(sc, reverse=True)


def test_turn_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_turn.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_turn.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # two directions times four format pairs
    assert len(names) == 8 and len(set(names)) == 8 and all("turn_kernel" in n for n in names), names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 8
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 8
