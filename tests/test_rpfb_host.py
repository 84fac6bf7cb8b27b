"""The real-input polyphase filter bank's host side (no GPU): its C ABI in the header, the libraries and the binding; the call
planning, the tap table, the places of a bin and its partner and the untangling twiddles of
qo-100-tools_amd/csrc/if_fir_rpfb_plan.h through the stand-alone checker tests/c/rpfb_plan_check.cpp, against Python-integer
arithmetic; the three float64 forms of tests/rpfb_ref.py against each other; the float32 model against half the GPU test's
bound; the init refusals and their messages; the compiled kernels' resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ddc_ref
import rpfb_ref
from matrix_util import TOL, row_edge_taps
from test_rpfb_gpu import MATRIX, stream_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
RPFB_ABI = {"if_fir_rpfb_init", "if_fir_rpfb_destroy", "if_fir_rpfb_reset", "if_fir_rpfb_set_input_format", "if_fir_rpfb_set_stream",
            "if_fir_rpfb_synchronize", "if_fir_rpfb_last_error", "if_fir_rpfb_frame_count", "if_fir_rpfb_process",
            "if_fir_rpfb_process_device"}
RPFB_DEV = {"if_fir_debug_rpfb_config"}
POSITIONS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 63, 2 ** 64 - 1001, 2 ** 64 - 1]
CHECKER = os.path.join(ROOT, "tests", "c", "rpfb_plan_check.cpp")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rpfb_plan_check") / "rpfb_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, CHECKER, "-o", exe])
    return exe


def ask(exe, lines):
    """the answer lines (lists of words) to the request lines"""
    run = subprocess.run([exe, "query"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return [line.split() for line in run.stdout.splitlines()]


def digit_reverse(k, N):
    pos, length = 0, N
    while length > 1:
        r = 4 if length >= 4 else 2
        pos += (k % r) * (length // r)
        k //= r
        length //= r
    return pos


def test_header_declares_and_libraries_export_the_family(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_rpfb_[a-z_]+)\s*\(", header))
    assert declared == RPFB_ABI, declared ^ RPFB_ABI
    assert "typedef struct if_fir_rpfb if_fir_rpfb_t;" in header and "} if_fir_rpfb_config_t;" in header
    section = header[header.index("real-input polyphase filter bank"):]
    assert "captured into a hipGraph are refused" in section and "docs/SPEC.md §17" in section
    for field in ("ulChannels", "ulHop", "ulFirstBin", "ulBins"):
        assert field in section
    assert [name for name, _ in fir.RpfbConfig._fields_] == ["ulChannels", "ulHop", "ulFirstBin", "ulBins"]
    assert all(t is ctypes.c_uint32 for _, t in fir.RpfbConfig._fields_)
    assert RPFB_ABI <= set(fir.EXPORTS) and RPFB_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert RPFB_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert RPFB_ABI <= product and RPFB_ABI <= dev
    assert not (RPFB_DEV & product) and RPFB_DEV <= dev
    for name in ("frame_count", "process", "process_device", "reset", "set_input_format", "set_stream", "synchronize", "debug_config",
                 "__enter__", "__exit__"):
        assert hasattr(fir.IfFirRpfb, name), name


def test_self_check(plan_check):
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("calls checked: OK"), run.stdout + run.stderr
    assert run.stdout.startswith("%d shapes, %d calls" % (7 * 7, 7 * 7 * 6 * 11 * 8)), run.stdout


def test_self_check_under_sanitizers(tmp_path):
    """tests/c/rpfb_plan_check.cpp with -fsanitize=address,undefined, run as a program: the tap table, the places and the
    twiddles into heap buffers of exactly their sizes, the calls and the kernel's index algebra against 128-bit arithmetic"""
    exe = str(tmp_path / "rpfb_plan_check_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, CHECKER, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("calls checked: OK"), run.stdout + run.stderr


def test_calls_equal_python_integers(plan_check):
    """frames, runs of frames, the first frame's offset, c mod M and the carry at every position (up to 2^64 - 1) x call size x
    (M, D, T) of a spread, against Python's integers; the refusal past 2^64"""
    rng = np.random.default_rng(5)
    lines, wants = [], []
    for M, T, D in MATRIX[::3] + ((128, 187, 17), (256, 2047, 255), (8192, 65340, 4096), (1024, 4095, 768)):
        (K, batch, group, lds, per_cu), = ([int(v) for v in row] for row in ask(plan_check, ["shape %d %d" % (M, T)]))
        assert K == -(-T // M) and batch == max(1, 2048 // M) and group == max(8, 2 * batch) and group % batch == 0
        assert lds == 4 * batch * M + 6 * M and 1 <= per_cu <= 8 and per_cu * lds <= 160 * 1024
        for c in POSITIONS + [int(rng.integers(0, 2 ** 63))]:
            for n in (0, 1, 2, D - 1, D, D + 1, 1000, 2 ** 20 + 7, int(rng.integers(0, 2 ** 36))):
                lines.append("call %d %d %d %d %d" % (c, n, M, D, T))
                if c + n >= 2 ** 64:
                    wants.append(["refused"])
                    continue
                frames = rpfb_ref.frame_count(c, n, D)
                wants.append([str(v) for v in (frames, -(-frames // group), rpfb_ref.first_offset(c, D), c % M, T - 1)])
    got = ask(plan_check, lines)
    assert len(got) == len(wants)
    bad = [(lines[k], got[k], wants[k]) for k in range(len(wants)) if got[k] != wants[k]]
    assert not bad, (len(bad), bad[:5])
    assert ["refused"] in wants and any(line.startswith("call %d 0 " % (2 ** 64 - 1)) for line in lines)
    assert ask(plan_check, ["call %d 2 128 3 5" % (2 ** 64 - 1), "call 5 10 128 0 5"]) == [["refused"], ["refused"]]


@pytest.mark.parametrize("M,T", [(128, 1), (128, 127), (128, 128), (128, 129), (256, 187), (256, 16 * 256), (8192, 8193)])
def test_tap_table_is_the_rows_time_reversed(plan_check, M, T):
    rows = ask(plan_check, ["taps %d %d" % (M, T)])
    K = -(-T // M)
    got = np.array([[float(v) for v in row] for row in rows])
    assert got.shape == (K, M)
    h = np.zeros(K * M)
    h[:T] = np.arange(1, T + 1)
    assert np.array_equal(got, h.reshape(K, M)[:, ::-1])


def test_every_bin_and_its_partner_are_where_the_transform_leaves_them(plan_check):
    """for every M and EVERY channel k = 0 .. M/2: Z[k] at the digit-reversed place of k mod M/2 of an M/2-point transform, its
    partner at that of (M/2 - k) mod M/2; k = 0 and M/2 read Z[0] twice, k = M/4 is its own partner"""
    for M in rpfb_ref.SIZES:
        H = M // 2
        got = ask(plan_check, ["place %d %d" % (M, k) for k in range(H + 1)])
        want = [[str(digit_reverse(k % H, H)), str(digit_reverse((H - k) % H, H))] for k in range(H + 1)]
        assert got == want, M
        assert got[0] == got[H] == ["0", "0"] and got[M // 4][0] == got[M // 4][1]
        assert sorted(int(p) for p, _ in got[:H]) == list(range(H))
    assert ask(plan_check, ["size %d" % M for M in (64, 96, 128, 8192, 16384, 0)]) == [["refused"], ["refused"], ["ok"], ["ok"], ["refused"], ["refused"]]
    assert ask(plan_check, ["span 128 0 65", "span 128 0 66", "span 128 64 1", "span 128 64 2", "span 128 5 0"]) == [
        ["ok"], ["refused"], ["ok"], ["refused"], ["refused"]]


def signal(oracle, n, i16):
    return ddc_ref.real_signal(oracle, n, i16)[1]


SMALL = ((128, 187, 17), (128, 16 * 128, 128), (256, 3 * 256 - 5, 128), (256, 2047, 255), (512, 1017, 1), (256, 1, 256), (128, 100, 128))


@pytest.mark.parametrize("M,T,D", SMALL)
def test_fold_form_is_the_definition(oracle, M, T, D):
    """mix-filter-pick by the definition against the fold form with its real-input transform, 1e-12 of the largest output; with a
    span, and at an odd position that is a multiple of neither D nor M"""
    n = min(stream_len(M, T, D), 40 * D + T // 4)
    h = row_edge_taps(T, M, False)
    r = signal(oracle, n, False)
    for first, first_bin, bins in ((0, 0, M // 2 + 1), (2 ** 40 + 12345, M // 4 - 1, 3)):
        want = rpfb_ref.definition_f64(h, r, M, D, first_bin, bins, first)
        got = rpfb_ref.fold_f64(h, r, M, D, first_bin, bins, first)
        assert got.shape == want.shape == (rpfb_ref.frame_count(first, n, D), bins)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (first, np.max(np.abs(got - want)), np.max(np.abs(want)))


@pytest.mark.parametrize("M,T,D", MATRIX)
def test_fold_form_is_the_oracle_per_channel(oracle, M, T, D):
    """SPEC §17 defines channel k as the down-converter with the NCO at k / M: on every shape of the GPU matrix, the channels 0,
    1, 5, M/4, M/2 - 1, M/2 and a seeded one of the fold form equal oracle.fir_nco_f64 on the widened stream at phase word
    k 2^32 / M to 1e-12 of the largest output of the bank"""
    n = stream_len(M, T, D)
    h = row_edge_taps(T, M, False)
    r = signal(oracle, n, False)
    got = rpfb_ref.fold_f64(h, r, M, D)
    scale = np.max(np.abs(got))
    for k in (0, 1, 5, M // 4, M // 2 - 1, M // 2, int(np.random.default_rng([M, T, D]).integers(M // 2 + 1))):
        want = rpfb_ref.channel_f64(oracle, h, r, M, D, k)
        assert want.shape == got[:, k].shape
        assert np.max(np.abs(got[:, k] - want)) <= 1e-12 * scale, (k, np.max(np.abs(got[:, k] - want)), scale)


def test_model_meets_half_the_bound(oracle):
    """tests/test_rpfb_gpu.py asks nothing the arithmetic cannot deliver: the float32 model (fold in float32 in SPEC §13's order,
    scipy.fft on complex64 with M/2 points, the untangling pass in float32) stays within 5e-7 of float64, in both metrics over
    the whole output, on every shape of that matrix, float32 and int16 input; its bins 0 and M/2 are real."""
    worst = {"l2": (0.0, None), "max": (0.0, None)}
    for M, T, D in MATRIX:
        n = stream_len(M, T, D)
        h = row_edge_taps(T, M, False)
        for i16 in (False, True):
            r = signal(oracle, n, i16)
            model = rpfb_ref.model_c64(h, r, M, D)
            assert np.all(model[:, 0].imag == 0) and np.all(model[:, M // 2].imag == 0)
            l2, mx = oracle.err_metrics(rpfb_ref.iq(model), rpfb_ref.iq(rpfb_ref.fold_f64(h, r, M, D)))
            for name, v in (("l2", l2), ("max", mx)):
                worst[name] = max(worst[name], (v, (M, T, D, i16)))
            assert l2 <= TOL / 2 and mx <= TOL / 2, (M, T, D, i16, l2, mx)
    print("rpfb model worst l2=%.3g at %s, max=%.3g at %s" % (worst["l2"] + worst["max"]))


TAPS = np.ones(16 * 128 + 1, dtype=np.float32)


def _init(L, fir, channels=128, hop=64, first_bin=0, bins=65, T=131, max_samples=256, cfg=True, taps=True, ctx=True):
    c = fir.RpfbConfig(channels, hop, first_bin, bins)
    p = ctypes.c_void_p(0x1234)
    ok = L.if_fir_rpfb_init(ctypes.byref(p) if ctx else None, ctypes.byref(c) if cfg else None,
                            TAPS.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if taps else None, T, max_samples, 0)
    return ok, p.value, L.if_fir_rpfb_last_error(None).decode()


@pytest.mark.parametrize("kw,message", [
    (dict(channels=64), "channels must be 128, 256, 512, 1024, 2048, 4096 or 8192 (got 64)"),
    (dict(channels=96), "channels must be 128, 256, 512, 1024, 2048, 4096 or 8192 (got 96)"),
    (dict(channels=16384), "channels must be 128, 256, 512, 1024, 2048, 4096 or 8192 (got 16384)"),
    (dict(channels=0), "channels must be 128, 256, 512, 1024, 2048, 4096 or 8192 (got 0)"),
    (dict(T=0), "taps must be 1..2048 = 16 x channels (got 0)"),
    (dict(T=16 * 128 + 1), "taps must be 1..2048 = 16 x channels (got 2049)"),
    (dict(hop=0), "hop must be 1..128 (got 0)"),
    (dict(hop=129), "hop must be 1..128 (got 129)"),
    (dict(first_bin=1, bins=65), "the span needs 1 <= ulBins and ulFirstBin + ulBins <= 65 = channels / 2 + 1 (got 1, 65)"),
    (dict(first_bin=0, bins=66), "the span needs 1 <= ulBins and ulFirstBin + ulBins <= 65 = channels / 2 + 1 (got 0, 66)"),
    (dict(first_bin=3, bins=0), "the span needs 1 <= ulBins and ulFirstBin + ulBins <= 65 = channels / 2 + 1 (got 3, 0)"),
    (dict(max_samples=0), "ullMaxSamples must be 1..2^40 (got 0)"),
    (dict(max_samples=2 ** 40 + 1), "ullMaxSamples must be 1..2^40 (got 1099511627777)"),
    (dict(cfg=False), "pCfg is NULL"),
    (dict(taps=False), "taps must be 1..2048 = 16 x channels (got 131), pfTaps is NULL"),
])
def test_init_refusals_name_the_limit_and_the_value(fir, kw, message):
    """every refused argument: status 0, no context, the message names the limit and what was received (no GPU is touched:
    the arguments are checked before the device)"""
    ok, ctx, err = _init(fir.lib(), fir, **kw)
    assert ok == 0 and ctx is None
    assert err == "if_fir_rpfb_init: " + message


def test_null_arguments(fir):
    L = fir.lib()
    ok, _, err = _init(L, fir, ctx=False)
    assert ok == 0 and err == "if_fir_rpfb_init: ppCtx is NULL"
    assert L.if_fir_rpfb_frame_count(None, 1 << 20) == 0
    assert L.if_fir_rpfb_reset(None) == 0 and L.if_fir_rpfb_set_input_format(None, 0) == 0 and L.if_fir_rpfb_set_stream(None, None) == 0
    assert L.if_fir_rpfb_synchronize(None) == 0
    assert L.if_fir_rpfb_process(None, None, None, 0, None) == 0 and L.if_fir_rpfb_process_device(None, None, None, 0, None) == 0
    L.if_fir_rpfb_destroy(None)
    assert fir.dev_lib().if_fir_debug_rpfb_config(None, 0, None, 0) == 0
    with pytest.raises(fir.IfFirError, match="unsigned"):
        fir.IfFirRpfb(TAPS[:100], 128, first_bin=-1)


def test_rpfb_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_rpfb.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_rpfb.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # seven sizes and the carry, float32 and int16 input
    assert len(names) == 16 and sum("rpfb_kernel" in n for n in names) == 14 and sum("rpfb_carry_kernel" in n for n in names) == 2, names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 16
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 16
