"""The polyphase filter bank's host side (no GPU): its C ABI in the header, the libraries and the binding; the call planning, the
tap table and the bin places of qo-100-tools_amd/csrc/if_fir_pfb_plan.h through the stand-alone checker
tests/c/pfb_plan_check.cpp, against Python-integer arithmetic; the fold form of tests/pfb_ref.py against the definition and the
project's float64 oracle; the complex64 model against half the GPU test's bound; the compiled kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_ref
from matrix_util import TOL, row_edge_taps, signal
from test_pfb_gpu import MATRIX, stream_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
PFB_ABI = {"if_fir_pfb_init", "if_fir_pfb_destroy", "if_fir_pfb_reset", "if_fir_pfb_set_input_format", "if_fir_pfb_set_stream",
           "if_fir_pfb_synchronize", "if_fir_pfb_last_error", "if_fir_pfb_frame_count", "if_fir_pfb_process", "if_fir_pfb_process_device"}
PFB_DEV = {"if_fir_debug_pfb_config"}
POSITIONS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 63, 2 ** 64 - 1001]
CHECKER = os.path.join(ROOT, "tests", "c", "pfb_plan_check.cpp")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pfb_plan_check") / "pfb_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, CHECKER, "-o", exe])
    return exe


def ask(exe, lines):
    """the answer lines (lists of words) to the request lines"""
    run = subprocess.run([exe, "query"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return [line.split() for line in run.stdout.splitlines()]


def test_header_declares_and_libraries_export_the_family(fir):
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_pfb_[a-z_]+)\s*\(", header))
    assert declared == PFB_ABI, declared ^ PFB_ABI
    assert "typedef struct if_fir_pfb if_fir_pfb_t;" in header and "} if_fir_pfb_config_t;" in header
    section = header[header.index("polyphase filter bank"):]
    assert "captured into a hipGraph are refused" in section
    for field in ("ulChannels", "ulHop", "lFirstBin", "ulBins"):
        assert field in section
    assert [name for name, _ in fir.PfbConfig._fields_] == ["ulChannels", "ulHop", "lFirstBin", "ulBins"]
    assert PFB_ABI <= set(fir.EXPORTS) and PFB_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert PFB_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert PFB_ABI <= product and PFB_ABI <= dev
    assert not (PFB_DEV & product) and PFB_DEV <= dev
    for name in ("frame_count", "process", "process_device", "reset", "set_input_format", "set_stream", "synchronize", "debug_config",
                 "__enter__", "__exit__"):
        assert hasattr(fir.IfFirPfb, name), name


def test_self_check(plan_check):
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("calls checked: OK"), run.stdout + run.stderr
    assert run.stdout.startswith("%d shapes, %d calls" % (7 * 7, 7 * 7 * 6 * 11 * 8)), run.stdout


def test_self_check_under_sanitizers(tmp_path):
    """tests/c/pfb_plan_check.cpp with -fsanitize=address,undefined, run as a program: the tap table into a heap buffer of
    exactly its size, the calls and the kernel's index algebra against 128-bit arithmetic"""
    exe = str(tmp_path / "pfb_plan_check_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, CHECKER, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("calls checked: OK"), run.stdout + run.stderr


def test_calls_equal_python_integers(plan_check):
    """frames, runs of frames, the first frame's offset, c mod M and the carry at every position x call size x (M, D, T) of a
    spread, against Python's integers; the refusal past 2^64"""
    rng = np.random.default_rng(5)
    lines, wants = [], []
    for M, T, D in MATRIX[::3] + ((64, 187, 17), (256, 2047, 255), (4096, 32668, 2048), (1024, 4095, 768)):
        (K, batch, group, lds, per_cu), = ([int(v) for v in row] for row in ask(plan_check, ["shape %d %d" % (M, T)]))
        assert K == -(-T // M) and batch == max(1, 1024 // M) and group == max(8, 2 * batch) and group % batch == 0
        assert lds == 8 * batch * M + 10 * M and 1 <= per_cu <= 8 and per_cu * lds <= 160 * 1024
        for c in POSITIONS + [int(rng.integers(0, 2 ** 63))]:
            for n in (0, 1, 2, D - 1, D, D + 1, 1000, 2 ** 20 + 7, int(rng.integers(0, 2 ** 36))):
                lines.append("call %d %d %d %d %d" % (c, n, M, D, T))
                if c + n >= 2 ** 64:
                    wants.append(["refused"])
                    continue
                frames = pfb_ref.frame_count(c, n, D)
                wants.append([str(v) for v in (frames, -(-frames // group), pfb_ref.first_offset(c, D), c % M, T - 1)])
    got = ask(plan_check, lines)
    assert len(got) == len(wants)
    bad = [(lines[k], got[k], wants[k]) for k in range(len(wants)) if got[k] != wants[k]]
    assert not bad, (len(bad), bad[:5])
    assert ["refused"] in wants
    assert ask(plan_check, ["call %d 2 64 3 5" % (2 ** 64 - 1), "call 5 10 64 0 5"]) == [["refused"], ["refused"]]


def test_summed_counts_over_any_split_equal_the_one_call_count():
    rng = np.random.default_rng(8)
    for D in (1, 2, 17, 64, 385, 4095, 4096):
        for start in (0, 5, 2 ** 32 - 5, 2 ** 40 + 12345):
            n = int(rng.integers(1, 50000))
            cuts = np.sort(rng.integers(0, n + 1, 6))
            pieces = np.diff(np.concatenate([[0], cuts, [n]]))
            c = start
            total = 0
            for s in pieces:
                total += pfb_ref.frame_count(c, int(s), D)
                c += int(s)
            assert total == pfb_ref.frame_count(start, n, D), (D, start, pieces)


@pytest.mark.parametrize("M,T", [(64, 1), (64, 63), (64, 64), (64, 65), (128, 187), (256, 16 * 256), (4096, 4097)])
def test_tap_table_is_the_rows_time_reversed(plan_check, M, T):
    rows = ask(plan_check, ["taps %d %d" % (M, T)])
    K = -(-T // M)
    got = np.array([[float(v) for v in row] for row in rows])
    assert got.shape == (K, M)
    h = np.zeros(K * M)
    h[:T] = np.arange(1, T + 1)
    assert np.array_equal(got, h.reshape(K, M)[:, ::-1])


def test_bin_places_follow_the_transforms_digit_order(plan_check):
    """place of channel k: its radix-4 digits (a last radix-2 one where M is an odd power of two) reversed, as psd_bin_position"""
    for M in pfb_ref.SIZES:
        lines = ["place %d %d %d" % (M, first, j) for first, j in ((0, 0), (0, 1), (0, M - 1), (-M // 2, 0), (-3, 5), (M - 1, 1), (77 % M, 0))]
        for line, (ch, place) in zip(lines, ask(plan_check, lines)):
            _, _, first, j = line.split()
            k = (int(first) + int(j)) % M
            assert int(ch) == k
            pos, length, kk = 0, M, k
            while length > 1:
                r = 4 if length >= 4 else 2
                pos += (kk % r) * (length // r)
                kk //= r
                length //= r
            assert int(place) == pos, (M, line)


SMALL = ((64, 187, 17), (64, 16 * 64, 64), (128, 3 * 128 - 5, 64), (256, 2047, 255), (512, 1017, 1), (256, 1, 256), (128, 100, 128))


@pytest.mark.parametrize("M,T,D", SMALL)
def test_fold_form_is_the_definition(oracle, M, T, D):
    """mix-filter-pick by the definition against the fold form, 1e-12 of the largest output; with a span, and at a position
    that is a multiple of neither D nor M"""
    n = min(stream_len(T, D), 40 * D + T // 4)
    h = row_edge_taps(T, M, False)
    x = signal(oracle, n, False)[1]
    for first, first_bin, bins in ((0, 0, M), (2 ** 40 + 12345, -3, 7)):
        want = pfb_ref.definition_f64(h, x, M, D, first_bin, bins, first)
        got = pfb_ref.fold_f64(h, x, M, D, first_bin, bins, first)
        assert got.shape == want.shape == (pfb_ref.frame_count(first, n, D), bins)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (first, np.max(np.abs(got - want)), np.max(np.abs(want)))


@pytest.mark.parametrize("M,T,D", MATRIX)
def test_fold_form_is_the_oracle_per_channel(oracle, M, T, D):
    """SPEC §13 defines channel k as the decimator with the NCO at k / M: on every shape of the GPU matrix, the channels 0, 1,
    5, M/2, M - 1 and a seeded one of the fold form equal oracle.fir_nco_f64 at phase word k 2^32 / M to 1e-12 of the largest
    output of the bank"""
    n = stream_len(T, D)
    h = row_edge_taps(T, M, False)
    x = signal(oracle, n, False)[1]
    got = pfb_ref.fold_f64(h, x, M, D)
    scale = np.max(np.abs(got))
    for k in (0, 1, 5, M // 2, M - 1, int(np.random.default_rng([M, T, D]).integers(M))):
        want = pfb_ref.channel_f64(oracle, h, x, M, D, k)
        assert want.shape == got[:, k].shape
        assert np.max(np.abs(got[:, k] - want)) <= 1e-12 * scale, (k, np.max(np.abs(got[:, k] - want)), scale)


def test_model_meets_half_the_bound(oracle):
    """tests/test_pfb_gpu.py asks nothing the arithmetic cannot deliver: the complex64 model (fold in float32 in SPEC §13's
    order, scipy.fft on complex64) stays within 5e-7 of float64, in both metrics over the whole output, on every shape of that
    matrix, float32 and int16 input."""
    worst = {"l2": (0.0, None), "max": (0.0, None)}
    for M, T, D in MATRIX:
        n = stream_len(T, D)
        h = row_edge_taps(T, M, False)
        for i16 in (False, True):
            x = signal(oracle, n, i16)[1]
            l2, mx = oracle.err_metrics(pfb_ref.iq(pfb_ref.model_c64(h, x, M, D)), pfb_ref.iq(pfb_ref.fold_f64(h, x, M, D)))
            for name, v in (("l2", l2), ("max", mx)):
                worst[name] = max(worst[name], (v, (M, T, D, i16)))
            assert l2 <= TOL / 2 and mx <= TOL / 2, (M, T, D, i16, l2, mx)
    print("pfb model worst l2=%.3g at %s, max=%.3g at %s" % (worst["l2"] + worst["max"]))


def test_pfb_kernels_use_no_scratch():
    path = os.path.join(CSRC, "if_fir_pfb.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_pfb.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # seven sizes and the carry, float32 and int16 input
    assert len(names) == 16 and sum("pfb_kernel" in n for n in names) == 14 and sum("pfb_carry_kernel" in n for n in names) == 2, names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 16
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 16
