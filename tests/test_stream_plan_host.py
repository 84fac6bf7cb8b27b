"""What the plan headers of the streaming families share (no GPU): qo-100-tools_amd/csrc/if_fir_stream_plan.h through the
stand-alone checker tests/c/stream_plan_check.cpp, built with the address and undefined-behaviour sanitizers and run directly;
and that every family's plan header takes these pieces from there."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
PLAN_FAMILIES = ("resamp", "psd", "ddc", "duc", "arb", "pfb", "synth")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_plan_check") / "stream_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "c", "stream_plan_check.cpp"), "-o", exe])
    return exe


def test_shared_plan_functions_against_their_restatements(plan_check):
    """the decimating call plan at every hop and position around 2^32, 2^63 and 2^64, workgroups per CU at every LDS size edge,
    the highest segment of every K, the NCO-shifted taps against long double, the size predicate at every size (the checker's
    header comment lists the grids), under the address and undefined-behaviour sanitizers"""
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    hops = list(range(1, 65)) + [65, 4095, 4096]
    calls = sum(7 * 15 + sum(1 for n in (0, 1, 2, D - 1, D, D + 1, 1000) if n) for D in hops)
    per_cu = sum(1 for kb in range(0, 2 * 160 + 1) for d in range(-2, 3) if kb * 1024 + d >= 1)
    mixes = 5 * 2 * (1 + 2 + 255)
    assert run.stdout == "%d checks: OK\n" % (calls + per_cu + 4096 + mixes + 8194 + 7), run.stdout


def test_plan_dump_lists_every_family(tmp_path):
    """tools/plan_dump.cpp, the listing two versions of the plan headers are compared by, builds against the headers as they
    are and walks every family's grid to the end, under the same sanitizers"""
    exe = str(tmp_path / "plan_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tools", "plan_dump.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and not run.stderr, run.stderr
    heads = {line.split(" ", 1)[0] for line in run.stdout.splitlines() if line[:1].isalpha()}
    assert heads == set(PLAN_FAMILIES), heads
    assert run.stdout.count("\n") > 600000 and run.stdout.splitlines()[-1].startswith("  channel index 4096 ")


def test_family_plan_headers_take_the_shared_pieces_from_one_place():
    """no family header states the CU's LDS size, the segment length, the highest-segment expression, the NCO-shifted taps'
    formula or a list of transform sizes of its own any more"""
    shared = open(os.path.join(CSRC, "if_fir_stream_plan.h")).read()
    assert len(re.findall(r"160 \* 1024", shared)) == 1 and "4294967296.0" in shared
    for family in PLAN_FAMILIES:
        text = open(os.path.join(CSRC, "if_fir_%s_plan.h" % family)).read()
        assert "if_fir_stream_plan.h" in text or "if_fir_psd_plan.h" in text, family
        for private in (r"160 \* 1024", r"_SEG = 16", r"\(K - 1\) / \w+\) \* ", r"cos\(a\)", r"== 1024 \|\| \w+ == 2048", r"__host__ __device__"):
            assert not re.search(private, text), (family, private)
