"""CPU tests of bench.py's launch path: `python3 bench.py --gpus N` must work as the driver runs it (no launcher around
it): the parent spawns the ranks as a child process and relays rank 0's single JSON line.  --dry-run replaces the
filter by a sleep (gloo, no GPU, no oracle), so only the plumbing is exercised here."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(*argv, env_drop=("WORLD_SIZE", "RANK", "LOCAL_RANK")):
    env = {k: v for k, v in os.environ.items() if k not in env_drop}
    p = subprocess.run([sys.executable, BENCH] + list(argv), capture_output=True, text=True, env=env, timeout=300)
    return p


def test_self_launch_argv_is_the_drivers_command():
    sys.path.insert(0, ROOT)
    import bench
    argv = bench.self_launch_argv(4, ["--gpus", "4", "--steps", "7"], 29777)
    assert argv[0] == sys.executable and argv[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in argv and argv[argv.index("--nproc-per-node") + 1] == "4"
    assert argv[argv.index("--master-addr") + 1] == "127.0.0.1" and argv[argv.index("--master-port") + 1] == "29777"
    assert argv[-5:] == [BENCH, "--gpus", "4", "--steps", "7"]


def test_gpus2_without_a_launcher_prints_exactly_one_json_line():
    p = run_bench("--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["warmup"] == 1 and line["dry_run"] is True
    assert line["scaling"] == "weak" and line["config"]["channels"] == 2 and line["value"] > 0


def test_channels_form_is_strong_scaling():
    p = run_bench("--gpus", "2", "--channels", "8", "--dry-run", "--steps", "2", "--warmup", "0")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["scaling"] == "strong" and line["config"]["channels"] == 8 and line["config"]["channels_on_rank0"] == 4


def test_single_gpu_dry_run_and_failing_child_exit_code():
    p = run_bench("--dry-run", "--steps", "2", "--warmup", "0")
    assert p.returncode == 0 and json.loads(p.stdout.strip())["n_gpus"] == 1
    # a child that fails (fewer channels than GPUs) must surface as a non-zero exit code and no JSON line
    p = run_bench("--gpus", "2", "--channels", "1", "--dry-run")
    assert p.returncode != 0 and not p.stdout.strip()


def test_scatter_legs_are_rehearsed_over_gloo():
    """VERDICT r2 #6a: `--scatter` (channel_shard) and `--scatter-mc` (the C front's transfer plan: chunks, groups, two-slot
    staging) run their control flow with real processes over gloo in --dry-run, so the first 8-GPU run is not the first
    execution; rank 0 checks that every channel's bytes came back in place."""
    for gpus in ("2", "3"):
        p = run_bench("--gpus", gpus, "--dry-run", "--steps", "2", "--warmup", "0", "--scatter", "--scatter-mc")
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        sg, mc = line["extra"]["scatter_gather"], line["extra"]["scatter_gather_mc"]
        assert sg["ok"] is True and sg["channels"] == int(gpus)
        assert mc["ok"] is True and mc["chunks"] == 3 and mc["channels"] == int(gpus) + 1 and mc["groups"] == 7
        # the record the first multi-GPU box must produce in one go -- per-rank times, bytes through
        # ncclSend / ncclRecv, bit-identity per channel -- has a fixed schema, filled here from the gloo rehearsal; the bytes
        # its formula states per rank are the bytes of that rank's transfer plan
        chk = mc["multi_gpu_check"]
        assert tuple(chk) == bench_keys() and chk["world"] == int(gpus) and chk["channels"] == int(gpus) + 1
        assert len(chk["per_rank_ms"]) == chk["calls"] == 1 and len(chk["per_rank_ms"][0]) == int(gpus)
        assert len(chk["bytes_sent_per_rank"]) == len(chk["bytes_received_per_rank"]) == int(gpus)
        assert sum(chk["bytes_sent_per_rank"]) == sum(chk["bytes_received_per_rank"]) == chk["bytes_through_send_recv"] > 0
        assert chk["channels_identical"] == [True] * (int(gpus) + 1) and chk["ok"] is True
        assert mc["plan_bytes_agree_with_record"] is True


def bench_keys():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_keys", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MULTI_GPU_CHECK_KEYS


def test_multi_gpu_check_record_schema_and_bytes():
    """The record's byte accounting for BASELINE configs[3] (8 channels x 2^28 samples, decimation 4, 8 ranks): seven channels
    travel, 2 GiB each way in and 512 MiB back, plus seven 4-byte status words."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_rec", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 1 << 28
    rec = bench.multi_gpu_check_record(8, 8, n, 255, 4, "rccl", [[10.0] * 8, [9.0, 9.5] + [9.1] * 6], [True] * 8)
    assert tuple(rec) == bench.MULTI_GPU_CHECK_KEYS and rec["ok"] is True and rec["end_to_end_ms"] == 9.5
    assert rec["bytes_sent_per_rank"][0] == 7 * n * 8 and rec["bytes_received_per_rank"][0] == 7 * (n // 4) * 8 + 7 * 4
    assert rec["bytes_sent_per_rank"][3] == (n // 4) * 8 + 4 and rec["bytes_received_per_rank"][3] == n * 8
    assert rec["bytes_through_send_recv"] == 7 * n * 8 + 7 * (n // 4) * 8 + 28
    rec = bench.multi_gpu_check_record(2, 3, 1000, 255, 4, "x", [[1.0, 2.0]], [True, False, True])
    assert rec["ok"] is False


def test_dump_index_is_fixed_sorted_and_within_budget():
    """--dump-outputs writes the last step's outputs at these indices: the same ones in every run, inside the output,
    unique, with the first and last outputs of the step, and with the outputs of all channels within the 64 MB limit."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_for_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert np.array_equal(bench.dump_index(1000, 1), np.arange(1000))
    for m, channels in ((1 << 26, 1), (1 << 28, 1), (1 << 26, 8), (3 << 20, 1), ((3 << 20) + 1, 1), (1 << 26, 4000)):
        idx = bench.dump_index(m, channels)
        assert np.array_equal(idx, bench.dump_index(m, channels))
        assert idx[0] == 0 and idx[-1] == m - 1 and (np.diff(idx) > 0).all()
        assert idx.size * 8 * (channels + 1) <= min(bench.DUMP_BYTES, 64 << 20)
        assert idx.size >= bench.DUMP_BYTES // (8 * (channels + 1)) - 1


def test_extras_first_needs_full():
    p = run_bench("--extras-first", "--dry-run")
    assert p.returncode != 0 and "--full" in p.stderr and not p.stdout.strip()
    p = run_bench("--steps", "0", "--dry-run")
    assert p.returncode != 0 and not p.stdout.strip()
