"""The N>1 bench path on the HIP engine (-m gpu): `bench.py --gpus 2` starts two
ranks itself; on a one-GPU box both share cuda:0 (--share-device) and the
timing / byte reductions run over gloo (--dist-backend gloo) -- on an 8-GPU node
the driver runs the same path with one GPU per rank over RCCL.  Each rank chunks
its own block of the config-4 batch with no data-path collective and checks its
first streams bit-exact against the oracle (--rank-parity, min over ranks)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_on_hip_engine():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-device",
                        "--rank-parity", "--workload", "batch", "--batch-streams", "8",
                        "--batch-stream-bytes", str(8 << 20), "--steps", "2", "--warmup", "1", "--cpu-seconds", "0"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["n_gpus"] == 2 and line["scaling"] == "strong"
    assert line["config"]["streams_per_gpu"] == 4
    assert line["parity_all_ranks"] is True
    assert line["value"] > 0


def test_two_ranks_default_stream_workload():
    """The driver's own N>1 command shape (`bench.py --gpus N`, default
    `--workload stream`, default gloo reductions) with small sizes: `value` is
    config 2 per GPU (weak), the config-4 leg runs its N>1 branch (rank 0 re-times
    the whole batch alone: the strong-scaling denominator) and the config-5 leg
    runs every walk rule at avg 2/8/64 KiB across both ranks, checked against
    the oracle."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-device", "--full",
                        "--rank-parity", "--stream-bytes", str(64 << 20), "--batch-streams", "8",
                        "--batch-stream-bytes", str(8 << 20), "--config4-steps", "2", "--config5-streams", "4",
                        "--config5-stream-bytes", str(32 << 20), "--config5-check", str(8 << 20), "--steps", "2",
                        "--warmup", "1", "--cpu-seconds", "0"],
                       capture_output=True, text=True, timeout=400, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["config"]["workload"].startswith("config2")
    assert line["parity_all_ranks"] is True and line["value"] > 0
    c4 = line["config4"]
    assert c4["streams_per_gpu"] == 4 and c4["parity_vs_oracle"] is True
    assert c4["strong_scaling_efficiency"] > 0 and c4["n1_value_rank0_alone"] > 0
    c5 = line["config5"]
    assert c5["streams_per_gpu"] == 2 and len(c5["lines"]) == 12
    assert all(v["parity_vs_oracle"] is True for v in c5["lines"].values()), c5["lines"]


def test_eight_ranks_real_shard_counts():
    """The driver's 8-GPU shapes rehearsed on one GPU: `bench.py --gpus 8` with
    the real shard COUNTS (config 4: 1024 streams = 128 per rank; config 5: 16
    streams = 2 per rank) at small sizes, every rank sharing cuda:0, every
    rank's first streams checked against the oracle (min over ranks; config
    5: the whole first streams of ranks 0 and 7), the config-4 strong-scaling efficiency reported (rank 0 re-times the whole
    1024-stream batch alone)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--share-device", "--full",
                        "--rank-parity", "--stream-bytes", str(24 << 20), "--batch-streams", "1024",
                        "--batch-stream-bytes", str(1 << 20), "--config4-steps", "1", "--config5-streams", "16",
                        "--config5-stream-bytes", str(8 << 20), "--steps", "2",
                        "--warmup", "1", "--cpu-seconds", "0"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["n_gpus"] == 8 and line["scaling"] == "weak"
    assert line["parity_all_ranks"] is True and line["value"] > 0
    c4 = line["config4"]
    assert c4["streams_per_gpu"] == 128 and c4["parity_vs_oracle"] is True
    assert c4["strong_scaling_efficiency"] > 0 and c4["n1_value_rank0_alone"] > 0
    c5 = line["config5"]
    assert c5["streams_per_gpu"] == 2 and len(c5["lines"]) == 12
    assert all(v["parity_vs_oracle"] is True for v in c5["lines"].values()), c5["lines"]
    assert c5["parity_definition"].startswith("the whole first stream of rank 0 and of rank 7")
    assert "summary" in line and line["summary"]["value_GiBps"] == line["value"]


def test_plain_run_dumps_the_last_steps_chunk_list(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` (no --full):
    only the headline is measured, and DIR holds what the last timed step
    wrote -- first[] and the Chunk{offset, length} list, float64 -- equal to
    the oracle's chunks of the same seeded stream."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    n = (24 << 20) + 77
    d = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--stream-bytes", str(n), "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("config4", "config5", "sustained", "latency_sync", "host_path", "sweep", "other_chunkers",
              "config3", "parity_vs_oracle"):
        assert k not in line, k
    assert line["cpu_baseline"] is None and line["roofline"]["achievable_GBps"] is None
    ref = oracle.fastcdc(oracle.splitmix64_bytes(n, 1), 4096, 8192, 16384)
    chunks, first = np.load(d / "chunks.npy"), np.load(d / "first.npy")
    assert chunks.dtype == np.float64 and first.dtype == np.float64
    assert first.tolist() == [0.0, float(len(ref))] and line["config"]["chunks_total"] == len(ref)
    assert chunks.shape == ref.shape and np.array_equal(chunks, ref.astype(np.float64))
