"""bench.py's own N-rank launcher (CPU, gloo): `bench.py --gpus 2` must start
two ranks itself when no external launcher set WORLD_SIZE, reduce over both
and print n_gpus 2.  The --stub engine replaces the GPU (fixed-size cuts in
numpy) so only the launch, barrier and max/sum reductions are exercised."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True,
                       text=True, timeout=300, env=env, cwd=ROOT)
    return r


def test_bench_launches_two_ranks_itself():
    """Default: `value` is config 2 per GPU (weak scaling, the same per-GPU work
    as the N=1 line), plus the config-4 strong-scaling sub-object with rank 0's
    whole-batch time from the same run as its N=1 denominator."""
    r = _run(["--gpus", "2", "--stub", "--full", "--steps", "2", "--warmup", "1", "--stream-bytes", str(1 << 20),
              "--batch-streams", "6", "--batch-stream-bytes", "65536", "--config4-steps", "2", "--cpu-seconds", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    line = lines[0]
    assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    assert line["config"]["workload"].startswith("config2")
    assert line["config"]["bytes_per_gpu"] == 1 << 20 and line["config"]["streams_per_gpu"] == 1
    assert line["config"]["chunks_total"] == 2 * ((1 << 20) // 8192)
    assert line["value"] > 0
    c4 = line["config4"]
    assert c4["scaling"] == "strong" and c4["workload"].startswith("config4")
    assert c4["streams_per_gpu"] == 3 and c4["chunks_total"] == 6 * (65536 // 8192)
    assert c4["value"] > 0 and c4["n1_value_rank0_alone"] > 0
    assert abs(c4["strong_scaling_efficiency"] - c4["value"] / (2 * c4["n1_value_rank0_alone"])) < 1e-9


def test_bench_batch_value_is_config4():
    r = _run(["--gpus", "2", "--stub", "--workload", "batch", "--steps", "2", "--warmup", "1",
              "--batch-streams", "6", "--batch-stream-bytes", "65536", "--cpu-seconds", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    line = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")][0]
    assert line["scaling"] == "strong" and line["config"]["workload"].startswith("config4")
    assert line["config"]["streams_per_gpu"] == 3 and "config4" not in line


def test_bench_single_rank_has_config4():
    r = _run(["--gpus", "1", "--stub", "--full", "--steps", "2", "--warmup", "1", "--stream-bytes", str(1 << 20),
              "--batch-streams", "4", "--batch-stream-bytes", "65536", "--cpu-seconds", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    line = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")][0]
    assert line["n_gpus"] == 1 and line["config4"]["streams_per_gpu"] == 4
    assert "strong_scaling_efficiency" not in line["config4"]


def test_world_size_mismatch_fails_loudly():
    r = _run(["--gpus", "2", "--stub", "--steps", "1"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """Without --full the run is set-up, warm-up, the --steps timed steps and
    the line: no other leg.  --dump-outputs writes the last step's first[] as
    float64 (the stub has no chunk list)."""
    import numpy as np
    d = tmp_path / "dump"
    r = _run(["--gpus", "1", "--stub", "--steps", "3", "--warmup", "1", "--stream-bytes", str(1 << 20),
              "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    for k in ("config4", "config5", "sustained", "latency_sync", "host_path", "sweep", "other_chunkers",
              "config3", "parity_vs_oracle"):
        assert k not in line, k
    assert line["cpu_baseline"] is None and line["roofline"]["achievable_GBps"] is None
    first = np.load(d / "first.npy")
    assert first.dtype == np.float64 and first.tolist() == [0.0, float((1 << 20) // 8192)]
    assert sorted(p.name for p in d.iterdir()) == ["first.npy"]


def test_dump_outputs_samples_a_list_over_its_budget(tmp_path, monkeypatch):
    """A chunk list larger than the dump budget is cut to a fixed seeded sample
    of its rows (the same rows on every run), their indices beside them; rank
    r > 0 writes its own files."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = 5000
    w = bench.Work([n * 8192])
    w.out = torch.arange(2 * (n + 7), dtype=torch.int64).reshape(-1, 2)  # 7 rows of capacity past first[-1]
    first = np.array([0, n], dtype=np.uint64)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 24 * 1000 + 16)
    bench.dump_outputs(str(tmp_path / "a"), w, first, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), w, first, 1, 2)
    rows, chunks = np.load(tmp_path / "a" / "chunks_rows.npy"), np.load(tmp_path / "a" / "chunks.npy")
    assert rows.dtype == chunks.dtype == np.float64 and rows.shape == (1000,) and chunks.shape == (1000, 2)
    assert (np.diff(rows) > 0).all() and rows[-1] < n
    assert np.array_equal(chunks, np.stack([2 * rows, 2 * rows + 1], axis=1))
    bench.dump_outputs(str(tmp_path / "a2"), w, first, 0, 1)
    assert np.array_equal(rows, np.load(tmp_path / "a2" / "chunks_rows.npy"))
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["chunks_rank1.npy", "chunks_rows_rank1.npy",
                                                                  "first_rank1.npy"]
    assert np.load(tmp_path / "b" / "chunks_rank1.npy").shape == (499, 2)  # half the budget, less first[]
    monkeypatch.setattr(bench, "DUMP_BUDGET", 60_000_000)
    bench.dump_outputs(str(tmp_path / "c"), w, first, 0, 1)
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == ["chunks.npy", "first.npy"]
    assert np.array_equal(np.load(tmp_path / "c" / "chunks.npy"), w.out[:n].numpy().astype(np.float64))
