"""The plain bench.py run and its --dump-outputs files: the sampling rule on the CPU (not gpu), one short plain run on the GPU.

A plain `bench.py --gpus 1 --steps K --warmup W` times exactly K steps (one batch) and prints one line; everything else it
measures or checks runs with --full. --dump-outputs writes what the timed path returned at its last step, at most 64 MB, the
same points in every run, so that two builds of the project can be compared output for output."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _outputs(torch, n, d):
    """Outputs whose entries name their own position: point i's dp is i, its sigma row i*d .. i*d+d-1, its tangent i*d*d .. ."""
    return (torch.arange(n * d * d, dtype=torch.float64), torch.arange(n * d, dtype=torch.float64), torch.arange(n, dtype=torch.float64))


def test_dump_writes_the_same_float64_sample_of_a_large_output_within_64_MB(tmp_path):
    import torch

    import bench

    n, d = bench.DUMP_POINTS + 4321, 6
    for run in ("a", "b"):
        bench.dump_outputs(torch, tmp_path / run, *_outputs(torch, n, d), d)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["C_tang.npy", "dp.npy", "sigma.npy"]
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64_000_000
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert got[f].dtype == np.float64
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f))      # the same points in every run
    idx = got["dp.npy"].astype(np.int64)
    m = bench.DUMP_POINTS
    assert idx.shape == (m,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert got["sigma.npy"].shape == (m, d) and np.array_equal(got["sigma.npy"], idx[:, None] * d + np.arange(d))
    assert got["C_tang.npy"].shape == (m, d, d)
    assert np.array_equal(got["C_tang.npy"], (idx[:, None] * d * d + np.arange(d * d)).reshape(m, d, d))


def test_dump_writes_every_point_of_a_small_output(tmp_path):
    import torch

    import bench

    n, d = 1000, 4
    bench.dump_outputs(torch, tmp_path, *_outputs(torch, n, d), d)
    assert np.array_equal(np.load(tmp_path / "dp.npy"), np.arange(n, dtype=np.float64))
    assert np.array_equal(np.load(tmp_path / "sigma.npy").reshape(-1), np.arange(n * d, dtype=np.float64))
    assert np.load(tmp_path / "C_tang.npy").shape == (n, d, d)


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_asked_for_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--nqp", "500000",
                          "--dump-outputs", str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1                              # one line, written once
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["batches"] == 1 and len(line["ms_per_step_batches"]) == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(line["config"]["points_per_gpu"] / (line["ms_per_step"] * 1e-3))
    assert line["unit"] == "qp/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert "cpu_baseline" not in line and "secondary_summary" not in line and "end_to_end_summary" not in line   # --full only
    d, n = line["config"]["d"], line["config"]["points_per_gpu"]
    C, s, dp = (np.load(tmp_path / f) for f in ("C_tang.npy", "sigma.npy", "dp.npy"))
    m = dp.shape[0]
    assert m == min(n, 1 << 17) and C.shape == (m, d, d) and s.shape == (m, d)
    assert np.isfinite(s).all() and (dp >= 0).all() and (dp > 0).any()      # the returned state: stresses, plastic increments
