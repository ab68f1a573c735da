"""bench.py's command line: a plain run is the timed C1 steps and the headline
line only, `--full` adds every other measurement, `--dump-outputs DIR` writes
what the last timed step returned."""
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "cpu_baseline", "c1_sweep", "sparse_conv", "pointpillars", "kpconv", "randlanet",
             "ops_roofline")


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    """dump_outputs: small arrays whole, an array over its share of the budget
    as the same seeded sample on every call (first and last entry kept);
    integers as float64, floats in their own precision."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 8 * 1000)  # 1000 float64 / 2000 float32 entries per array
    Res = namedtuple("res", ["neighbors_index", "neighbors_row_splits", "neighbors_distance"])
    idx = torch.arange(50000, dtype=torch.int32) * 7 % 1013
    res = Res(idx, torch.arange(0, 901, dtype=torch.int64) * (1 << 28), torch.empty(0))
    bench.dump_outputs(res, str(tmp_path / "e"))  # an empty field (no distances asked for) writes no file
    assert sorted(os.listdir(tmp_path / "e")) == ["neighbors_index.npy", "neighbors_row_splits.npy"]
    res = res._replace(neighbors_distance=torch.linspace(0, 1, 1500))
    bench.dump_outputs(res, str(tmp_path / "a"))
    bench.dump_outputs(res, str(tmp_path / "b"))
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in Res._fields}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in Res._fields)
    for n in Res._fields:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy"))
    assert a["neighbors_index"].dtype == np.float64 and 900 < a["neighbors_index"].size <= 1000
    assert a["neighbors_index"][0] == idx[0] and a["neighbors_index"][-1] == idx[-1]
    assert set(a["neighbors_index"]) <= set(idx.tolist())
    assert a["neighbors_row_splits"].dtype == np.float64  # whole, exact beyond 2^32
    assert np.array_equal(a["neighbors_row_splits"], res.neighbors_row_splits.numpy().astype(np.float64))
    assert a["neighbors_distance"].dtype == np.float32
    assert np.array_equal(a["neighbors_distance"], res.neighbors_distance.numpy())
    assert sum(v.nbytes for v in a.values()) <= 3 * 8 * 1000


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return lines[0]


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_the_last_step(cuda, tmp_path):
    """`bench.py --steps N --warmup W --dump-outputs DIR` (two scenes): the
    line has the headline fields and none of the --full ones; DIR holds what
    dump_outputs writes for layers.FixedRadiusSearch's result on the bench batch."""
    import bench
    from o3dml_amd import layers
    rec = _bench("--steps", "3", "--warmup", "1", "--scenes", "2", "--dump-outputs", str(tmp_path / "d"))
    assert all(k in rec for k in HEADLINE) and not any(k in rec for k in FULL_ONLY)
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 2 * bench.N_POINTS / rec["ms_per_step"] / 1e3) <= 0.01 * rec["value"]
    pts, rs = bench.make_batch(0, 2, cuda)
    ref = layers.FixedRadiusSearch()(pts, pts, bench.RADIUS, rs, rs)
    bench.dump_outputs(ref, str(tmp_path / "ref"))  # the index list is over the budget: the same sample of it
    kept = [n for n in ref._fields if getattr(ref, n).numel()]
    assert kept == ["neighbors_index", "neighbors_row_splits"]  # no distances asked for: that field is empty
    assert sorted(os.listdir(tmp_path / "d")) == sorted(f"{n}.npy" for n in kept)
    for n in kept:
        got = np.load(tmp_path / "d" / f"{n}.npy")
        assert got.dtype in (np.float32, np.float64)
        assert np.array_equal(got, np.load(tmp_path / "ref" / f"{n}.npy")), n
    assert np.array_equal(np.load(tmp_path / "d" / "neighbors_row_splits.npy"),
                          ref.neighbors_row_splits.cpu().numpy().astype(np.float64))  # under the budget: whole
    assert rec["config"]["pairs_per_step_rank0"] == np.load(tmp_path / "d" / "neighbors_row_splits.npy")[-1]


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements(cuda):
    """`--full` (its legs at their smallest or off): the same headline fields
    plus the search kernels' roofline and the per-op rooflines."""
    rec = _bench("--full", "--steps", "2", "--warmup", "1", "--scenes", "1", "--no-cpu-baseline", "--kernel-reps", "1",
                 "--op-reps", "1", "--randla-frames", "0", "--kpconv-steps", "0", "--pointpillars-steps", "0",
                 "--sparse-conv-reps", "0", "--sweep-reps", "0")
    assert all(k in rec for k in HEADLINE)
    assert set(rec["roofline"]["kernel_ms_all"]) == set(__import__("bench").KERNELS)
    assert rec["roofline"]["kernel_ms"] > 0 and rec["cpu_baseline"] is None
    assert set(rec["ops_roofline"]) == {"knn", "grid_subsample", "voxelize"}
