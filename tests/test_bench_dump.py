"""bench.py --dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy in float64, so that two
builds can be compared output for output.  CPU: the writer and its fixed sample of an output above the size limit;
GPU: the headline's dump against the C oracle on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT, norm_rel


def test_dump_writes_every_output_in_float64(tmp_path):
    coef = torch.arange(6 * 2 * 3, dtype=torch.float64).reshape(6, 2, 3)
    status = torch.tensor([0, 1, 0, -3, 0, 2], dtype=torch.int32)
    names = bench.dump_outputs(str(tmp_path), {"coef": coef, "status": status})
    assert names == ["coef", "status"] and sorted(os.listdir(tmp_path)) == ["coef.npy", "status.npy"]
    for name, x in (("coef", coef), ("status", status)):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, x.numpy())


def test_dump_above_the_limit_writes_a_fixed_sample_of_drones(tmp_path):
    n = 1000
    coef = torch.randn(n, 4, 8, dtype=torch.float64)
    dur = torch.rand(n, 4, dtype=torch.float64)
    per_drone = 8 * (4 * 8 + 4)
    limit = 100 * per_drone
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"coef": coef, "dur": dur}, limit=limit)
    got = {f: np.load(tmp_path / "a" / f) for f in ("coef.npy", "dur.npy", "drone_index.npy")}
    assert sum(a.nbytes for a in got.values()) <= limit
    idx = got["drone_index.npy"].astype(np.int64)
    assert len(idx) > 90 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(got["coef.npy"], coef.numpy()[idx]) and np.array_equal(got["dur.npy"], dur.numpy()[idx])
    for f, a in got.items():      # the same sample on every run
        assert np.array_equal(np.load(tmp_path / "b" / f), a)


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """--steps sets the timed steps; the dump is the headline batch's coefficients, durations and status, equal to
    the C oracle's on the same seeded inputs"""
    import c_oracle
    from drone_path_planning_python_amd.synthetic import swarm
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--no-configs", "--no-saturated", "--no-shared-grid", "--no-concurrent", "--no-end-to-end",
                        "--no-cpu-baseline", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["steps"] == 7 and d["ms_per_step"] > 0
    assert sorted(os.listdir(out)) == ["coef.npy", "dur.npy", "status.npy"]
    coef, dur, status = (np.load(out / f"{n}.npy") for n in ("coef", "dur", "status"))
    assert coef.dtype == dur.dtype == status.dtype == np.float64
    assert coef.shape == (256, 10, 4, 8) and dur.shape == (256, 10) and status.shape == (256,)
    assert not status.any()
    wp, t = swarm(2, 256, 10)
    ref, rdur, _, _ = c_oracle.solve_batch(wp, t, ncoef=8, faithful=False, n_threads=4)
    assert norm_rel(coef, ref) <= 1e-6
    assert np.array_equal(dur, rdur)
