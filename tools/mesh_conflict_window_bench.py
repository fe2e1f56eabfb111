#!/usr/bin/env python3
"""Mesh conflict windows timed with events on the stream, beside the mesh clearance on the same inputs:
device-resident buffers, 3 warm-up calls, then the median of 7 single timed calls, the two entries timed alternately
(tools/conflict_window_bench.py's method).

Loads: 256 x 10 and 4096 x 20 swarms with per-drone times at order 7 against the 56 triangles of
tests/golden/env-scene-hole.stl.  The synthetic swarm's waypoints are moved to one side of the wall
(y -> 0.75 + 0.35 (y + 5): left where it is, every drone pierces the wall and the median min_dist is zero); the paths
between them still swing towards the wall and through it.  threshold = the median min_dist of the swarm, so that about
half of the drones are in conflict; t_res = 1e-6 s.  msnap_mesh_conflict_window_device walks every segment twice
(forward and backward) and a later segment cannot know that an earlier one already holds the first conflict, so no
ratio is promised: the measured ratio is reported, with the mean and maximum nodes per lane and direction from the NumPy restatement
(tests/mesh_conflict_exact.py) on the first 64 drones.  One JSON line per load, appended to
profiles/mesh_conflict_window_bench.jsonl, with the sources' csrc hash.

    python tools/mesh_conflict_window_bench.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_conflict_exact as MX  # noqa: E402
from conflict_window_bench import dev, timed_alternately  # noqa: E402
from drone_path_planning_python_amd import Context, _lib, stl, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mesh_conflict_window_bench.jsonl")
T_RES = 1e-6
RESTATED_DRONES = 64


def one_load(ctx, comp, tris, n, m, seed):
    wp, t = synthetic.swarm(seed, n, m)
    wp[..., 1] = 0.75 + 0.35 * (wp[..., 1] + 5.0)
    coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    assert int(st.abs().sum()) == 0
    coef, dur = coef.clone(), dur.clone()
    T = int(tris.shape[0])
    f64 = lambda: torch.empty((n,), dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda: torch.empty((n,), dtype=torch.int32, device=dev)        # noqa: E731
    oc = [f64(), f64(), i32(), f64(), i32()]
    ctx.mesh_clearance_device(n, m, coef, dur, T, tris, *oc)
    torch.cuda.synchronize()
    threshold = float(oc[0].median())
    ow = [f64(), f64(), f64(), i32(), f64(), f64(), i32(), f64(), i32()]
    t = timed_alternately({
        "clearance": lambda: ctx.mesh_clearance_device(n, m, coef, dur, T, tris, *oc),
        "window": lambda: ctx.mesh_conflict_window_device(n, m, coef, dur, T, tris, threshold, T_RES, *ow)})
    assert int(ow[8].abs().sum()) == 0 and int(oc[4].abs().sum()) == 0
    cu, tf, tl, cf = (ow[k].cpu().numpy() for k in (0, 1, 4, 7))
    found = np.isfinite(tf)
    # a drone is in conflict exactly when its attained minimum is below the threshold (up to rounding at the level)
    agree = found == (oc[0].cpu().numpy() < threshold)
    closed = (tf[found] - cu[found] <= T_RES * 1.001) & (cf[found] - tl[found] <= T_RES * 1.001)
    stats = {}
    k = min(RESTATED_DRONES, n)
    r = MX.fp64_mesh_conflict_window(coef[:k].cpu().numpy(), dur[:k].cpu().numpy(), tris.cpu().numpy(), threshold, T_RES,
                                     stats=stats)
    assert (np.isfinite(r[1]) == found[:k]).mean() > 0.95
    nodes = stats["nodes"]
    return {"load": "hole_scene", "order": 7, "drones": n, "segments": m, "lanes": n * m, "triangles": T,
            "threshold_m": threshold, "t_res_s": T_RES,
            "mesh_clearance_device_us": t["clearance"][0], "mesh_clearance_us_min_max": t["clearance"][1:],
            "mesh_conflict_window_device_us": t["window"][0], "mesh_conflict_window_us_min_max": t["window"][1:],
            "ratio_to_mesh_clearance": round(t["window"][0] / t["clearance"][0], 3),
            "drones_in_conflict": int(found.sum()), "drones_undecided": int((~found & np.isfinite(cu)).sum()),
            "drones_agreeing_with_min_dist": int(agree.sum()), "searches_closed": int(closed.sum()),
            "restated_drones": k, "nodes_per_lane_and_direction_mean": round(float(nodes.mean()), 2),
            "nodes_per_lane_and_direction_max": int(nodes.max()), "reps": 7,
            "csrc": _lib.csrc_sha(), "device": torch.cuda.get_device_name(0)}


def main():
    tris_h = stl.load_stl(os.path.join(ROOT, "tests", "golden", "env-scene-hole.stl"))
    with Context(0, 7, 32) as ctx:
        comp = DeviceCompute(ctx, torch)
        tris = torch.from_numpy(np.ascontiguousarray(tris_h)).to(dev)
        rows = [one_load(ctx, comp, tris, n, m, seed) for n, m, seed in ((256, 10, 51), (4096, 20, 52))]
    with open(OUT, "a") as f:
        for row in rows:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
