#!/usr/bin/env python3
"""Mesh clearance timed with events on the stream (tools/clearance_bench.py's method: device-resident buffers, 3 warm-up
calls, the median of 7 single timed calls), beside msnap_mesh_sweep_device on the same swarm, the two timed alternately:

  whole     a 4096 x 20 swarm with per-drone times against the 68 triangles of the two scenes
            (tests/golden/env-scene-hole.stl, env-scene-ltu-experiment.stl);
  pipeline  the drones swarm.certify_mesh_clearance keeps of that swarm (radius 0.1, 0.1 s samples), the kernel on
            that list alone, and the whole pipeline's wall time.

One JSON line per load, appended to profiles/clearance_bench.jsonl, with the sources' csrc hash.

    python tools/mesh_clearance_bench.py
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clearance_bench import OUT, dev, timed_alternately  # noqa: E402
from drone_path_planning_python_amd import Context, _lib, stl, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, certify_mesh_clearance  # noqa: E402

RADIUS = 0.1


def time_call(ctx, comp, coef, dur, tris, pos):
    n, M = dur.shape
    md, tm, lower = (torch.empty((n,), dtype=torch.float64, device=dev) for _ in range(3))
    tri, st = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(2))
    t = timed_alternately({
        "clearance": lambda: ctx.mesh_clearance_device(n, M, coef, dur, tris.shape[0], tris, md, tm, tri, lower, st),
        "sweep": lambda: comp.mesh(pos, tris, RADIUS)})
    assert int(st.abs().sum()) == 0 and bool((lower <= md).all())
    return {"drones": n, "segments": M, "triangles": int(tris.shape[0]), "samples": int(pos.shape[1]),
            "mesh_clearance_device_us": t["clearance"][0], "mesh_clearance_us_min_max": t["clearance"][1:],
            "mesh_sweep_device_us": t["sweep"][0], "mesh_sweep_us_min_max": t["sweep"][1:],
            "certified_hits": int((md < RADIUS).sum()), "undecided": int(((md >= RADIUS) & (lower < RADIUS)).sum()),
            "reps": 7}


def main():
    g = os.path.join(ROOT, "tests", "golden")
    tris_h = np.concatenate([stl.load_stl(os.path.join(g, "env-scene-hole.stl")),
                             stl.load_stl(os.path.join(g, "env-scene-ltu-experiment.stl"))])
    rows = []
    with Context(0, 7, 32) as ctx:
        comp = DeviceCompute(ctx, torch)
        tris = torch.from_numpy(tris_h).to(dev)
        wp, t = synthetic.swarm(48, 4096, 20)
        coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        assert int(st.abs().sum()) == 0
        S = int(np.ceil(float(dur.sum(dim=1).max()) / synthetic.SAMPLE_DT))
        pos = comp.sample(coef, dur, synthetic.SAMPLE_DT, S).clone()
        rows.append({"load": "mesh_whole", "order": 7, **time_call(ctx, comp, coef, dur, tris, pos)})
        res = certify_mesh_clearance(comp, coef, dur, tris, RADIUS, synthetic.SAMPLE_DT, S)
        torch.cuda.synchronize()
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            certify_mesh_clearance(comp, coef, dur, tris, RADIUS, synthetic.SAMPLE_DT, S)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        keep = torch.nonzero(~res.cleared_by_sampling, as_tuple=True)[0]
        row = {"load": "mesh_pipeline", "order": 7, "uncertain_drones": res.n_uncertain, "gap_s": res.gap,
               "sampled_hits": int(res.sampled_hit.sum()), "pipeline_hits": int(res.hit.sum()),
               "pipeline_undecided": int(res.undecided.sum()),
               "certify_mesh_clearance_wall_ms_median": round(statistics.median(wall), 2)}
        if keep.numel():
            row.update(time_call(ctx, comp, coef[keep].contiguous(), dur[keep].contiguous(), tris, pos[keep].contiguous()))
        rows.append(row)
    with open(OUT, "a") as f:
        for r in rows:
            r["csrc"] = _lib.csrc_sha()
            r["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
