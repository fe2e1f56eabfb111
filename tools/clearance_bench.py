#!/usr/bin/env python3
"""Pairwise clearance timed with events on the stream: msnap_pair_clearance_device, device-resident buffers, 3 warm-up
calls, then the median of 7 single timed calls, at two loads:

  random     65 536 random pairs of a 4096 x 10 swarm with per-drone times;
  pipeline   the pair list swarm.certify_clearance produces on the 4096-drone formation swarm (BASELINE.json
             configs[2]), with the list's length and |U| beside it, and the whole pipeline's wall time.

With each: the mean and maximum nodes per lane from the NumPy restatement (tests/clearance_exact.py).  One JSON line
per load, appended to profiles/clearance_bench.jsonl, with the sources' csrc hash.

    python tools/clearance_bench.py
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clearance_exact as CE  # noqa: E402
from drone_path_planning_python_amd import Context, _lib, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, certify_clearance  # noqa: E402

dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "clearance_bench.jsonl")


def timed(fn, warm=3, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us), max(us)


def time_list(ctx, coef, dur, pairs):
    N, M = dur.shape
    P = pairs.shape[0]
    out = [torch.empty((P,), dtype=torch.float64, device=dev) for _ in range(3)]
    st = torch.empty((P,), dtype=torch.int32, device=dev)
    med, lo, hi = timed(lambda: ctx.pair_clearance_device(N, M, coef, dur, P, pairs, out[0], out[1], out[2], st))
    assert int(st.abs().sum()) == 0
    stats = {}
    rmd, _, rlower = CE.fp64_clearance(coef.cpu().numpy(), dur.cpu().numpy(), pairs.cpu().numpy(), stats=stats)
    np.testing.assert_allclose(out[0].cpu().numpy(), rmd, rtol=1e-9, atol=CE.ABS_ROUND)
    nodes = stats["nodes"]
    return {"pairs": P, "lanes": P * (2 * M - 1), "live_lanes": int(stats["lanes"]),
            "pair_clearance_device_us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "reps": 7,
            "nodes_per_live_lane_mean": round(float(nodes.mean()), 2), "nodes_per_live_lane_max": int(nodes.max()),
            "capped_lanes": int(stats["capped"].sum()), "min_dist_min": float(rmd.min())}


def main():
    rows = []
    with Context(0, 7, 16) as ctx:
        comp = DeviceCompute(ctx, torch)
        # random pairs of a swarm with per-drone times
        wp, t = synthetic.swarm(47, 4096, 10)
        coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        rng = np.random.default_rng(47)
        a = rng.integers(0, 4096, size=65536)
        b = (a + rng.integers(1, 4096, size=65536)) % 4096
        pairs = torch.from_numpy(np.stack([a, b], axis=1).astype(np.int32)).to(dev)
        rows.append({"load": "random", "order": 7, "drones": 4096, "segments": 10, **time_list(ctx, coef, dur, pairs)})
        # the formation swarm through the pipeline
        rb, off, tg = synthetic.formation_config(2)
        G, m, _ = rb.shape
        poses = ctx.formation_transform(rb.reshape(G * m, 7), off)
        wp = synthetic.formation_waypoints(poses, G)
        coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(tg).to(dev))
        S = synthetic.formation_sample_count(tg)
        run = lambda: certify_clearance(comp, coef, dur, synthetic.DRONE_RADIUS, synthetic.SAMPLE_DT, S)      # noqa: E731
        res = run()
        torch.cuda.synchronize()
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        row = {"load": "pipeline", "order": 7, "drones": wp.shape[0], "segments": m - 1, "uncertain_drones": res.n_uncertain,
               "gap_s": res.gap, "sampled_hits": int(res.sampled_hit.sum()), "certified_hits": int(res.hit.sum()),
               "undecided": int(res.undecided.sum()), "certify_clearance_wall_ms_median": round(statistics.median(wall), 2)}
        if res.pairs.shape[0]:
            row.update(time_list(ctx, coef, dur, res.pairs))
        else:
            row["pairs"] = 0
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
