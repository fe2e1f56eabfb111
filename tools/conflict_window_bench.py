#!/usr/bin/env python3
"""Conflict windows timed with events on the stream, against the cross clearance on the same pairs: device-resident
buffers, 3 warm-up calls, then the median of 7 single timed calls, the two entries timed alternately.

The load is tools/cross_clearance_bench.py's "random": the 65 536 random pairs of the 4096 x 10 swarm, the swarm against
itself with NULL offsets.  threshold = the median min_dist of those pairs, so that about half of them are in conflict;
t_res = 1e-6 s.  msnap_cross_conflict_window_device walks every interval twice (forward and backward) and a later
interval cannot know that an earlier one already holds the first conflict, so no ratio is promised: the measured ratio
is reported, with the mean and maximum nodes per live lane and direction from the NumPy restatement
(tests/conflict_exact.py) on the first 2048 pairs.  One JSON line, appended to profiles/conflict_window_bench.jsonl,
with the sources' csrc hash.

    python tools/conflict_window_bench.py
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conflict_exact as KE  # noqa: E402
from drone_path_planning_python_amd import Context, _lib, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute  # noqa: E402

dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "conflict_window_bench.jsonl")
T_RES = 1e-6
RESTATED_PAIRS = 2048


def timed_alternately(fns, warm=3, reps=7):
    """{name: (median, min, max) us}: one timed call of each in turn, `reps` rounds"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: (round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)) for k, v in us.items()}


def main():
    with Context(0, 7, 16) as ctx:
        comp = DeviceCompute(ctx, torch)
        wp, t = synthetic.swarm(47, 4096, 10)
        coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        coef, dur = coef.clone(), dur.clone()
        N, M = dur.shape
        rng = np.random.default_rng(47)
        a = rng.integers(0, 4096, size=65536)
        b = (a + rng.integers(1, 4096, size=65536)) % 4096
        pairs = torch.from_numpy(np.stack([a, b], axis=1).astype(np.int32)).to(dev)
        P = pairs.shape[0]
        f64 = lambda: torch.empty((P,), dtype=torch.float64, device=dev)      # noqa: E731
        i32 = lambda: torch.empty((P,), dtype=torch.int32, device=dev)        # noqa: E731
        oc = [f64(), f64(), f64(), i32()]
        ctx.cross_clearance_device(N, M, coef, dur, None, N, M, coef, dur, None, P, pairs, *oc)
        torch.cuda.synchronize()
        threshold = float(oc[0].median())
        ow = [f64() for _ in range(6)] + [i32()]
        t = timed_alternately({
            "clearance": lambda: ctx.cross_clearance_device(N, M, coef, dur, None, N, M, coef, dur, None, P, pairs, *oc),
            "window": lambda: ctx.cross_conflict_window_device(N, M, coef, dur, None, N, M, coef, dur, None, P, pairs,
                                                               threshold, T_RES, *ow)})
        assert int(ow[6].abs().sum()) == 0 and int(oc[3].abs().sum()) == 0
        cu, tf, df, tl, dl, cf = (x.cpu().numpy() for x in ow[:6])
        found = np.isfinite(tf)
        # a pair is in conflict exactly when its attained minimum is below the threshold (up to rounding at the level)
        agree = found == (oc[0].cpu().numpy() < threshold)
        closed = (tf[found] - cu[found] <= T_RES * 1.001) & (cf[found] - tl[found] <= T_RES * 1.001)
        undecided = ~found & np.isfinite(cu)
        stats = {}
        sub = pairs[:RESTATED_PAIRS].cpu().numpy()
        c, d = coef.cpu().numpy(), dur.cpu().numpy()
        r = KE.fp64_conflict_window(c, d, None, c, d, None, sub, threshold, T_RES, stats=stats)
        assert (np.isfinite(r[1]) == found[:RESTATED_PAIRS]).mean() > 0.999
        nodes = stats["nodes"]
        row = {"load": "random", "order": 7, "drones": N, "segments": M, "pairs": P, "lanes": P * (2 * M - 1),
               "threshold_m": threshold, "t_res_s": T_RES,
               "cross_clearance_device_us": t["clearance"][0], "cross_clearance_us_min_max": t["clearance"][1:],
               "cross_conflict_window_device_us": t["window"][0], "cross_conflict_window_us_min_max": t["window"][1:],
               "ratio_to_cross_clearance": round(t["window"][0] / t["clearance"][0], 3),
               "pairs_in_conflict": int(found.sum()), "pairs_undecided": int(undecided.sum()),
               "pairs_agreeing_with_min_dist": int(agree.sum()), "searches_closed": int(closed.sum()),
               "restated_pairs": RESTATED_PAIRS, "restated_live_lanes": int(stats["lanes"]),
               "nodes_per_live_lane_and_direction_mean": round(float(nodes.mean()), 2),
               "nodes_per_live_lane_and_direction_max": int(nodes.max()), "reps": 7,
               "csrc": _lib.csrc_sha(), "device": torch.cuda.get_device_name(0)}
    with open(OUT, "a") as f:
        line = json.dumps(row)
        print(line, flush=True)
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
