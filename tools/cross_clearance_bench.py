#!/usr/bin/env python3
"""Cross clearance timed with events on the stream: device-resident buffers, 3 warm-up calls, then the median of 7
single timed calls, at two loads:

  random   the 65 536 random pairs of the 4096 x 10 swarm of tools/clearance_bench.py, the swarm against itself with
           zero offsets, through msnap_cross_clearance_device (offsets NULL, and an array of zeros) and through
           msnap_pair_clearance_device -- the yardstick, the same pairs and the same bits --, the three timed alternately;
  replan   an 8 x 4096 replan list: 8 new paths of 3 segments, each starting at 40 % of the flight, against all 4096
           paths of 10 segments.

With the replan load: the mean and maximum nodes per live lane from the NumPy restatement
(tests/cross_clearance_exact.py).  One JSON line per load, appended to profiles/cross_clearance_bench.jsonl, with the
sources' csrc hash.

    python tools/cross_clearance_bench.py
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
import cross_clearance_exact as XE  # noqa: E402
from drone_path_planning_python_amd import Context, _lib, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, replan  # noqa: E402

dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "cross_clearance_bench.jsonl")


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


def outputs(P):
    return [torch.empty((P,), dtype=torch.float64, device=dev) for _ in range(3)] + \
        [torch.empty((P,), dtype=torch.int32, device=dev)]


def main():
    rows = []
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
        zeros = torch.zeros((N,), dtype=torch.float64, device=dev)
        o9, ox, oz = outputs(P), outputs(P), outputs(P)
        t = timed_alternately({
            "pair": lambda: ctx.pair_clearance_device(N, M, coef, dur, P, pairs, *o9),
            "cross_null": lambda: ctx.cross_clearance_device(N, M, coef, dur, None, N, M, coef, dur, None, P, pairs, *ox),
            "cross_zeros": lambda: ctx.cross_clearance_device(N, M, coef, dur, zeros, N, M, coef, dur, zeros, P, pairs, *oz)})
        for x, y, z in zip(o9, ox, oz):
            assert torch.equal(x, y) and torch.equal(x, z)          # the yardstick's bits
        rows.append({"load": "random", "order": 7, "drones": N, "segments": M, "pairs": P, "lanes": P * (2 * M - 1),
                     "pair_clearance_device_us": t["pair"][0], "pair_clearance_us_min_max": t["pair"][1:],
                     "cross_clearance_device_us": t["cross_null"][0], "cross_clearance_us_min_max": t["cross_null"][1:],
                     "cross_clearance_device_zero_offsets_us": t["cross_zeros"][0],
                     "cross_clearance_zero_offsets_us_min_max": t["cross_zeros"][1:],
                     "ratio_to_pair_clearance": round(t["cross_null"][0] / t["pair"][0], 3), "reps": 7})
        # the replan list: 8 drones leave their paths at 40 % of the flight for three new waypoints, 1.5 s apart
        K = 8
        idx = torch.arange(0, N, N // K, device=dev)[:K]
        t_r = (0.4 * dur[idx].sum(dim=1)).contiguous()
        pos_r, _ = comp.eval_state(coef[idx].contiguous(), dur[idx].contiguous(), t_r)
        steps = torch.from_numpy(np.random.default_rng(8).uniform(-2.0, 2.0, (K, 3, 4))).to(dev)
        t_new = torch.tensor([1.5, 3.0, 4.5], dtype=torch.float64, device=dev)
        new_coef, new_dur, new_status, _ = replan(comp, coef[idx].contiguous(), dur[idx].contiguous(), t_r,
                                                  pos_r[:, None, :] + torch.cumsum(steps, dim=1), t_new)
        new_coef, new_dur = new_coef.clone(), new_dur.clone()
        assert int(new_status.abs().sum()) == 0
        Mn = new_dur.shape[1]
        rp = torch.stack([torch.arange(K, device=dev).repeat_interleave(N), torch.arange(N, device=dev).repeat(K)],
                         dim=1).to(torch.int32).contiguous()
        Pr = rp.shape[0]
        orp = outputs(Pr)
        t = timed_alternately({"replan": lambda: ctx.cross_clearance_device(K, Mn, new_coef, new_dur, t_r, N, M, coef, dur,
                                                                            None, Pr, rp, *orp)})
        assert int(orp[3].abs().sum()) == 0
        stats = {}
        rmd, _, _ = XE.fp64_cross_clearance(new_coef.cpu().numpy(), new_dur.cpu().numpy(), t_r.cpu().numpy(),
                                            coef.cpu().numpy(), dur.cpu().numpy(), None, rp.cpu().numpy(), stats=stats)
        np.testing.assert_allclose(orp[0].cpu().numpy(), rmd, rtol=1e-9, atol=1e-9)
        nodes = stats["nodes"]
        rows.append({"load": "replan", "order": 7, "new_paths": K, "new_segments": Mn, "drones": N, "segments": M,
                     "pairs": Pr, "lanes": Pr * (Mn + M - 1), "live_lanes": int(stats["lanes"]),
                     "cross_clearance_device_us": t["replan"][0], "cross_clearance_us_min_max": t["replan"][1:],
                     "nodes_per_live_lane_mean": round(float(nodes.mean()), 2), "nodes_per_live_lane_max": int(nodes.max()),
                     "capped_lanes": int(stats["capped"].sum()), "min_dist_min": float(rmd.min()), "reps": 7})
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
