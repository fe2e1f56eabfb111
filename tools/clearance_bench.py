#!/usr/bin/env python3
"""Pairwise clearance timed with events on the stream: msnap_pair_clearance_device, device-resident buffers, 3 warm-up
calls, then the median of 7 single timed calls, at two loads:

  random     65 536 random pairs of a 4096 x 10 swarm with per-drone times;
  pipeline   the pair list swarm.certify_clearance produces on the 4096-drone formation swarm (BASELINE.json
             configs[2]), with the list's length and |U| beside it, and the whole pipeline's wall time with the pair
             filter in torch (`pair_filter="torch"`) and on the GPU ("auto": msnap_formation_near_pairs), alternating;
  near_pairs msnap_formation_near_pairs_device alone on that swarm's positions (4096 drones, and 16 384: four copies
             100 m apart), with the pipeline's speeds and gap, against the pairwise pass (msnap_formation_collide_device,
             with and without its broad phase) on the same positions, the three timed alternately.

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
from drone_path_planning_python_amd.swarm import COMPARE_MARGIN, PEAK_MARGIN, DeviceCompute, certify_clearance  # noqa: E402

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


def time_near_pairs(ctx, comp, pos, speed, radius, gap, margin):
    """The near-pairs call alone against the pairwise pass on the same positions."""
    N, S = pos.shape[0], pos.shape[1]
    cap = max(4096, 8 * N)
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    dist = torch.empty((cap,), dtype=torch.float64, device=dev)
    found = torch.zeros((1,), dtype=torch.int64, device=dev)

    def k5(no_cull):
        def run():
            ctx.set_option("collide_no_cull", no_cull)
            comp.collide(pos, 0, pos, radius)
        return run
    t = timed_alternately({
        "near_pairs": lambda: ctx.near_pairs_device(N, S, pos, 2.0 * radius, speed, gap, margin, cap, pairs, dist, found),
        "collide": k5(0), "collide_all_pairs": k5(1)})
    ctx.set_option("collide_no_cull", 0)
    return {"load": "near_pairs", "drones": N, "samples": S, "pairs_found": int(found.item()), "capacity": cap,
            "near_pairs_device_us": t["near_pairs"][0], "near_pairs_us_min_max": t["near_pairs"][1:],
            "formation_collide_device_us": t["collide"][0], "formation_collide_us_min_max": t["collide"][1:],
            "formation_collide_all_pairs_us": t["collide_all_pairs"][0],
            "formation_collide_all_pairs_us_min_max": t["collide_all_pairs"][1:],
            "ratio_to_all_pairs": round(t["near_pairs"][0] / t["collide_all_pairs"][0], 3), "reps": 7}


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
        run = lambda f="auto": certify_clearance(comp, coef, dur, synthetic.DRONE_RADIUS, synthetic.SAMPLE_DT, S,      # noqa: E731
                                                 pair_filter=f)
        res = run()
        assert torch.equal(res.pairs, run("torch").pairs)
        torch.cuda.synchronize()
        wall = {"torch": [], "auto": []}
        for _ in range(5):
            for f in wall:
                t0 = time.perf_counter()
                run(f)
                torch.cuda.synchronize()
                wall[f].append((time.perf_counter() - t0) * 1e3)
        row = {"load": "pipeline", "order": 7, "drones": wp.shape[0], "segments": m - 1, "uncertain_drones": res.n_uncertain,
               "gap_s": res.gap, "sampled_hits": int(res.sampled_hit.sum()), "certified_hits": int(res.hit.sum()),
               "undecided": int(res.undecided.sum()),
               "certify_clearance_wall_ms_median": round(statistics.median(wall["auto"]), 2),
               "certify_clearance_wall_ms_median_torch_filter": round(statistics.median(wall["torch"]), 2)}
        if res.pairs.shape[0]:
            row.update(time_list(ctx, coef, dur, res.pairs))
        else:
            row["pairs"] = 0
        rows.append(row)
        # the near-pairs call alone, on the whole swarm's positions with the pipeline's numbers
        pos = comp.sample(coef, dur, synthetic.SAMPLE_DT, S).clone()
        peak, _, _ = comp.dynamic_peaks(coef, dur)
        v = (peak[:, 0] * (1.0 + PEAK_MARGIN)).contiguous()
        rows.append(time_near_pairs(ctx, comp, pos, v, synthetic.DRONE_RADIUS, res.gap, COMPARE_MARGIN))
        shift = torch.zeros((4, 1, 1, 3), dtype=torch.float64, device=dev)
        shift[:, 0, 0, 0] = 100.0 * torch.arange(4, dtype=torch.float64, device=dev)
        pos4 = (pos[None] + shift).reshape(4 * pos.shape[0], S, 3).contiguous()
        rows.append(time_near_pairs(ctx, comp, pos4, v.repeat(4).contiguous(), synthetic.DRONE_RADIUS, res.gap,
                                    COMPARE_MARGIN))
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
