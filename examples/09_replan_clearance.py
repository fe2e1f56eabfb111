#!/usr/bin/env python3
"""Replanning in flight, then the certificate: are the new paths clear of the paths that stay, and of each other?

Example 08's swarm of eight drones, rest-to-rest paths of six segments.  At 40 % of its own flight each of three drones
gets three new waypoints (swarm.replan).  The new paths start at t_r on the swarm's clock and have three segments where
the swarm has six, so msnap_pair_clearance cannot take them.  swarm.certify_replan runs every (new, old) and
(new, new) pair through msnap_cross_clearance with the offsets t_r and reports, per replanned drone, a proven lower
bound of its distance to everything else while both fly.

    python examples/09_replan_clearance.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, certify_replan, replan  # noqa: E402

N, M, RADIUS = 8, 6, 0.15
IDX = [1, 4, 6]
wp, t = synthetic.swarm(8, N, M)
rng = np.random.default_rng(8)
with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    coef, dur = coef.clone(), dur.clone()
    idx = torch.tensor(IDX, device=dev)
    t_r = 0.4 * dur[idx].sum(dim=1)
    old_c, old_d = coef[idx].contiguous(), dur[idx].contiguous()
    pos_r, _ = comp.eval_state(old_c, old_d, t_r)
    steps = torch.from_numpy(rng.uniform(-2.0, 2.0, (len(IDX), 3, 4))).to(dev)
    t_new = torch.tensor([1.5, 3.0, 4.5], dtype=torch.float64, device=dev)
    new_coef, new_dur, new_status, _ = replan(comp, old_c, old_d, t_r, pos_r[:, None, :] + torch.cumsum(steps, dim=1), t_new)
    new_coef, new_dur, new_status = new_coef.clone(), new_dur.clone(), new_status.clone()
    res = certify_replan(comp, coef, dur, idx, t_r, new_coef, new_dur, RADIUS, new_status=new_status)
    # a drone against the path it has just left: the two agree at t_r, so the window's start is the minimum
    own = torch.arange(len(IDX), device=dev, dtype=torch.int32)
    md, tm, lower, _ = comp.cross_clearance(new_coef, new_dur, old_c, old_d, torch.stack([own, own], dim=1), t0_a=t_r)
    torch.cuda.synchronize()
    print(f"{res.pairs.shape[0]} pairs certified ({len(IDX)} replanned drones x {N} drones), radius {RADIUS} m")
    for k, d in enumerate(IDX):
        mine = (res.pairs[:, 0] == d) | (res.pair_new_new & (res.pairs[:, 1] == d))
        p = int(torch.nonzero(mine)[res.pair_lower[mine].argmin()])
        other = [int(x) for x in res.pairs[p].tolist() if int(x) != d][0]
        verdict = "HIT" if bool(res.hit[k]) else ("undecided" if bool(res.undecided[k]) else "clear")
        print(f"drone {d}: replanned at t = {float(t_r[k]):.3f} s; certified distance to every other drone >= "
              f"{float(res.certified_lower[k]):.6f} m (closest: drone {other}{' on its new path' if bool(res.pair_new_new[p]) else ''}, "
              f"{float(res.pair_min_dist[p]):.6f} m at t = {float(res.pair_t_min[p]):.4f} s) -> {verdict}; "
              f"against the path it left: {float(md[k]):.1e} m at t = {float(tm[k]):.3f} s")
