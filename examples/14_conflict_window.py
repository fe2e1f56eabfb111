#!/usr/bin/env python3
"""From when is a pair too close -- and the hand-over time of a replan that still avoids it.

Example 05's two rest-to-rest drones cross at right angles, 2 m in 1.1 s each, through one point at t = 0.55 s.
certify_clearance says that they hit and where they are closest; t_min lies inside the violation.
swarm.conflict_windows (msnap_pair_conflict_window) certifies the interval during which the centres are closer than
2 radius; swarm.latest_replan_time turns its start into the hand-over time t_r of a replan that begins `margin`
seconds earlier.  Drone 1 is replanned at that t_r through one extra waypoint above the crossing point, and
swarm.certify_replan shows that the new path is clear of drone 0.

    python examples/14_conflict_window.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_path_planning_python_amd import Context, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import (DeviceCompute, certify_clearance, certify_replan, conflict_windows,  # noqa: E402
                                                  default_sample_count, latest_replan_time, replan, replan_conflict_windows)

RADIUS, MARGIN, TOTAL = 0.1, 0.5, 1.1
with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    wp = np.zeros((2, 2, 4))
    wp[0, :, 0] = [-1.0, 1.0]
    wp[1, :, 1] = [-1.0, 1.0]
    t = np.tile(np.array([0.0, TOTAL]), (2, 1))
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    coef, dur = coef.clone(), dur.clone()
    res = certify_clearance(comp, coef, dur, RADIUS, synthetic.SAMPLE_DT, default_sample_count(TOTAL, synthetic.SAMPLE_DT),
                            status=status)
    print(f"certify_clearance: hit {res.hit.tolist()}, closest {float(res.pair_min_dist[0]):.3e} m at "
          f"t_min = {float(res.pair_t_min[0]):.4f} s")
    win = conflict_windows(comp, res, coef, dur, RADIUS)
    print(f"conflict window of pair {win.pairs[0].tolist()} at 2 radius = {2 * RADIUS} m: proven clear on "
          f"[0, {float(win.t_clear_until[0]):.6f}), in conflict from {float(win.t_first[0]):.6f} s "
          f"({float(win.d_first[0]):.6f} m) to {float(win.t_last[0]):.6f} s ({float(win.d_last[0]):.6f} m), proven clear "
          f"on ({float(win.t_clear_from[0]):.6f}, {TOTAL}]")
    t_r = latest_replan_time(win, MARGIN)
    print(f"latest hand-over times with a margin of {MARGIN} s: {t_r.tolist()}")
    # drone 1 leaves its path at t_r for a waypoint 0.6 m above the crossing point, then flies on to its old end
    idx = torch.tensor([1], device=dev)
    wp_new = torch.tensor([[[0.0, 0.0, 0.6, 0.0], [0.0, 1.0, 0.0, 0.0]]], dtype=torch.float64, device=dev)
    t_new = torch.tensor([0.6, 1.3], dtype=torch.float64, device=dev)
    new_coef, new_dur, new_status, _ = replan(comp, coef[idx].contiguous(), dur[idx].contiguous(), t_r[idx], wp_new, t_new)
    new_coef, new_dur, new_status = new_coef.clone(), new_dur.clone(), new_status.clone()
    rep = certify_replan(comp, coef, dur, idx, t_r[idx], new_coef, new_dur, RADIUS, new_status=new_status)
    rwin = replan_conflict_windows(comp, coef, dur, idx, t_r[idx], new_coef, new_dur, RADIUS)
    torch.cuda.synchronize()
    verdict = "HIT" if bool(rep.hit[0]) else ("undecided" if bool(rep.undecided[0]) else "clear")
    print(f"drone 1 replanned at t_r = {float(t_r[1]):.6f} s: certified distance to drone 0 >= "
          f"{float(rep.certified_lower[0]):.4f} m (closest {float(rep.pair_min_dist[0]):.4f} m at "
          f"t = {float(rep.pair_t_min[0]):.4f} s) -> {verdict}; first conflict on the new path: "
          f"{float(rwin.first_conflict[0])}")
    assert verdict == "clear" and float(rwin.first_conflict[0]) == float("inf")
