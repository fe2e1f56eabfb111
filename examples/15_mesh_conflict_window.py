#!/usr/bin/env python3
"""From when is a drone too close to an obstacle -- and the hand-over time of a replan that starts before it.

Example 06's rest-to-rest drone tunnels through the wall of env-scene-hole.stl at x = 2.5, 4.4 m in 1.1 s.
certify_mesh_clearance says that it hits and where it is closest; t_min lies inside the violation.
swarm.mesh_conflict_windows (msnap_mesh_conflict_window) certifies from when until when the drone is closer to the mesh
than the radius -- the wall is hollow, 0.5 m between its faces, so the first conflict is with the front face and the last
with the back face; swarm.latest_replan_time turns the window's start into the hand-over time t_r of a replan that begins
`margin` seconds earlier.  The drone is replanned at that t_r through two waypoints on the hole's axis, one in front of
the wall and one behind it, and on to its old end, and certify_mesh_clearance is run again on the new path: its outcome
is printed, whatever it is.

    python examples/15_mesh_conflict_window.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, stl  # noqa: E402
from drone_path_planning_python_amd.swarm import (DeviceCompute, certify_mesh_clearance, default_sample_count,  # noqa: E402
                                                  latest_replan_time, mesh_conflict_windows, replan)

RADIUS, DT, MARGIN, TOTAL = 0.125, 0.1, 0.3, 1.1
tris_h = stl.load_stl(os.path.join(ROOT, "tests", "golden", "env-scene-hole.stl"))


def verdict_of(res, d=0):
    return "HIT" if bool(res.hit[d]) else ("undecided" if bool(res.undecided[d]) else "clear")


with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    tris = torch.from_numpy(np.ascontiguousarray(tris_h)).to(dev)
    wp = np.zeros((1, 2, 4))
    wp[0, :, 0], wp[0, :, 1] = 2.5, [-2.2, 2.2]
    t = np.array([[0.0, TOTAL]])
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    coef, dur = coef.clone(), dur.clone()
    res = certify_mesh_clearance(comp, coef, dur, tris, RADIUS, DT, default_sample_count(TOTAL, DT), status=status)
    print(f"certify_mesh_clearance: {verdict_of(res)}, sampled hit {bool(res.sampled_hit[0])}; closest "
          f"{float(res.min_dist[0]):.3e} m at t_min = {float(res.t_min[0]):.4f} s against triangle {int(res.triangle[0])}")
    win = mesh_conflict_windows(comp, res, coef, dur, tris, RADIUS)
    print(f"conflict window at radius {RADIUS} m: proven clear on [0, {float(win.t_clear_until[0]):.6f}), in conflict from "
          f"{float(win.t_first[0]):.6f} s ({float(win.d_first[0]):.6f} m, triangle {int(win.tri_first[0])}) to "
          f"{float(win.t_last[0]):.6f} s ({float(win.d_last[0]):.6f} m, triangle {int(win.tri_last[0])}), proven clear on "
          f"({float(win.t_clear_from[0]):.6f}, {TOTAL}]")
    t_r = latest_replan_time(win, MARGIN)
    print(f"latest hand-over time with a margin of {MARGIN} s: {float(t_r[0]):.6f} s")
    # the drone leaves its path at t_r for the hole's axis, passes the wall along it, then flies on to its old end
    wp_new = torch.tensor([[[0.0, -0.8, 0.0, 0.0], [0.0, 0.8, 0.0, 0.0], [2.5, 2.2, 0.0, 0.0]]], dtype=torch.float64,
                          device=dev)
    t_new = torch.tensor([0.8, 1.3, 2.2], dtype=torch.float64, device=dev)
    new_coef, new_dur, new_status, _ = replan(comp, coef, dur, t_r, wp_new, t_new)
    new_coef, new_dur, new_status = new_coef.clone(), new_dur.clone(), new_status.clone()
    total = float(new_dur.sum())
    rep = certify_mesh_clearance(comp, new_coef, new_dur, tris, RADIUS, DT, default_sample_count(total, DT),
                                 status=new_status)
    rwin = mesh_conflict_windows(comp, rep, new_coef, new_dur, tris, RADIUS)
    torch.cuda.synchronize()
    print(f"replanned at t_r = {float(t_r[0]):.6f} s through the hole: certified distance to the mesh >= "
          f"{float(rep.certified_lower[0]):.4f} m (closest {float(rep.min_dist[0]):.4f} m) -> {verdict_of(rep)}; first "
          f"conflict on the new path, on its own clock: {float(rwin.first_conflict[0])}")
