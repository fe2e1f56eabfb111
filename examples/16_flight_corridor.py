#!/usr/bin/env python3
"""A safe flight corridor through the hole in the wall: certify a path against a chain of convex polytopes.

The corridor is three boxes built from the vertices of env-scene-hole.stl: the free space in front of the wall, the hole
extruded through the wall's thickness (and half a metre beyond it on both sides, so that the boxes overlap), and the
free space behind the wall.  swarm.certify_corridor (msnap_halfspace_window) proves that a path stays in one box until
it is inside the next, and says when and through which plane a path leaves the corridor; no mesh pass is needed.

Three paths: example 15's replan along the hole's axis at radius 0.1 and at radius 0.125 -- the second beside
swarm.mesh_conflict_windows' window for the same path -- and example 06's drone that tunnels through the wall.  A box
corridor is more cautious than the distance to the mesh: a path that cuts the corner behind the rim leaves the hole's box
sideways before it is past the wall by a radius, although its distance to the rim's edge stays above the radius.  The
verdicts are printed, whatever they are.

    python examples/16_flight_corridor.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, stl  # noqa: E402
from drone_path_planning_python_amd.swarm import (DeviceCompute, certify_corridor, certify_mesh_clearance,  # noqa: E402
                                                  default_sample_count, latest_replan_time, mesh_conflict_windows,
                                                  replan)

DT, MARGIN, TOTAL, REACH = 0.1, 0.3, 1.1, 0.5
VERDICT = ["INSIDE", "OUTSIDE", "UNDECIDED", "FAILED"]
tris_h = np.ascontiguousarray(stl.load_stl(os.path.join(ROOT, "tests", "golden", "env-scene-hole.stl")), dtype=np.float64)


def box(lo, hi):
    """the six half-spaces n.x <= b of an axis-aligned box"""
    rows = []
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        rows += [[*e, hi[a]], [*(-e), -lo[a]]]
    return rows


def corridor_through_the_hole(tris):
    """planes [18, 4] and poly_offsets: the wall is a slab in y with one rectangular hole, whose vertices are those off
    the slab's outline"""
    v = tris.reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rim = v[(np.abs(v[:, 0]) < hi[0]) & (np.abs(v[:, 2]) < hi[2])]
    big = 1e3
    planes = (box((-big, -big, -big), (big, lo[1], big))
              + box((rim[:, 0].min(), lo[1] - REACH, rim[:, 2].min()), (rim[:, 0].max(), hi[1] + REACH, rim[:, 2].max()))
              + box((-big, hi[1], -big), (big, big, big)))
    return np.array(planes), [0, 6, 12, 18]


def report(name, res, planes):
    d = 0
    line = f"{name}: {VERDICT[int(res.verdict[d])]}, proven inside the corridor until {float(res.proven_until[d]):.6f} s; "
    line += "hand-over times " + ", ".join("-" if np.isnan(h) else f"{h:.6f}" for h in res.handover[d].tolist())
    if int(res.stage[d]) >= 0:
        p = int(res.plane[d])
        line += (f"; stopped in stage {int(res.stage[d])} at the plane n = {planes[p, :3].tolist()}: first outside it at "
                 f"{float(res.first_conflict[d]):.6f} s (n.p = {float(res.value[d]):.6f})")
    print(line)


with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    tris = torch.from_numpy(tris_h).to(dev)
    planes_h, off = corridor_through_the_hole(tris_h)
    planes = torch.from_numpy(planes_h).to(dev)
    # example 06's drone: 4.4 m in 1.1 s through the wall at x = 2.5
    wp = np.zeros((1, 2, 4))
    wp[0, :, 0], wp[0, :, 1] = 2.5, [-2.2, 2.2]
    t = np.array([[0.0, TOTAL]])
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    coef, dur, status = coef.clone(), dur.clone(), status.clone()
    report("through the wall, radius 0.125", certify_corridor(comp, coef, dur, planes, off, [0, 1, 2], radius=0.125,
                                                              status=status), planes_h)
    # example 15's replan: leave that path before its first conflict, pass the wall along the hole's axis
    res = certify_mesh_clearance(comp, coef, dur, tris, 0.125, DT, default_sample_count(TOTAL, DT), status=status)
    t_r = latest_replan_time(mesh_conflict_windows(comp, res, coef, dur, tris, 0.125), MARGIN)
    wp_new = torch.tensor([[[0.0, -0.8, 0.0, 0.0], [0.0, 0.8, 0.0, 0.0], [2.5, 2.2, 0.0, 0.0]]], dtype=torch.float64,
                          device=dev)
    t_new = torch.tensor([0.8, 1.3, 2.2], dtype=torch.float64, device=dev)
    new_coef, new_dur, new_status, _ = replan(comp, coef, dur, t_r, wp_new, t_new)
    new_coef, new_dur, new_status = new_coef.clone(), new_dur.clone(), new_status.clone()
    total = float(new_dur.sum())
    for radius in (0.1, 0.125):
        cor = certify_corridor(comp, new_coef, new_dur, planes, off, [0, 1, 2], radius=radius, status=new_status)
        report(f"replanned through the hole, radius {radius}", cor, planes_h)
        rep = certify_mesh_clearance(comp, new_coef, new_dur, tris, radius, DT, default_sample_count(total, DT),
                                     status=new_status)
        win = mesh_conflict_windows(comp, rep, new_coef, new_dur, tris, radius)
        torch.cuda.synchronize()
        print(f"    the mesh at radius {radius}: certified distance >= {float(rep.certified_lower[0]):.4f} m (closest "
              f"{float(rep.min_dist[0]):.4f} m); window: clear until {float(win.t_clear_until[0]):.6f}, in conflict "
              f"{float(win.t_first[0]):.6f} .. {float(win.t_last[0]):.6f}, clear from {float(win.t_clear_from[0]):.6f}")
