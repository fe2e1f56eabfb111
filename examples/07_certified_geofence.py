#!/usr/bin/env python3
"""Certified geofence: a minimum-snap fit through waypoints inside the workspace that leaves it between them.

The reference plans its rigid-body path inside x in [-2.2, 2.2], y in [2.8, 5.0], z in [0.5, 2.5] and then fits a
polynomial through the planned poses.  The four waypoints below lie inside that box; the fit passes the wall at x = 2.2
by more than a metre at t = 3 s.  msnap_path_extent gives the attained reach with its time and a proven bound per
direction; swarm.certify_geofence sorts the drones into inside / outside / undecided against a box and half-spaces;
swarm.geofence_windows (msnap_halfspace_window) says from when until when the path is outside.

    python examples/07_certified_geofence.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context  # noqa: E402
from drone_path_planning_python_amd.swarm import (GEOFENCE_OUTSIDE, DeviceCompute, certify_geofence,  # noqa: E402
                                                  geofence_windows)

LO, HI = [-2.2, 2.8, 0.5], [2.2, 5.0, 2.5]
wp = np.zeros((1, 4, 4))
wp[0, :, :3] = [(0.0, 3.0, 1.0), (2.1, 3.9, 1.5), (2.1, 4.8, 1.5), (0.0, 4.8, 2.0)]
t = np.array([0.0, 2.0, 4.0, 6.0])
NAMES = ["+x", "-x", "+y", "-y", "+z", "-z"]
for order in (7, 9):
    with Context(device_id=0, order=order, max_segments=16) as ctx:
        coef, dur, status = ctx.solve_batch(wp, t)
        axes = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
        ext, t_ext, upper, st = ctx.path_extent(coef, dur, axes)
        lo = 0.0 - upper[0, 1::2]
        print(f"order {order}: certified box x [{lo[0]:.4f}, {upper[0, 0]:.4f}] y [{lo[1]:.4f}, {upper[0, 2]:.4f}] "
              f"z [{lo[2]:.4f}, {upper[0, 4]:.4f}]")
        comp = DeviceCompute(ctx, torch)
        tc, td = torch.from_numpy(coef).cuda(), torch.from_numpy(dur).cuda()
        res = certify_geofence(comp, tc, td, lo=LO, hi=HI, status=torch.from_numpy(status))
        k = int(res.worst[0])
        n = res.normals[k].tolist()
        wall = NAMES[[i for i in range(6) if axes[i].tolist() == n][0]]
        verdict = "outside" if int(res.verdict[0]) == GEOFENCE_OUTSIDE else str(int(res.verdict[0]))
        print(f"order {order}: {verdict}: through the {wall} wall (limit {float(res.limits[k]):.2f}) by "
              f"{float(res.excess[0]):.4f} m at t = {float(res.t_worst[0]):.4f} s")
        # from when until when: the window during which x > 2.2 (msnap_halfspace_window)
        win = geofence_windows(comp, res, tc, td)
        q = int((win.queries[:, 1] == int(win.first_broken[0])).nonzero()[0])
        print(f"order {order}: x > {HI[0]} from {float(win.t_first[q]):.6f} s to {float(win.t_last[q]):.6f} s; proven inside "
              f"that wall on [0, {float(win.t_inside_until[q]):.6f}) and ({float(win.t_inside_from[q]):.6f}, {float(td.sum()):.1f}]; "
              f"inside every wall until {float(win.inside_until[0]):.6f} s and from {float(win.inside_from[0]):.6f} s on")
