#!/usr/bin/env python3
"""Certified drone-vs-mesh clearance: a drone that tunnels through the wall of env-scene-hole.stl between two samples.

The wall is 0.5 m thick.  A rest-to-rest drone that flies 4.4 m in 1.1 s passes it at 8.75 m/s: the 0.1 s samples
either side of the wall are 0.19 m from its faces, so msnap_mesh_sweep reports no hit at radius 0.125.
msnap_mesh_clearance finds the crossing in continuous time; swarm.certify_mesh_clearance runs both for a small swarm.

    python examples/06_certified_mesh_clearance.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, stl  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, certify_mesh_clearance  # noqa: E402

RADIUS, DT, S = 0.125, 0.1, 11
tris = stl.load_stl(os.path.join(ROOT, "tests", "golden", "env-scene-hole.stl"))
with Context(device_id=0, order=7, max_segments=16) as ctx:
    xs = [2.5, 5.0, 0.0, -3.0]                      # beside the hole, past the wall, at the hole's centre, beside it again
    wp = np.zeros((len(xs), 2, 4))
    for d, x in enumerate(xs):
        wp[d, :, 0], wp[d, :, 1] = x, [-2.2, 2.2]
    coef, dur, status = ctx.solve_batch(wp, np.array([0.0, 1.1]))
    smd, shit = ctx.mesh_sweep(ctx.sample(coef, dur, DT, S), tris, RADIUS)
    md, tm, tri, lower, st = ctx.mesh_clearance(coef, dur, tris)
    for d, x in enumerate(xs):
        print(f"x = {x:+.1f}: sampled minimum {smd[d]:.3f} m, hit {bool(shit[d])};  certified: min_dist {md[d]:.3e} m "
              f"at t = {tm[d]:.4f} s against triangle {tri[d]}, lower bound {lower[d]:.3e} m")

    comp = DeviceCompute(ctx, torch)
    tc, td, tt = (torch.from_numpy(a).cuda() for a in (coef, dur, tris))
    res = certify_mesh_clearance(comp, tc, td, tt, RADIUS, DT, S, status=torch.from_numpy(status))
    print("certify_mesh_clearance: hit", res.hit.tolist(), "undecided", res.undecided.tolist(), "cleared by sampling",
          res.cleared_by_sampling.tolist(), "sampled hit", res.sampled_hit.tolist())
