#!/usr/bin/env python3
"""Replanning in flight with allocated segment times.

The eight drones of example 08 leave their paths at 40 % of the flight for three new waypoints.  The caller's times for
them are a guess -- evenly spaced -- and a drone that arrives with some speed pays for a bad guess in snap, and then in
the peaks it has to fly.  swarm.replan(..., optimize={...}) lets msnap_optimize_times_states move the two interior
times of each drone before the solve: the state at the hand-over, the waypoints, the end state and the arrival time
stay as they are.  Printed per drone, for the even and for the allocated times: the snap cost and the certified speed
and acceleration peaks (msnap_dynamic_peaks) of the new path.

    python examples/10_replan_time_allocation.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, replan  # noqa: E402

N, M = 8, 6
wp, t = synthetic.swarm(8, N, M)
rng = np.random.default_rng(8)
with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    t_r = 0.4 * dur.sum(dim=1)
    steps = torch.from_numpy(rng.uniform(-2.0, 2.0, (N, 3, 4))).to(dev)
    t_new = torch.tensor([1.5, 3.0, 4.5], dtype=torch.float64, device=dev)
    pos_r, _ = comp.eval_state(coef, dur, t_r)
    wp_new = pos_r[:, None, :] + torch.cumsum(steps, dim=1)
    rows = {}
    for name, optimize in (("even", None), ("allocated", {"min_fraction": 0.1, "max_iter": 200, "tol": 1e-4})):
        c, d, st, _ = replan(comp, coef, dur, t_r, wp_new, t_new, optimize=optimize)
        peak, _, pst = comp.dynamic_peaks(c, d)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0 and int(pst.abs().sum()) == 0
        c, d = c.cpu().numpy().copy(), d.cpu().numpy().copy()
        rows[name] = (ctx.snap_cost(c, d).sum(axis=1), peak.cpu().numpy().copy(), np.cumsum(d, axis=1))
    for k in range(N):
        for name in ("even", "allocated"):
            J, peak, knots = rows[name]
            print(f"drone {k} {name:9s}: knots {np.round(knots[k], 3).tolist()} s, snap cost {J[k]:.4g}, "
                  f"speed peak {peak[k, 0]:.3f} m/s, acceleration peak {peak[k, 1]:.3f} m/s^2")
        print(f"         cost ratio allocated / even: {rows['allocated'][0][k] / rows['even'][0][k]:.3f}")
