#!/usr/bin/env python3
"""Replanning in flight: leave a path at time t_r and fly through new waypoints, without landing.

A swarm of eight drones flies rest-to-rest paths of six segments.  At 40 % of the flight the goal changes: every drone
gets three new waypoints.  swarm.replan reads each drone's full state at t_r (msnap_eval_state), makes its position the
first waypoint and its derivatives the start state, and solves the new path (msnap_solve_states).  The new path
continues the old one: position, velocity, acceleration and jerk agree at the hand-over, and the certified peaks of the
new path include the speed the drone already had.

    python examples/08_replan_in_flight.py        (needs an MI355X)
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
    old = ctx.eval_flat(coef.cpu().numpy(), dur.cpu().numpy(), t_r.cpu().numpy())     # [N, N, 13]: drone d at t_r[d]
    old = old[np.arange(N), np.arange(N)]
    # three new waypoints per drone, 1.5 s apart, starting near where the drone is
    steps = torch.from_numpy(rng.uniform(-2.0, 2.0, (N, 3, 4))).to(dev)
    t_new = torch.tensor([1.5, 3.0, 4.5], dtype=torch.float64, device=dev)
    pos_r, _ = comp.eval_state(coef, dur, t_r)
    wp_new = pos_r[:, None, :] + torch.cumsum(steps, dim=1)
    new_coef, new_dur, new_status, (pos, deriv) = replan(comp, coef, dur, t_r, wp_new, t_new)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and int(new_status.abs().sum()) == 0
    new = ctx.eval_flat(new_coef.cpu().numpy(), new_dur.cpu().numpy(), np.zeros(1))[:, 0]
    peak, t_peak, _ = comp.dynamic_peaks(new_coef, new_dur)
    for d in range(N):
        v_old, v_new = np.linalg.norm(old[d, 3:6]), np.linalg.norm(new[d, 3:6])
        print(f"drone {d}: leaves its path at t = {float(t_r[d]):.3f} s with |v| = {v_old:.4f} m/s; the new path starts "
              f"with |v| = {v_new:.4f}, position gap {np.abs(old[d, :3] - new[d, :3]).max():.1e} m, "
              f"certified speed peak {float(peak[d, 0]):.4f} m/s")
