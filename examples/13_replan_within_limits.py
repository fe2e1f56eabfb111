#!/usr/bin/env python3
"""Replanning in flight within dynamic limits.

The eight drones of example 08 leave their paths at 40 % of the flight for three new waypoints, and the caller's guess
for the new legs is deliberately short: 1.5 s in all.  A replanned path cannot be stretched afterwards -- its start
state is in physical units, so msnap_retime_to_limits does not apply -- and with msnap_optimize_times_states the guess
would be final.  swarm.replan_within_limits searches the time weight of msnap_optimize_times_free per drone instead:
each round is one allocation with a free total, one msnap_dynamic_peaks and one read, and a drone keeps the fastest
path found whose certified peaks are within the limits.  Printed per drone: the peaks of the plain replan at the guess,
the peaks and the total of the path kept, the weight, and whether it is feasible (a drone that leaves faster than
v_max, or under more acceleration than a_max, cannot be: the limit is broken at the hand-over).

    python examples/13_replan_within_limits.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, replan, replan_within_limits  # noqa: E402

N, M = 8, 6
LIMITS = [22.0, 60.0, 0.0, 0.0]      # speed [m/s], acceleration [m/s^2], jerk and yaw rate unconstrained
wp, t = synthetic.swarm(8, N, M)
rng = np.random.default_rng(8)
with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    t_r = 0.4 * dur.sum(dim=1)
    steps = torch.from_numpy(rng.uniform(-2.0, 2.0, (N, 3, 4))).to(dev)
    t_new = torch.tensor([0.5, 1.0, 1.5], dtype=torch.float64, device=dev)
    pos_r, _ = comp.eval_state(coef, dur, t_r)
    wp_new = (pos_r[:, None, :] + torch.cumsum(steps, dim=1)).clone()
    c, d, st, _ = replan(comp, coef, dur, t_r, wp_new, t_new)
    before = comp.dynamic_peaks(c, d)[0].cpu().numpy().copy()
    c, d, st, (pos, deriv), info = replan_within_limits(comp, coef, dur, t_r, wp_new, t_new, LIMITS, rounds=8)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    after, totals = info["peaks"].cpu().numpy(), d.sum(dim=1).cpu().numpy()
    v0 = torch.linalg.norm(deriv[:, :3, 0], dim=1).cpu().numpy()
    print(f"limits: {LIMITS[0]} m/s, {LIMITS[1]} m/s^2; guess {float(t_new[-1])} s")
    for k in range(N):
        print(f"drone {k}: leaves at {v0[k]:5.2f} m/s; at the guess {before[k, 0]:6.2f} m/s {before[k, 1]:7.2f} m/s^2; kept "
              f"{totals[k]:6.3f} s, {after[k, 0]:6.2f} m/s {after[k, 1]:7.2f} m/s^2, time weight {info['time_weight'][k]:.3g} "
              f"(violating: {info['violating_weight'][k]:.3g}), feasible: {bool(info['feasible'][k])}")
