#!/usr/bin/env python3
"""Holding patterns: park a flying swarm on closed loops until a new goal exists.

Eight drones fly rest-to-rest paths of six segments.  At 40 % of the flight a check fails and there is nowhere to go yet,
so every drone is sent to a holding loop of its own: eight closed curves through eight waypoints each, all on ONE shared
time grid, solved by msnap_solve_periodic -- the last waypoint is joined to the first with derivatives 1..6 continuous,
and yaw gains one full turn per lap (the lap offset).  swarm.join_loop leaves each path at t_r (msnap_eval_state) and
arrives on the loop at its first waypoint in the loop's own state (msnap_solve_states with that state as `end`), so
position, velocity, acceleration and jerk are continuous at both hand-overs.  Because all loops share the period,
certify_clearance over one period certifies every lap.

    python examples/11_holding_loop.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, certify_clearance, join_loop  # noqa: E402

N, M, L = 8, 6, 8
PERIOD = 12.0
wp, t = synthetic.swarm(11, N, M)
# the loops: circles of radius 1.5 m around eight centres 4 m apart on a 4 x 2 grid, 2 m above the paths' start,
# eight waypoints per lap; the last waypoint is the first again, with yaw one turn further
ang = 2.0 * np.pi * np.arange(L + 1) / L
centre = np.stack([4.0 * (np.arange(N) % 4), 4.0 * (np.arange(N) // 4), np.full(N, 2.0)], axis=1)
loop_wp = np.empty((N, L + 1, 4))
loop_wp[:, :, 0] = centre[:, None, 0] + 1.5 * np.cos(ang)[None, :]
loop_wp[:, :, 1] = centre[:, None, 1] + 1.5 * np.sin(ang)[None, :]
loop_wp[:, :, 2] = centre[:, None, 2]
loop_wp[:, :, 3] = ang[None, :] + 0.5 * np.pi              # nose along the circle: 2 pi further after a lap
loop_wp[:, L, :3] = loop_wp[:, 0, :3]                      # (closed bit for bit)
loop_t = PERIOD * np.arange(L + 1) / L                     # one time grid for all loops

with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    loop_coef, loop_dur, loop_status = comp.solve_periodic(torch.from_numpy(loop_wp).to(dev),
                                                           torch.from_numpy(loop_t).to(dev))
    t_r = 0.4 * dur.sum(dim=1)
    # one waypoint on the way: halfway between where the drone is and where its loop starts
    pos_r, _ = comp.eval_state(coef, dur, t_r)
    via = (0.5 * (pos_r.clone() + torch.from_numpy(loop_wp[:, 0]).to(dev)))[:, None, :]
    t_via = torch.tensor([3.0, 6.0], dtype=torch.float64, device=dev)
    join_coef, join_dur, join_status, (pos, deriv) = join_loop(comp, coef, dur, t_r, loop_coef, loop_dur, via, t_via)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and int(loop_status.abs().sum()) == 0 and int(join_status.abs().sum()) == 0

    c, d = ctx, lambda x: x.cpu().numpy()      # noqa: E731
    _, old_d = c.eval_state(d(coef), d(dur), d(t_r))
    j0_p, j0_d = c.eval_state(d(join_coef), d(join_dur), np.zeros(N))
    j1_p, j1_d = c.eval_state(d(join_coef), d(join_dur), np.full(N, 6.0))
    l0_p, l0_d = c.eval_state(d(loop_coef), d(loop_dur), np.zeros(N))
    l1_p, l1_d = c.eval_state(d(loop_coef), d(loop_dur), np.full(N, PERIOD))
    for k in range(N):
        print(f"drone {k}: leaves at t = {float(t_r[k]):.3f} s (state gap {np.abs(j0_d[k] - old_d[k]).max():.1e}), joins its "
              f"loop 6 s later (position gap {np.abs(j1_p[k] - l0_p[k]).max():.1e} m, derivative gap "
              f"{np.abs(j1_d[k] - l0_d[k]).max():.1e}); across the loop's seam: derivatives {np.abs(l1_d[k] - l0_d[k]).max():.1e}, "
              f"x, y, z {np.abs(l1_p[k, :3] - l0_p[k, :3]).max():.1e} m, yaw + {l1_p[k, 3] - l0_p[k, 3]:.6f} rad")
    # one period of the loops certifies every lap: all loops share the period
    n_samples = synthetic.formation_sample_count(loop_t)
    res = certify_clearance(comp, loop_coef, loop_dur, synthetic.DRONE_RADIUS, synthetic.SAMPLE_DT, n_samples,
                            status=loop_status)
    torch.cuda.synchronize()
    print(f"holding loops, one period of {PERIOD} s: {int(res.cleared_by_sampling.sum())} of {N} cleared by sampling, "
          f"{res.pairs.shape[0]} pairs certified exactly, certified hits {int(res.hit.sum())}, undecided "
          f"{int(res.undecided.sum())}; smallest certified lower bound {float(res.certified_lower.min()):.4f} m")
    assert int(res.hit.sum()) == 0 and int(res.undecided.sum()) == 0
