#!/usr/bin/env python3
"""Time allocation on closed loops: patrol circuits whose waypoints are unevenly spaced.

Eight drones patrol racetrack-shaped circuits of ten waypoints each -- two straights and two bends, the waypoints
crowded into the bends -- on ONE shared period of 12 s, so that one period of certify_clearance certifies every lap.  The
period is the caller's; the knot times inside it are a guess, and evenly spaced times are a bad one for legs of such
different lengths.  msnap_optimize_times_periodic moves the interior knots of each loop, the period and the waypoints
kept, and the snap cost and the peak speed / acceleration fall.  A flying swarm then joins the allocated loops
(swarm.join_loop), and one period of the loops is certified.

    python examples/12_loop_time_allocation.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, certify_clearance, join_loop  # noqa: E402

N, M, L = 8, 6, 10
PERIOD = 12.0
W = (1.0, 1.0, 1.0, 0.5)
wp, t = synthetic.swarm(12, N, M)
loop_wp, loop_t = synthetic.patrol_circuits(N, L, PERIOD)      # the evenly spaced grid, shared by all loops

with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    d = lambda x: x.cpu().numpy()      # noqa: E731
    dwp, dt = torch.from_numpy(loop_wp).to(dev), torch.from_numpy(loop_t).to(dev)
    # even times
    c0, d0, s0 = comp.solve_periodic(dwp, dt)
    peak0 = comp.dynamic_peaks(c0, d0)[0].clone()
    J0 = (ctx.snap_cost(d(c0), d(d0)) * np.array(W)).sum(axis=1)
    # allocated times
    t_out, loop_coef, loop_dur, loop_status, info = comp.optimize_times_periodic(dwp, dt, W, min_fraction=0.1,
                                                                                max_iter=500, tol=1e-4)
    peak1 = comp.dynamic_peaks(loop_coef, loop_dur)[0]
    torch.cuda.synchronize()
    assert int(s0.abs().sum()) == 0 and int(loop_status.abs().sum()) == 0
    J1 = d(info["cost"])[:, 1]
    for k in range(N):
        print(f"loop {k}: cost x {J1[k] / J0[k]:.3f} after {int(info['iters'][k])} steps; peak speed "
              f"{float(peak0[k, 0]):.2f} -> {float(peak1[k, 0]):.2f} m/s, peak acceleration {float(peak0[k, 1]):.2f} -> "
              f"{float(peak1[k, 1]):.2f} m/s^2; durations {np.round(d(loop_dur)[k], 2).tolist()}")
    assert (J1 < J0).all() and np.array_equal(d(t_out)[:, -1], np.full(N, PERIOD))

    # a flying swarm joins the allocated loops at 40 % of its flight, through one waypoint on the way
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    t_r = 0.4 * dur.sum(dim=1)
    pos_r, _ = comp.eval_state(coef, dur, t_r)
    via = (0.5 * (pos_r.clone() + dwp[:, 0]))[:, None, :]
    t_via = torch.tensor([3.0, 6.0], dtype=torch.float64, device=dev)
    join_coef, join_dur, join_status, _ = join_loop(comp, coef, dur, t_r, loop_coef, loop_dur, via, t_via)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and int(join_status.abs().sum()) == 0
    j1_p, j1_d = ctx.eval_state(d(join_coef), d(join_dur), np.full(N, 6.0))
    l0_p, l0_d = ctx.eval_state(d(loop_coef), d(loop_dur), np.zeros(N))
    print(f"hand-over onto the loops: position gap {np.abs(j1_p - l0_p).max():.1e} m, derivative gap "
          f"{np.abs(j1_d - l0_d).max():.1e}")
    # one period of the loops certifies every lap: all loops share the period
    n_samples = synthetic.formation_sample_count(loop_t)
    res = certify_clearance(comp, loop_coef, loop_dur, synthetic.DRONE_RADIUS, synthetic.SAMPLE_DT, n_samples,
                            status=loop_status)
    torch.cuda.synchronize()
    print(f"allocated loops, one period of {PERIOD} s: {int(res.cleared_by_sampling.sum())} of {N} cleared by sampling, "
          f"{res.pairs.shape[0]} pairs certified exactly, certified hits {int(res.hit.sum())}, undecided "
          f"{int(res.undecided.sum())}; smallest certified lower bound {float(res.certified_lower.min()):.4f} m")
    assert int(res.hit.sum()) == 0 and int(res.undecided.sum()) == 0
