#!/usr/bin/env python3
"""Time allocation through gates (msnap_optimize_times_gates).

Example 17's path -- eight drones, five segments, a gate at waypoint 2 crossed at 3 m/s along +x, a full stop at
waypoint 4 -- first with the even times it was given, then with the interior times allocated by the library.  The
total duration, the waypoints and the gate values in m/s stay; what moves is when each waypoint is crossed.  Printed
per drone: the cost ratio, the certified speed peak before and after (msnap_dynamic_peaks), and the velocity read back
at the gate's own knot of the new path (msnap_eval_state): still the gate speed.

    python examples/18_gated_time_allocation.py        (needs an MI355X)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drone_path_planning_python_amd import Context, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute  # noqa: E402

N, M = 8, 5
GATE, STOP, GATE_SPEED = 2, 4, 3.0
wp, t = synthetic.swarm(17, N, M)
fix = np.zeros((N, M - 1), dtype=np.int32)
via = np.full((N, M - 1, 4, 3), np.nan)          # entries under a clear bit are never read
fix[:, GATE - 1] = 0b001                         # velocity
via[:, GATE - 1, :, 0] = [GATE_SPEED, 0.0, 0.0, 0.0]
fix[:, STOP - 1] = 0b111                         # velocity, acceleration and jerk
via[:, STOP - 1] = 0.0
with Context(device_id=0, order=7, max_segments=16) as ctx:
    comp = DeviceCompute(ctx, torch)
    dev = comp.device
    to = lambda x: torch.from_numpy(x).to(dev)      # noqa: E731
    gates = dict(fix=to(fix), via=to(via))
    coef0, dur0, st0 = comp.solve_gates(to(wp), to(t), **gates)
    peak0 = comp.dynamic_peaks(coef0, dur0)[0].clone()
    t_out, coef, dur, status, info = comp.optimize_times_gates(to(wp), to(t), **gates)
    knots = torch.cumsum(dur, dim=1)
    _, at_gate = comp.eval_state(coef, dur, knots[:, GATE - 1].contiguous())
    peak, _, _ = comp.dynamic_peaks(coef, dur)
    torch.cuda.synchronize()
    assert int(st0.abs().sum()) == 0 and int(status.abs().sum()) == 0
    for d in range(N):
        v = at_gate[d, :3, 0].cpu().numpy()
        c = info["cost"][d].cpu().numpy()
        print(f"drone {d}: cost x {c[1] / c[0]:.3f} in {int(info['iters'][d])} steps; gate crossed at t = "
              f"{float(t[d, GATE]):.3f} -> {float(knots[d, GATE - 1]):.3f} s with v = ({v[0]:.12f}, {v[1]:+.1e}, {v[2]:+.1e}) "
              f"m/s; certified speed peak {float(peak0[d, 0]):.3f} -> {float(peak[d, 0]):.3f} m/s; total "
              f"{float(t[d, M]):.3f} s kept: {bool(t_out[d, M] == float(t[d, M]))}")
