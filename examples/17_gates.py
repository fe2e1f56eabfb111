#!/usr/bin/env python3
"""Gates: prescribed derivatives at interior waypoints (msnap_solve_gates).

Eight drones fly five segments.  Waypoint 2 is a gate: every drone crosses it at 3 m/s along the gate's axis (+x),
whatever the minimisation would have picked.  Waypoint 4 is a stop-and-go point: velocity, acceleration and jerk are
all zero there, the drone comes to rest and goes on.  The other waypoints are positions only.  The state at the gate
and at the stop is read back with msnap_eval_state, and the certified speed peak of the whole path
(msnap_dynamic_peaks) is at least the gate speed.

    python examples/17_gates.py        (needs an MI355X)
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
    coef, dur, status = comp.solve_gates(to(wp), to(t), fix=to(fix), via=to(via))
    knots = torch.cumsum(dur, dim=1)
    _, at_gate = comp.eval_state(coef, dur, knots[:, GATE - 1].contiguous())
    _, at_stop = comp.eval_state(coef, dur, knots[:, STOP - 1].contiguous())
    peak, t_peak, _ = comp.dynamic_peaks(coef, dur)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    for d in range(N):
        v = at_gate[d, :3, 0].cpu().numpy()
        s = at_stop[d, :3].abs().max(dim=0).values.cpu().numpy()
        print(f"drone {d}: crosses the gate at t = {float(knots[d, GATE - 1]):.3f} s with v = ({v[0]:.12f}, {v[1]:+.1e}, "
              f"{v[2]:+.1e}) m/s; at the stop |v|, |a|, |j| <= {s[0]:.1e}, {s[1]:.1e}, {s[2]:.1e}; "
              f"certified speed peak {float(peak[d, 0]):.4f} m/s at t = {float(t_peak[d, 0]):.3f} s")
