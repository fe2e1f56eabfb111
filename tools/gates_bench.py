#!/usr/bin/env python3
"""The solve with prescribed derivatives at interior waypoints timed with events on the stream
(tools/clearance_bench.py's method: device-resident buffers, 3 warm-up calls, the median of 7 single timed calls):
msnap_solve_gates_device beside msnap_solve_states_device on the same waypoints, times and end states, timed alternately,

  256 x 10 and 4096 x 10, orders 7 and 9 (per-drone times, synthetic.swarm with the first time 0),

once with an empty mask (fix of zeros: what the gates cost a caller who has none) and once with a velocity gate at every
second knot.  One JSON line per shape and mask, appended to profiles/gates_bench.jsonl (or the file named on the command
line), with the sources' csrc hash.  The figure is the ratio to msnap_solve_states_device; there is no target.

    python tools/gates_bench.py [out.jsonl]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clearance_bench import dev, timed_alternately  # noqa: E402
from drone_path_planning_python_amd import Context, _lib, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "gates_bench.jsonl")
SHAPES = [(7, 256, 10), (7, 4096, 10), (9, 256, 10), (9, 4096, 10)]


def time_shape(order, n, M, mask):
    K = (order + 1) // 2
    with Context(0, order, 32) as ctx:
        DeviceCompute(ctx, torch)             # (puts the context on torch's stream, where the events are recorded)
        wp, t = synthetic.swarm(51, n, M)
        assert (t[:, 0] == 0.0).all()
        rng = np.random.default_rng(52)
        scale = np.array([2.0, 2.0, 4.0, 8.0][:K - 1])
        start, end = (torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 4, K - 1)) * scale).to(dev) for _ in range(2))
        fix = np.zeros((n, M - 1), dtype=np.int32)
        if mask == "velocity_every_second_knot":
            fix[:, ::2] = 1
        via = rng.uniform(-1.0, 1.0, (n, M - 1, 4, K - 1)) * scale
        wp, t, fix, via = (torch.from_numpy(x).to(dev) for x in (wp, t, fix, via))
        coef = torch.empty((n, M, 4, order + 1), dtype=torch.float64, device=dev)
        dur = torch.empty((n, M), dtype=torch.float64, device=dev)
        st = torch.empty((n,), dtype=torch.int32, device=dev)
        tm = timed_alternately({
            "gates": lambda: ctx.solve_gates_device(n, M, wp, t, False, start, end, fix, via, coef, dur, st),
            "states": lambda: ctx.solve_states_device(n, M, wp, t, False, start, end, coef, dur, st)})
        ctx.solve_gates_device(n, M, wp, t, False, start, end, fix, via, coef, dur, st)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        return {"load": "solve_gates", "order": order, "drones": n, "segments": M, "mask": mask,
                "solve_gates_device_us": tm["gates"][0], "solve_gates_us_min_max": tm["gates"][1:],
                "solve_states_device_us": tm["states"][0], "solve_states_us_min_max": tm["states"][1:],
                "ratio_to_solve_states": round(tm["gates"][0] / tm["states"][0], 3), "reps": 7}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    rows = [time_shape(*s, mask) for s in SHAPES for mask in ("empty", "velocity_every_second_knot")]
    with open(out, "a") as f:
        for r in rows:
            r["csrc"] = _lib.csrc_sha()
            r["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
