#!/usr/bin/env python3
"""The boundary-state solve timed with events on the stream (tools/clearance_bench.py's method: device-resident
buffers, 3 warm-up calls, the median of 7 single timed calls): msnap_solve_states_device with both end states given,
beside msnap_solve_batch_device on the same waypoints and times -- with its default launch, and with "no_twist" and
"no_twin" set (the one-sided kernels, whose mapping the boundary-state kernel shares) -- the three timed alternately:

  256 x 10 and 4096 x 10, orders 7 and 9 (per-drone times, synthetic.swarm with the first time 0).

One JSON line per shape, appended to profiles/states_bench.jsonl, with the sources' csrc hash.  The figures are the
ratios to the rest-to-rest solve; there is no target.

    python tools/states_bench.py
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

OUT = os.path.join(ROOT, "profiles", "states_bench.jsonl")
SHAPES = [(7, 256, 10), (7, 4096, 10), (9, 256, 10), (9, 4096, 10)]


def time_shape(order, n, M):
    K = (order + 1) // 2
    with Context(0, order, 32) as ctx:
        DeviceCompute(ctx, torch)             # (puts the context on torch's stream, where the events are recorded)
        wp, t = synthetic.swarm(51, n, M)
        assert (t[:, 0] == 0.0).all()
        rng = np.random.default_rng(52)
        scale = np.array([2.0, 2.0, 4.0, 8.0][:K - 1])
        start, end = (torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 4, K - 1)) * scale).to(dev) for _ in range(2))
        wp, t = torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev)
        coef = torch.empty((n, M, 4, order + 1), dtype=torch.float64, device=dev)
        dur = torch.empty((n, M), dtype=torch.float64, device=dev)
        st = torch.empty((n,), dtype=torch.int32, device=dev)
        names = {}

        def batch(one_sided):
            def run():
                ctx.set_option("no_twist", one_sided)
                ctx.set_option("no_twin", one_sided)
                ctx.solve_batch_device(n, M, wp, t, False, coef, dur, st)
                names[one_sided] = ctx.last_kernel()
            return run
        tm = timed_alternately({
            "states": lambda: ctx.solve_states_device(n, M, wp, t, False, start, end, coef, dur, st),
            "batch": batch(0), "one_sided": batch(1)})
        ctx.solve_states_device(n, M, wp, t, False, start, end, coef, dur, st)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        return {"load": "solve_states", "order": order, "drones": n, "segments": M,
                "solve_states_device_us": tm["states"][0], "solve_states_us_min_max": tm["states"][1:],
                "solve_batch_device_us": tm["batch"][0], "solve_batch_us_min_max": tm["batch"][1:],
                "solve_batch_kernel": names[0],
                "solve_batch_one_sided_us": tm["one_sided"][0], "solve_batch_one_sided_us_min_max": tm["one_sided"][1:],
                "solve_batch_one_sided_kernel": names[1],
                "ratio_to_solve_batch": round(tm["states"][0] / tm["batch"][0], 3),
                "ratio_to_one_sided": round(tm["states"][0] / tm["one_sided"][0], 3), "reps": 7}


def main():
    rows = [time_shape(*s) for s in SHAPES]
    with open(OUT, "a") as f:
        for r in rows:
            r["csrc"] = _lib.csrc_sha()
            r["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
