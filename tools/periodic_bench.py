#!/usr/bin/env python3
"""The periodic solve timed with events on the stream (tools/clearance_bench.py's method: device-resident buffers,
3 warm-up calls, the median of 7 single timed calls): msnap_solve_periodic_device beside msnap_solve_states_device
(both end states given) on the same waypoints and times, the two timed alternately:

  256 x 10 and 4096 x 10, orders 7 and 9 (per-drone times, synthetic.swarm with the first time 0).

One JSON line per shape, appended to profiles/periodic_bench.jsonl, with the sources' csrc hash and the kernel's
registers as the compiler's resource remarks give them (make EXTRA=-Rpass-analysis=kernel-resource-usage; REGISTERS
below is copied from there and belongs to the csrc hash it was recorded with).  The figure is the ratio to the
boundary-state solve; there is no target.  Then one line per order with the accuracy of the cases of
tests/periodic_exact.py against their 60-digit solutions, beside msnap_solve_states given the exact seam state.

    python tools/periodic_bench.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clearance_bench import dev, timed_alternately  # noqa: E402
from drone_path_planning_python_amd import Context, _lib, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "periodic_bench.jsonl")
SHAPES = [(7, 256, 10), (7, 4096, 10), (9, 256, 10), (9, 4096, 10)]
# periodic_solve_kernel<K>: architectural / accumulation VGPRs, SGPRs, scratch bytes per lane, waves per SIMD by registers
REGISTERS = {7: {"vgprs": 216, "agprs": 0, "sgprs": 58, "scratch": 0, "waves_per_simd": 2},
             9: {"vgprs": 256, "agprs": 66, "sgprs": 90, "scratch": 0, "waves_per_simd": 1}}


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
        tm = timed_alternately({
            "periodic": lambda: ctx.solve_periodic_device(n, M, wp, t, False, coef, dur, st),
            "states": lambda: ctx.solve_states_device(n, M, wp, t, False, start, end, coef, dur, st)})
        ctx.solve_periodic_device(n, M, wp, t, False, coef, dur, st)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        return {"load": "solve_periodic", "order": order, "drones": n, "segments": M,
                "solve_periodic_device_us": tm["periodic"][0], "solve_periodic_us_min_max": tm["periodic"][1:],
                "solve_states_device_us": tm["states"][0], "solve_states_us_min_max": tm["states"][1:],
                "ratio_to_solve_states": round(tm["periodic"][0] / tm["states"][0], 3), "reps": 7,
                "registers": REGISTERS[order]}


def accuracy(order):
    import periodic_exact as PE
    from conftest import norm_rel
    rows = {}
    with Context(0, order, 64) as ctx:
        for M, kind in PE.gpu_cases(order):
            wp, t = PE.case(order, M, kind=kind)
            ref, seam = PE.reference(order, M, kind)
            coef, _, st = ctx.solve_periodic(wp, t)
            yard, _, st2 = ctx.solve_states(wp, t, seam, seam)
            assert (st == 0).all() and (st2 == 0).all()
            rows[f"{M}_{kind}"] = {"solve_periodic": norm_rel(coef, ref), "solve_states_at_exact_seam": norm_rel(yard, ref)}
    return {"load": "solve_periodic_accuracy", "order": order, "drones": PE.N_CASE, "metric": "norm_rel vs 60 digits",
            "cases": rows}


def main():
    rows = [time_shape(*s) for s in SHAPES] + [accuracy(order) for order in (7, 9)]
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
