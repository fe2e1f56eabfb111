#!/usr/bin/env python3
"""Dynamic limits timed with device events: dynamic_peaks_device and retime_to_limits_device (fit, common) on solved
synthetic swarms, 256 x 10 (order 7), 4096 x 20 (order 7) and 65 536 x 10 (order 9).  Device-resident buffers, 10
warm-up + 30 timed launches each; one JSON line per config (times in microseconds) with the sources' csrc hash.

    python tools/limits_bench.py [--quick]        (--quick: 5 timed launches, for a profiler run)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_path_planning_python_amd import Context, _lib  # noqa: E402
from drone_path_planning_python_amd.synthetic import swarm  # noqa: E402

CONFIGS = ((7, 256, 10), (7, 4096, 20), (9, 65536, 10))
REPS = 5 if "--quick" in sys.argv else 30
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


for order, N, M in CONFIGS:
    wp, t = swarm(40 + order, min(N, 4096), M)
    wp, t = np.tile(wp, (N // wp.shape[0], 1, 1)), np.tile(t, (N // t.shape[0], 1))
    with Context(0, order, 64) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        coef = torch.empty((N, M, 4, order + 1), dtype=torch.float64, device=dev)
        dur = torch.empty((N, M), dtype=torch.float64, device=dev)
        st = torch.empty((N,), dtype=torch.int32, device=dev)
        ctx.solve_batch_device(N, M, torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev), False, coef, dur, st)
        peak = torch.empty((N, 4), dtype=torch.float64, device=dev)
        t_peak = torch.empty((N, 4), dtype=torch.float64, device=dev)
        pst = torch.empty((N,), dtype=torch.int32, device=dev)
        c2, d2, sc = torch.empty_like(coef), torch.empty_like(dur), torch.empty((N,), dtype=torch.float64, device=dev)
        us_peaks = timed(lambda: ctx.dynamic_peaks_device(N, M, coef, dur, peak, t_peak, pst))
        lim = [3.0, 4.0, 0.0, 1.0]
        us_retime = timed(lambda: ctx.retime_to_limits_device(N, M, coef, dur, lim, 3, c2, d2, sc))
        torch.cuda.synchronize()
        assert int(pst.abs().sum()) == 0 and int(st.abs().sum()) == 0
        print(json.dumps({"order": order, "drones": N, "segments": M, "dynamic_peaks_device_us": round(us_peaks, 2),
                          "retime_to_limits_device_us": round(us_retime, 2), "reps": REPS,
                          "coef_MB": round(coef.numel() * 8 / 1e6, 2), "csrc": _lib.csrc_sha()}), flush=True)
