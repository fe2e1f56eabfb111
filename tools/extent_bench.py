#!/usr/bin/env python3
"""Path extent timed with events on the stream (tools/clearance_bench.py's method: device-resident buffers, 3 warm-up
calls, the median of 7 single timed calls): msnap_path_extent_device with the six axis directions -- the certified
bounding box of every path -- beside msnap_dynamic_peaks_device on the same coefficients, the two timed alternately:

  256 x 10 and 4096 x 20 at order 7, 65 536 x 10 at order 9 (per-drone times, synthetic.swarm).

One JSON line per shape, appended to profiles/extent_bench.jsonl, with the sources' csrc hash.

    python tools/extent_bench.py
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

OUT = os.path.join(ROOT, "profiles", "extent_bench.jsonl")
AXES = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
SHAPES = [(7, 256, 10), (7, 4096, 20), (9, 65536, 10)]


def time_shape(order, n, M):
    with Context(0, order, 32) as ctx:
        comp = DeviceCompute(ctx, torch)
        wp, t = synthetic.swarm(49, n, M)
        coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        assert int(st.abs().sum()) == 0
        dirs = torch.from_numpy(AXES).to(dev)
        ext, t_ext, upper = (torch.empty((n, 6), dtype=torch.float64, device=dev) for _ in range(3))
        est = torch.empty((n,), dtype=torch.int32, device=dev)
        peak, t_peak = (torch.empty((n, 4), dtype=torch.float64, device=dev) for _ in range(2))
        pst = torch.empty((n,), dtype=torch.int32, device=dev)
        tm = timed_alternately({
            "extent": lambda: ctx.path_extent_device(n, M, coef, dur, 6, dirs, ext, t_ext, upper, est),
            "peaks": lambda: ctx.dynamic_peaks_device(n, M, coef, dur, peak, t_peak, pst)})
        assert int(est.abs().sum()) == 0 and bool((ext <= upper).all())
        gap = float((upper - ext - 1e-9 * ext.abs()).max())
        return {"load": "extent_box", "order": order, "drones": n, "segments": M, "directions": 6, "lanes": n * M * 6,
                "path_extent_device_us": tm["extent"][0], "path_extent_us_min_max": tm["extent"][1:],
                "dynamic_peaks_device_us": tm["peaks"][0], "dynamic_peaks_us_min_max": tm["peaks"][1:],
                "largest_upper_minus_ext_less_relative_part": gap, "reps": 7}


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
