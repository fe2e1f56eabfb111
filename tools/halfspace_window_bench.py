#!/usr/bin/env python3
"""Half-space windows timed with events on the stream, against the path extent on the same inputs: device-resident
buffers, 3 warm-up calls, then the median of 7 single timed calls, the two entries timed alternately.

Swarms: 256 x 10 and 4096 x 20 at order 7, 65 536 x 10 at order 9.  The planes are the six signed axes, each at the
median over the swarm of msnap_path_extent's ext in that direction, so that about half of the drones leave each
half-space; every drone is queried against every plane (6 N queries) over its whole flight, t_res = 1e-6 s.
msnap_halfspace_window_device walks every segment twice (forward and backward), and a later segment cannot know that an
earlier one already holds the first exit, so no ratio is promised: the measured ratio is reported, with the mean and
maximum nodes per live lane and direction from the NumPy restatement (tests/halfspace_exact.py) on the first 64 drones.

Then the corridor: swarm.certify_corridor of 256 straight flights through the three-box corridor of the hole in the
wall of tests/golden/env-scene-hole.stl (tests/halfspace_cases.py) -- three rounds of the entry and the routine's own
tensor work, timed as a whole on the host clock around a synchronise -- beside msnap_mesh_clearance_device on the same
flights.

One JSON line per load, appended to profiles/halfspace_window_bench.jsonl, with the sources' csrc hash.

    python tools/halfspace_window_bench.py
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import halfspace_cases as HC  # noqa: E402
import halfspace_exact as HE  # noqa: E402
from drone_path_planning_python_amd import Context, _lib, stl, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import CORRIDOR_INSIDE, DeviceCompute, certify_corridor  # noqa: E402

dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "halfspace_window_bench.jsonl")
T_RES = 1e-6
RESTATED_DRONES = 64
AXES = [[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]]


def timed_alternately(fns, warm=3, reps=7):
    """{name: (median, min, max) us}: one timed call of each in turn, `reps` rounds"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: (round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)) for k, v in us.items()}


def emit(row):
    row.update({"t_res_s": T_RES, "reps": 7, "csrc": _lib.csrc_sha(), "device": torch.cuda.get_device_name(0)})
    with open(OUT, "a") as f:
        line = json.dumps(row)
        print(line, flush=True)
        f.write(line + "\n")


def axes_load(order, N, M):
    with Context(0, order, max(M, 16)) as ctx:
        comp = DeviceCompute(ctx, torch)
        wp, t = synthetic.swarm(53, N, M)
        coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        coef, dur = coef.clone(), dur.clone()
        dirs = torch.tensor(AXES, dtype=torch.float64, device=dev)
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)      # noqa: E731
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)        # noqa: E731
        oe = [f64(N, 6), f64(N, 6), f64(N, 6), i32(N)]
        ctx.path_extent_device(N, M, coef, dur, 6, dirs, *oe)
        torch.cuda.synchronize()
        planes = torch.cat([dirs, oe[0].median(dim=0).values[:, None]], dim=1).contiguous()
        q = torch.stack(torch.meshgrid(torch.arange(N), torch.arange(6), indexing="ij"), dim=-1).reshape(-1, 2)
        queries = q.to(torch.int32).to(dev).contiguous()
        Q = queries.shape[0]
        ow = [f64(Q) for _ in range(6)] + [i32(Q)]
        t = timed_alternately({
            "extent": lambda: ctx.path_extent_device(N, M, coef, dur, 6, dirs, *oe),
            "window": lambda: ctx.halfspace_window_device(N, M, coef, dur, 6, planes, Q, queries, None, None, T_RES, *ow)})
        assert int(ow[6].abs().sum()) == 0 and int(oe[3].abs().sum()) == 0
        iu, tf, vf, tl, vl, ifr = (x.cpu().numpy() for x in ow[:6])
        found = np.isfinite(tf)
        # a drone is found outside exactly when its attained reach is above the limit (up to rounding at the level)
        agree = found == (oe[0].reshape(-1) > planes[:, 3].repeat(N)).cpu().numpy()
        closed = (tf[found] - iu[found] <= T_RES * 1.001) & (ifr[found] - tl[found] <= T_RES * 1.001)
        undecided = ~found & np.isfinite(iu)
        stats = {}
        n_sub = min(N, RESTATED_DRONES)
        r = HE.fp64_halfspace_window(coef[:n_sub].cpu().numpy(), dur[:n_sub].cpu().numpy(), planes.cpu().numpy(),
                                     queries[:6 * n_sub].cpu().numpy(), T_RES, stats=stats)
        assert (np.isfinite(r[1]) == found[:6 * n_sub]).mean() > 0.99
        nodes = stats["nodes"]
        emit({"load": "six axes at the median ext", "order": order, "drones": N, "segments": M, "queries": Q, "lanes": Q * M,
              "path_extent_device_us": t["extent"][0], "path_extent_us_min_max": t["extent"][1:],
              "halfspace_window_device_us": t["window"][0], "halfspace_window_us_min_max": t["window"][1:],
              "ratio_to_path_extent": round(t["window"][0] / t["extent"][0], 3),
              "queries_outside": int(found.sum()), "queries_undecided": int(undecided.sum()),
              "queries_agreeing_with_ext": int(agree.sum()), "searches_closed": int(closed.sum()),
              "restated_drones": n_sub, "restated_live_lanes": int(stats["lanes"]),
              "nodes_per_live_lane_and_direction_mean": round(float(nodes.mean()), 2),
              "nodes_per_live_lane_and_direction_max": int(nodes.max())})


def corridor_load(N=256, M=10):
    """N straight flights from y = -2 to y = 2 through or into the wall, cut into M segments of equal duration"""
    tris_h = np.ascontiguousarray(stl.load_stl(os.path.join(ROOT, "tests", "golden", "env-scene-hole.stl")), dtype=np.float64)
    planes_h, off = HC.hole_corridor(tris_h)
    rng = np.random.default_rng(54)
    a = np.stack([rng.uniform(-2.0, 2.0, N), np.full(N, -2.0), rng.uniform(-1.2, 1.2, N)], axis=1)
    b = np.stack([rng.uniform(-2.0, 2.0, N), np.full(N, 2.0), rng.uniform(-1.2, 1.2, N)], axis=1)
    wp = np.zeros((N, M + 1, 4))
    wp[:, :, :3] = a[:, None, :] + (b - a)[:, None, :] * np.linspace(0.0, 1.0, M + 1)[None, :, None]
    t = np.tile(np.linspace(0.0, 4.0, M + 1), (N, 1))
    with Context(0, 7, 16) as ctx:
        comp = DeviceCompute(ctx, torch)
        coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        coef, dur = coef.clone(), dur.clone()
        tris, planes = torch.from_numpy(tris_h).to(dev), torch.from_numpy(planes_h).to(dev)
        T = tris.shape[0]
        om = [torch.empty((N,), dtype=k, device=dev) for k in (torch.float64, torch.float64, torch.int32, torch.float64,
                                                                torch.int32)]
        t = timed_alternately({"mesh": lambda: ctx.mesh_clearance_device(N, M, coef, dur, T, tris, *om)})
        host = []
        for _ in range(3 + 7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = certify_corridor(comp, coef, dur, planes, off, [0, 1, 2], radius=HC.HOLE_RADIUS, t_res=T_RES)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e6)
        host = host[3:]
        inside = (res.verdict == CORRIDOR_INSIDE).cpu().numpy()
        lower = om[3].cpu().numpy()
        emit({"load": "three-box corridor through the hole against the mesh", "order": 7, "drones": N, "segments": M,
              "triangles": T, "radius_m": HC.HOLE_RADIUS, "mesh_clearance_device_us": t["mesh"][0],
              "mesh_clearance_us_min_max": t["mesh"][1:],
              "certify_corridor_host_us": round(statistics.median(host), 1),
              "certify_corridor_host_us_min_max": (round(min(host), 1), round(max(host), 1)),
              "drones_inside_the_corridor": int(inside.sum()),
              "of_those_with_mesh_lower_at_least_radius": int((lower[inside] >= HC.HOLE_RADIUS - 1e-9).sum()),
              "drones_with_mesh_lower_at_least_radius": int((lower >= HC.HOLE_RADIUS).sum())})


def main():
    for order, N, M in ((7, 256, 10), (7, 4096, 20), (9, 65536, 10)):
        axes_load(order, N, M)
    corridor_load()
    return 0


if __name__ == "__main__":
    sys.exit(main())
