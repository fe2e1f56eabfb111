#!/usr/bin/env python3
"""The rounding of the mesh conflict windows' fp64 method against the exact reference.

msnap_mesh_conflict_window states its guarantees up to an allowance r = 1e-13 + C 2^-52 R (include/msnap.h): distance >=
threshold - r on the proven ranges, distance at t_first / t_last < threshold + r.  Per drone the deviation is the largest
of threshold - (the exact infimum over [0, t_clear_until] and over [t_clear_from, W]) and (the exact distance at t_first,
at t_last) - threshold, less the distance-relative 1e-13 threshold, in units of 2^-52 R (R: msnap_mesh_clearance's).
The exact reference is tests/mesh_conflict_exact.py's for straight flights, so the loads are the straight-flight
families of tests/mesh_clearance_cases.py: FEATURES (every closest feature), RANDOM's lines of up to three segments at
every scale, and FAR (the same moved by +5000, -8000 and +1e5 m).  Each drone gets a threshold of its own, its exact D
rounded to fp64 plus 1/16 m, so that every drone is in conflict, and t_res far below any useful resolution: every
crossing is followed down to the depth cap, and what is left between the brackets and the threshold is rounding.

    python tools/mesh_conflict_window_rounding.py            the NumPy restatement, on the CPU
    python tools/mesh_conflict_window_rounding.py --gpu      the kernel (needs the GPU)

Ten times the worst ratio, rounded up, is what the header's constant has to cover.
"""
from __future__ import annotations

import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import mesh_clearance_cases as MC  # noqa: E402
import mesh_clearance_exact as ME  # noqa: E402
import mesh_conflict_exact as MX  # noqa: E402

MARGIN = 2.0 ** -4
T_RES = 1e-14
RANDOM_LINES = ("o7_m1", "o7_m2", "o7_m3", "o9_m1", "o9_m2", "o9_m3", "o7_m2_small", "o9_m3_small", "o7_m3_large",
                "o9_m2_large", "o7_m3_quick", "o9_m2_quick", "o7_m2_slow", "o9_m3_slow")


def families():
    for name in sorted(MC.FEATURES):
        yield "FEATURES", name
    for name in RANDOM_LINES:
        yield "RANDOM", name
    for name in sorted(MC.FAR):
        yield "FAR", name


def measure(family, name, window):
    """window(coef, dur, tris, threshold, t_res) -> the entry's outputs.  Returns the worst ratio of the line."""
    line = MC.get_line(family, name)
    coef, dur, tris = MC.line_paths(line)
    scale = float(np.abs(line["points"] - line["points"].mean()).max())
    exactD = MC.line_exact(family, name)
    worst, dev_w, found = -np.inf, -np.inf, 0
    for d in range(len(dur)):
        thr = float(exactD[d][0]) + MARGIN * min(1.0, scale)              # (a small-scale line: a margin of its scale)
        ex = MX.StraightExact(line["points"][d], line["durs"][d], line["nc"], tris, thr)
        W = float(dur[d].sum())
        cu, tf, df, wf, tl, dl, wl, cf = (x[0] for x in window(coef[d:d + 1], dur[d:d + 1], tris, thr, T_RES)[:8])
        dev = -np.inf
        if not np.isfinite(cu):
            dev = max(dev, thr - float(ex.infimum(0, Fraction(W))))
        else:
            if not cu == tf == 0.0:
                dev = max(dev, thr - float(ex.infimum(0, Fraction(float(cu)))))
            if not cf == tl == W:
                dev = max(dev, thr - float(ex.infimum(Fraction(float(cf)), Fraction(W))))
        for t in (tf, tl):
            if np.isfinite(t):
                found += 1
                dev = max(dev, float(ex.distance_at(float(t))) - thr)
        dev -= ME.REL_ROUND * thr
        dev_w, worst = max(dev_w, dev), max(worst, dev / (ME.EPS * ME.mesh_R(coef[d], dur[d], tris)))
    print(f"[{family}] {name}: drones {len(dur)}  conflict times {found}  deviation <= {dev_w:.3e} m  "
          f"/ (2^-52 R) <= {worst:.3f}", flush=True)
    return worst


def main():
    if "--gpu" in sys.argv[1:]:
        from drone_path_planning_python_amd import Context
        ctxs = {8: Context(device_id=0, order=7, max_segments=64), 10: Context(device_id=0, order=9, max_segments=64)}
        window = lambda c, t, tris, thr, res: ctxs[c.shape[3]].mesh_conflict_window(c, t, tris, thr, res)      # noqa: E731
        what = "kernel"
    else:
        window = MX.fp64_mesh_conflict_window
        what = "restatement"
    worst = max(measure(family, name, window) for family, name in families())
    print(f"{what}: worst ratio {worst:.4f}; ten times: {10 * worst:.3f}; msnap_mesh_clearance's C_ROUND_MESH: "
          f"{ME.C_ROUND_MESH}; C_ROUND_MESH_WINDOW in include/msnap.h and tests/mesh_conflict_exact.py: "
          f"{MX.C_ROUND_MESH_WINDOW}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
