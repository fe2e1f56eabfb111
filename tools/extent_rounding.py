#!/usr/bin/env python3
"""The rounding of the path extent's fp64 method against the exact reference, on the CPU.

Runs tests/extent_exact.fp64_extent (the NumPy restatement of csrc/msnap_extent.hip) against exact_extent on the
families of tests/extent_cases.py at both orders: "near" (solved swarms within a few metres of the origin), "far" (the
same moved by +5000 m and +1e5 m), "long" (49 segments) and "hand" (the hand-built polynomials).  Per (drone, direction)
the largest of ext - S, S - upper and |ext - the exact value at t_ext|, in units of 2^-52 R_k (R_k = extent_R,
include/msnap.h).  C_ROUND_EXTENT is ten times the worst over the families, rounded up.  Also the nodes per lane (mean,
maximum) and whether any lane met a cap.  About a minute of CPU.

    python tools/extent_rounding.py
"""
from __future__ import annotations

import math
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import extent_cases as EC  # noqa: E402
import extent_exact as EE  # noqa: E402


def case(name, order):
    if name in EC.SWARMS:
        return EC.swarm_case(name, order)
    if name.startswith("parabola"):
        coef, dur = EC.parabola(order, float(name.split("_")[1]))
        return coef, dur, EC.AXES[:2]
    if name == "constant":
        return EC.constant_path(order)
    return EC.hand_case(name, order)[:3]


def names():
    return list(EC.SWARMS) + ["parabola_1", "parabola_3", "constant"] + list(EC.HAND)


def measure(job):
    name, order = job
    coef, dur, dirs = case(name, order)
    st = {}
    ext, t_ext, upper = EE.fp64_extent(coef, dur, dirs, stats=st)
    cands = EE.candidate_segments(coef, dur, dirs)
    worst, gap = 0.0, -np.inf
    for d in range(ext.shape[0]):
        for k in range(ext.shape[1]):
            R = EE.extent_R(coef[d], dur[d], dirs[k])
            if R == 0.0:
                continue
            S, _ = EE.exact_extent(coef[d], dur[d], dirs[k], cands[d][k])
            at = EE.exact_value_at(coef[d], dur[d], dirs[k], t_ext[d, k])
            worst = max(worst, EE.round_ratio(ext[d, k], upper[d, k], S, R, at))
            if not st["capped"][d, :, k].any():      # what the closed-walk bound is missed by without the r term
                e = ext[d, k]
                gap = max(gap, (upper[d, k] - (e + EE.REL_CLOSE * abs(e) + EE.ABS_CLOSE)) / (EE.EPS * R))
    family = EC.SWARMS[name][0] if name in EC.SWARMS else "hand"
    return family, name, order, worst, gap, float(st["nodes"].mean()), int(st["nodes"].max()), bool(st["capped"].any())


def main():
    worst, nodes = {}, {}
    jobs = [(n, o) for n in names() for o in (7, 9)]
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for family, name, order, ratio, gap, mean, most, capped in ex.map(measure, jobs):
            print(f"[{family}] {name} order {order}: rounding / (2^-52 R) {ratio:.3f}  closed-walk bound missed by / "
                  f"(2^-52 R) {gap:.3f}  nodes/lane mean {mean:.1f} max {most}  capped {capped}", flush=True)
            worst[family] = max(worst.get(family, -np.inf), ratio, gap)
            m = nodes.setdefault(family, [0.0, 0, 0])
            m[0], m[1], m[2] = m[0] + mean, m[1] + 1, max(m[2], most)
    for family, w in worst.items():
        print(f"{family}, worst: {w:.3f}  nodes/lane mean {nodes[family][0] / nodes[family][1]:.1f} max {nodes[family][2]}")
    c = max(worst.values())
    print(f"worst ratio over the families: {c:.3f}; ten times that, rounded up: {max(1, math.ceil(10 * c))}; "
          f"C_ROUND_EXTENT in tests/extent_exact.py and include/msnap.h: {EE.C_ROUND_EXTENT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
