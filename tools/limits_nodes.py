#!/usr/bin/env python3
"""Nodes the peak search of csrc/msnap_limits.hip visits, restated on the CPU (the same Taylor shift, Bernstein bound,
prune rule and stackless walk; no GPU needed): mean per (drone, segment, quantity) item and the mean over waves of the
64-lane maximum -- the trip count of the wave-uniform loop, which sets the kernel time.

    python tools/limits_nodes.py [order] [drones] [segments]      (default: 7 256 10)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import limits_exact as LE  # noqa: E402  (fp64_walk_peaks: the restated walk)
import msnap_oracle as O  # noqa: E402  (the CPU solve, tools only)
from drone_path_planning_python_amd.synthetic import swarm  # noqa: E402


def main():
    order = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    M = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    nc = order + 1
    wp, t = swarm(40 + order, N, M)
    coef, dur = O.solve_batch_fast(wp, t, ncoef=nc)
    _, _, nodes, _ = LE.fp64_walk_peaks(coef, dur)
    c = nodes.reshape(-1)
    waves = c[: len(c) // 64 * 64].reshape(-1, 64).max(axis=1)
    print(f"order {order}, {N} x {M}: nodes per item mean {c.mean():.1f} (q: "
          + ", ".join(f"{c.reshape(-1, 4)[:, q].mean():.1f}" for q in range(4))
          + f"), max {c.max()}; per wave (64-lane max) mean {waves.mean():.1f}, max {waves.max()}")


if __name__ == "__main__":
    main()
