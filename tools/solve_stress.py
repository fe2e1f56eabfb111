#!/usr/bin/env python3
"""Randomised check of the solve kernels against the C oracle: batch sizes across the launcher's regimes (small-batch
two-sided kernel, two-sided column-split throughput kernel, one-sided persistent kernel, shared-grid GEMM), segment counts
1..24, both orders, shared / per-drone time grids, the start-time quirk, random launch-geometry options (persistent grids
of a few waves: every wave walks several tiles).  usage: solve_stress.py [seconds] [seed].  GPU box only."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import c_oracle  # noqa: E402
from conftest import norm_rel  # noqa: E402
from drone_path_planning_python_amd import Context  # noqa: E402

# order 9 on random grids with duration ratios up to 6 and 15-20 segments: kernels and oracle differ by up to a few 1e-9 of
# the largest coefficient, and the difference is the KERNELS'.  Against 60-digit solutions on this draw the oracle's dense
# LU is within 1e-12 (8e-12 at worst), the kernels within 8e-10 on nine drones per segment count and, over the millions of
# drones walked here, 5.5e-9: the reduced block system has a condition number of 1-2e9 on such grids, every kernel family
# loses the same digits in the same places (DESIGN.md sections 2 and 3, profiles/solve_accuracy.md,
# profiles/solve_loss_stages.md).  Order 7: oracle 1e-12, kernels 2.5e-12.  The tests hold 1e-9 on the suite's even grids
# and these bars on this draw (tests/test_solve_exact_gpu.py).
from solve_cases import STRESS_TOL as TOL  # noqa: E402  ({7: 1e-9, 9: 2e-8})


def run(budget=60.0, seed=1, max_cases=None):
    rng = np.random.default_rng(seed)
    t0, n_cases, worst = time.time(), 0, {7: 0.0, 9: 0.0}
    ctxs = {7: Context(order=7, max_segments=64), 9: Context(order=9, max_segments=64)}
    try:
        while time.time() - t0 < budget and (max_cases is None or n_cases < max_cases):
            order = int(rng.choice([7, 9]))
            ctx = ctxs[order]
            M = int(rng.integers(1, 25 if order == 7 else 21))
            r = rng.random()
            N = int(rng.integers(1, 300)) if r < 0.45 else int(rng.integers(300, 5000)) if r < 0.85 else \
                int(rng.choice([8191, 16385, 40000, 70001]))
            shared = bool(rng.integers(0, 2))
            wp = rng.uniform(-5, 5, size=(N, M + 1, 4))
            T = rng.uniform(0.4, 2.5, size=(1 if shared else N, M))
            t = np.concatenate([np.zeros((T.shape[0], 1)), np.cumsum(T, axis=1)], axis=1)
            if not shared and N > 2 and rng.random() < 0.5:
                t[int(rng.integers(0, N))] += 0.25 * float(T.min())          # the reference's start-row quirk
            opts = {"no_twist": int(rng.random() < 0.3), "no_twin": int(rng.random() < 0.3),
                    "solve_grid_waves": int(rng.choice([0, 0, 3, 7, 64])), "gemm_grid_waves": int(rng.choice([0, 0, 5]))}
            for k, v in opts.items():
                ctx.set_option(k, v)
            grid = shared and rng.random() < 0.5 and M <= 49
            tt = t[0] if shared else t
            if grid:
                ctx.prepare_grid(tt)
                coef, dur, status = ctx.solve_grid(wp)
            else:
                coef, dur, status = ctx.solve_batch(wp, tt)
            kern = ctx.last_kernel()
            ref, rdur, info, _ = c_oracle.solve_batch(wp, tt, ncoef=order + 1, faithful=False, n_threads=8)
            err = norm_rel(coef, ref)
            ok = (status == 0).all() and not info.any() and err <= TOL[order] and np.array_equal(dur, rdur)
            if not ok:
                print(f"MISMATCH order={order} N={N} M={M} shared={shared} grid={grid} opts={opts} kernel={kern} err={err:.3e} "
                      f"status!=0: {int((status != 0).sum())} dur equal: {np.array_equal(dur, rdur)}")
                sys.exit(1)
            worst[order] = max(worst[order], err)
            n_cases += 1
    finally:
        for c in ctxs.values():
            c.close()
    print(f"solve_stress: {n_cases} random cases within {TOL} of the oracle in {time.time() - t0:.0f} s; worst {worst}")
    return n_cases


if __name__ == "__main__":
    run(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
