#!/usr/bin/env python3
"""The rounding of the cross clearance's fp64 method against the exact reference, on the CPU.

The allowance of include/msnap.h is r = 1e-13 + C_ROUND_CROSS 2^-52 R + C_CLOCK 2^-52 T_c R'.  Per pair the deviation is
the largest of lower - D, D - min_dist and |min_dist - the exact distance at t_min|, less the distance-relative 1e-13
(tests/cross_clearance_exact.deviation), from the NumPy restatement on the C oracle's coefficients.

  C_ROUND_CROSS  the deviation in units of 2^-52 R over the families with zero offsets: there fl(t - 0) is exact and
                 nothing of the deviation is the clock's;
  C_CLOCK        the deviation in units of 2^-52 T_c R' over the families with offsets -- ALL of it, the coordinate
                 part included, so the figure is an over-estimate.

Ten times the worst ratio, rounded up, is the constant (the rule of C_ROUND, C_ROUND_MESH and C_ROUND_EXTENT).

    python tools/cross_clearance_rounding.py
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import c_oracle  # noqa: E402
import cross_clearance_cases as XC  # noqa: E402
import cross_clearance_exact as XE  # noqa: E402


def solve(wp, t, nc):
    coef, dur, info, _ = c_oracle.solve_batch(wp, t, ncoef=nc)
    assert not info.any()
    return coef, dur


def families():
    """(constant the family measures, name, (A, B, pairs))"""
    for nc, ma, mb in ((8, 3, 10), (8, 1, 1), (10, 2, 5)):
        o = nc - 1
        yield "clock", f"order {o}, {ma} against {mb} segments, t0_a in [0, 4]", XC.unequal(solve, nc, ma, mb)
        for off in (1000.0, 5000.0, 1e5):
            yield "round", f"order {o}, {ma} against {mb} segments at +{off:g} m, zero offsets", XC.far_origin(solve, nc, ma, mb, off)
        for t0 in (100.0, 1e4, 1e6):
            yield "clock", f"order {o}, {ma} against {mb} segments, clocks at {t0:g} s", XC.far_clock(solve, nc, ma, mb, t0)
        yield "clock", f"order {o}, {ma} against {mb} segments, clocks at 1e4 s, +5000 m", XC.far_clock(solve, nc, ma, mb, 1e4, 5000.0)
    for nc in (8, 10):
        for off in (5000.0, 1e5):
            yield "round", f"order {nc - 1}, one set against itself (K9's far swarm) at +{off:g} m", XC.same_set_far(solve, nc, off)
        yield "clock", f"order {nc - 1}, times and waypoints x 1000, t0_a = 1000 T0_A + 0.3", XC.long_clock(solve, nc)
    yield "clock", "order 7, crossing pair, both t0 = 3.7", XC.crossing(solve, 8, 3.7, 3.7)
    yield "clock", "order 7, crossing pair, t0 = 3.7 and 3.9", XC.crossing(solve, 8, 3.7, 3.9)
    A, B, pairs = XC.windows(solve, 8)
    yield "clock", "order 7, windows (touching, starting and ending inside a segment)", (A, B, pairs[1:])
    coef, dur = solve(*XC.swarm(8, 8, 6), 8)
    t_r = 0.4 * np.add.accumulate(dur, axis=1)[[1, 4, 6], -1]
    nc_, nd_ = XC.continued(coef, dur, [1, 4, 6], t_r)
    yield "clock", "order 7, three continued paths against the paths they left", \
        ((nc_, nd_, t_r), (coef[[1, 4, 6]], dur[[1, 4, 6]], None), np.array([[k, k] for k in range(3)]))


def measure(name, A, B, pairs):
    (ca, da, t0a), (cb, db, t0b) = A, B
    ta, tb = XE._t0(t0a, len(da)), XE._t0(t0b, len(db))
    st = {}
    md, tm, lower = XE.fp64_cross_clearance(ca, da, ta, cb, db, tb, pairs, stats=st)
    exact = XE.exact_of((ca, da, ta), (cb, db, tb), pairs)
    dev_w, rr, rc, gap = -np.inf, -np.inf, -np.inf, -np.inf
    capped_pair = np.zeros(len(pairs), dtype=bool)
    capped_pair[st["lane_pair"][st["capped"]]] = True
    for k, (a, b) in enumerate(pairs):
        if exact[k] is None:            # the drones never fly at the same time
            assert md[k] == np.inf and lower[k] == np.inf and np.isnan(tm[k])
            continue
        D = exact[k][0]
        args = (ca[a], da[a], ta[a], cb[b], db[b], tb[b])
        R, Rp, Tc = XE.pair_R(*args), XE.pair_Rprime(*args), XE.T_c(da[a], ta[a], db[b], tb[b])
        dev = XE.deviation(md[k], lower[k], D, XE.exact_cross_distance_at(*args, tm[k]))
        if not capped_pair[k]:          # the closed-walk inequality carries the same r
            dev = max(dev, md[k] * (1 - XE.REL_CLOSE) - XE.ABS_CLOSE - lower[k])
        dev_w, rr, rc = max(dev_w, dev), max(rr, dev / (XE.EPS * R)), max(rc, dev / (XE.EPS * Tc * Rp))
        gap = max(gap, md[k] * (1 - XE.REL_CLOSE) - lower[k])
    nodes = st["nodes"]
    print(f"{name}: pairs {len(pairs)}  deviation <= {dev_w:.3e} m  / (2^-52 R) <= {rr:.3f}  / (2^-52 T_c R') <= {rc:.4f}  "
          f"min_dist (1 - 1e-9) - lower <= {gap:.3e}  nodes/lane mean {nodes.mean():.1f} max {nodes.max()}  "
          f"capped lanes {int(st['capped'].sum())}", flush=True)
    return rr, rc


def main():
    worst = {"round": -np.inf, "clock": -np.inf}
    for which, name, (A, B, pairs) in families():
        rr, rc = measure(f"[{which}] {name}", A, B, pairs)
        worst[which] = max(worst[which], rr if which == "round" else rc)
    for which, const, have in (("round", "C_ROUND_CROSS", XE.C_ROUND_CROSS), ("clock", "C_CLOCK", XE.C_CLOCK)):
        print(f"{const}: worst ratio {worst[which]:.4f}; ten times, rounded up: {max(1, math.ceil(10 * worst[which]))}; "
              f"in tests/cross_clearance_exact.py and include/msnap.h: {have}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
