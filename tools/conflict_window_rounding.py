#!/usr/bin/env python3
"""The rounding of the conflict windows' fp64 method against the exact reference, on the CPU.

The entries state their guarantees up to the allowance r of the matching clearance entry (include/msnap.h):
distance >= threshold - r on the proven ranges, distance at t_first / t_last < threshold + r.  Per pair the deviation is
the largest of threshold - (the exact infimum over [S, t_clear_until] and over [t_clear_from, W]) and (the exact distance
at t_first, at t_last) - threshold, less the distance-relative 1e-13 threshold, from the NumPy restatement
(tests/conflict_exact.py) on the C oracle's coefficients.  As tools/cross_clearance_rounding.py:

  C_ROUND_CROSS  the deviation in units of 2^-52 R over the families with zero offsets;
  C_CLOCK        the deviation in units of 2^-52 T_c R' over the families with offsets -- all of it.

Ten times the worst ratio must stay below the constants the header states for the clearance entries.

    python tools/conflict_window_rounding.py
"""
from __future__ import annotations

import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import conflict_exact as KE  # noqa: E402
import conflict_window_cases as KC  # noqa: E402
import cross_clearance_cases as XC  # noqa: E402
import cross_clearance_exact as XE  # noqa: E402

THRESHOLD = 2.5
# far below any useful resolution: every crossing is followed down to the depth cap, leaves of 2^-40 of an interval, so
# that what is left between the brackets and the threshold is rounding and not the resolution (at t_res = 1e-6 s the
# brackets sit 1e-8 .. 1e-6 m either side of the threshold and every deviation is negative)
T_RES = 1e-14


def families():
    """(constant the family measures, name, (A, B, pairs))"""
    for nc, ma, mb in ((8, 3, 10), (10, 2, 5)):
        o = nc - 1
        yield "clock", f"order {o}, {ma} against {mb} segments, t0_a in [0, 4]", XC.unequal(KC.solve, nc, ma, mb)
        for off in (1000.0, 5000.0, 1e5):
            yield "round", f"order {o}, {ma} against {mb} segments at +{off:g} m, zero offsets", \
                XC.far_origin(KC.solve, nc, ma, mb, off)
        for t0 in (1e4, 1e6):
            yield "clock", f"order {o}, {ma} against {mb} segments, clocks at {t0:g} s", XC.far_clock(KC.solve, nc, ma, mb, t0)
        yield "clock", f"order {o}, {ma} against {mb} segments, clocks at 1e4 s, +5000 m", \
            XC.far_clock(KC.solve, nc, ma, mb, 1e4, 5000.0)
    for nc in (8, 10):
        yield "round", f"order {nc - 1}, one set against itself (K9's far swarm) at +1e5 m", XC.same_set_far(KC.solve, nc, 1e5)


def measure(name, A, B, pairs, threshold=THRESHOLD, t_res=T_RES):
    (ca, da, t0a), (cb, db, t0b) = A, B
    pairs = np.asarray(pairs)[::2]
    ta, tb = XE._t0(t0a, len(da)), XE._t0(t0b, len(db))
    st = {}
    cu, tf, df, tl, dl, cf = KE.fp64_conflict_window(ca, da, ta, cb, db, tb, pairs, threshold, t_res, stats=st)
    dev_w, rr, rc, found = -np.inf, -np.inf, -np.inf, 0
    for k, (a, b) in enumerate(pairs):
        args = (ca[a], da[a], ta[a], cb[b], db[b], tb[b])
        pcs, (S, W) = KE.pieces(*args)
        if not pcs:
            continue
        R, Rp, Tc = XE.pair_R(*args), XE.pair_Rprime(*args), XE.T_c(da[a], ta[a], db[b], tb[b])
        dev = -np.inf
        if not np.isfinite(cu[k]):
            dev = max(dev, threshold - float(KE.exact_infimum(pcs, S, W)))
        else:
            if not cu[k] == tf[k] == float(S):
                dev = max(dev, threshold - float(KE.exact_infimum(pcs, S, Fraction(float(cu[k])))))
            if not cf[k] == tl[k] == float(W):
                dev = max(dev, threshold - float(KE.exact_infimum(pcs, Fraction(float(cf[k])), W)))
        for t in (tf[k], tl[k]):
            if np.isfinite(t):
                found += 1
                dev = max(dev, float(XE.exact_cross_distance_at(*args, t)) - threshold)
        dev -= XE.REL_ROUND * threshold
        dev_w, rr, rc = max(dev_w, dev), max(rr, dev / (XE.EPS * R)), max(rc, dev / (XE.EPS * Tc * Rp))
    nodes = st["nodes"]
    print(f"{name}: pairs {len(pairs)}  conflict times {found}  deviation <= {dev_w:.3e} m  / (2^-52 R) <= {rr:.3f}  "
          f"/ (2^-52 T_c R') <= {rc:.4f}  nodes/lane and direction mean {nodes.mean():.1f} max {nodes.max()}", flush=True)
    return rr, rc


def main():
    worst = {"round": -np.inf, "clock": -np.inf}
    for which, name, (A, B, pairs) in families():
        rr, rc = measure(f"[{which}] {name}", A, B, pairs)
        worst[which] = max(worst[which], rr if which == "round" else rc)
    for which, const, have in (("round", "C_ROUND_CROSS", XE.C_ROUND_CROSS), ("clock", "C_CLOCK", XE.C_CLOCK)):
        print(f"{const}: worst ratio {worst[which]:.4f}; ten times: {10 * worst[which]:.3f}; the clearance entries' "
              f"constant in include/msnap.h: {have}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
