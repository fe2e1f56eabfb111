#!/usr/bin/env python3
"""The rounding of the dynamic-limit peaks' fp64 method against the exact reference, on the CPU.

Two groups of inputs.  "near": the solved shapes of tests/test_limits_gpu.py (C oracle), on which the allowance without
its coordinate term holds.  The families of tests/limits_cases.py -- hand-built polynomials, ties across segments,
peaks on the closed ends, jumps at a knot, equioscillating speeds, extreme scales, a mixed batch, deep paths -- which set the
coefficient c of the coordinate term r_q = c 2^-52 R_q (R_q = tests/limits_exact.peaks_R, include/msnap.h).

Per case, from tests/limits_exact.walk_peaks, the NumPy restatement of the kernel:
  - the worst |peak - exact |p^(r)(T u)|| / (2^-52 R_q) at the local time T u the lane evaluated, the exact value from
    mpmath: the rounding of the Horner alone, which C_ROUND_PEAKS is ten times of (rounded up);
  - the worst |peak - exact |p^(r)(t_peak)|| / (2^-52 R_q) at t_peak, on the segment msnap_eval_flat's <= lookup selects
    (the segment that starts at the knot where the lane that won is that one's start), and how much of it is left
    beyond the header's term for the rounding of t_peak itself, 2^-52 t_peak R'_q -- that must stay below C_ROUND_PEAKS;
  - the worst (peak - S) / S either way against exact_peaks and whether the inequality holds without and with r_q;
  - the nodes per lane and any capped lane.
The "deep" family (300 and 1500 equioscillating segments, the peak on the steep last point) has no exact_peaks: the
root finder would take hours, and it is there for the value at t_peak.

    python tools/limits_rounding.py [--near-only]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import c_oracle  # noqa: E402
import limits_cases as LC  # noqa: E402
import limits_exact as LE  # noqa: E402
from drone_path_planning_python_amd import synthetic  # noqa: E402


def solve(wp, t, nc):
    coef, dur, info, _ = c_oracle.solve_batch(wp, t, ncoef=nc)
    assert not info.any()
    return coef, dur


def near_cases():
    for m, n in ((1, 8), (2, 8), (10, 10), (49, 6)):
        yield f"order 7, {n} x {m}", solve(*synthetic.swarm(700 + m, n, m), 8)
    for m, n in ((4, 6), (10, 6), (20, 4)):
        yield f"order 9, {n} x {m}", solve(*synthetic.swarm(900 + m, n, m), 10)


def family_cases():
    """(family, name, (coef, dur), the drones that go through exact_peaks or None for all)"""
    for nc in (8, 10):
        o = nc - 1
        for name, (coef, dur, _) in LC.hand_built(nc).items():
            yield "hand-built", f"order {o}, {name}", (coef, dur), None
        for bump in (False, True):
            yield "ties", f"order {o}, first and third segment alike" + (", third x (1 + 2^-40)" if bump else ""), \
                LC.tie_segments(nc, bump), None
        yield "ends", f"order {o}, rising to the end", LC.rising(nc), None
        yield "ends", f"order {o}, falling from the start", LC.rising(nc, mirror=True), None
        for later in (False, True):
            yield "ends", f"order {o}, jump at a knot, larger value " + ("after" if later else "before"), \
                LC.knot_jump(nc, later), None
        yield "equioscillating", f"order {o}, T*_{o - 1}", LC.equioscillating(nc), None
        yield "solved", f"order {o}, 8 x 4", LC.solved_swarm(solve, nc), None
        for st, sw in LC.SCALES:
            yield "scales", f"order {o}, times x {st:g}, waypoints x {sw:g}", LC.scaled(solve, nc, st, sw), None
        coef, dur = LC.busy_batch(nc)
        good = np.isfinite(coef).all(axis=(1, 2, 3)) & (dur > 0).all(axis=1)
        yield "mixed batch", f"order {o}, 67 x 3 (its 65 valid drones)", (coef[good], dur[good]), 16
        for m in (300, 1500):
            yield "deep", f"order {o}, {m} equioscillating segments", LC.deep_path(nc, m), 0


def measure(name, coef, dur, candidates, exact_drones=None):
    """exact_drones: how many of the drones go through exact_peaks (the root finder; default all) -- the ratio at
    t_peak, the nodes and the caps are taken over every drone."""
    res = LE.walk_peaks(coef, dur)
    peak, t_peak, nodes, capped = res[:4]
    ratio = float(LC.horner_ratios(coef, dur, res).max())
    err, Rq, tau = LC.attained_errors(coef, dur, peak, t_peak, LC.later_pairs(res, dur))
    with np.errstate(invalid="ignore", divide="ignore"):
        at_t = float(np.nan_to_num(err / (LE.EPS * Rq)).max())
        beyond = float(np.nan_to_num(np.maximum(err - tau, 0.0) / (LE.EPS * Rq)).max())
    over = under = 0.0
    old = new = True
    for d in range(coef.shape[0] if exact_drones is None else exact_drones):
        S, _ = LE.exact_peaks(coef[d], dur[d], LE.candidate_segments(coef[d], dur[d]) if candidates else None)
        R = LE.peaks_R(coef[d], dur[d])
        for q in range(4):
            s = float(S[q])
            if s > 0:
                over = max(over, (peak[d, q] - s) / s)
                under = max(under, (s - peak[d, q]) / s)
            old = old and LE.in_contract(peak[d, q], S[q])
            new = new and LE.in_contract(peak[d, q], S[q], R[q])
    live = nodes[nodes > 0]
    print(f"{name}: drones {coef.shape[0]}  |peak - exact at T u| / (2^-52 R) <= {ratio:.3f}  "
          f"at t_peak <= {at_t:.3f}, beyond the time term <= {beyond:.3f}  "
          f"(peak - S) / S <= {over:.2e}  (S - peak) / S <= {under:.2e}  in contract without the term: {old}, with: {new}  "
          f"nodes/lane mean {live.mean() if live.size else 0:.1f} max {nodes.max()}  capped lanes {int(capped.sum())}",
          flush=True)
    return {"ratio": ratio, "at_t_peak": at_t, "beyond_time_term": beyond, "over": over, "under": under, "capped": int(capped.sum()), "nodes": int(nodes.max()),
            "old": old, "new": new}


def fold(worst, got):
    out = {k: max(v, worst.get(k, -np.inf)) for k, v in got.items() if k not in ("old", "new")}
    out["old"] = bool(got["old"] and worst.get("old", True))
    out["new"] = bool(got["new"] and worst.get("new", True))
    return out


def show(w):
    return {k: (v if isinstance(v, (bool, int, np.integer)) else float(f"{v:.3e}")) for k, v in w.items()}


def main():
    worst = {}
    for name, (coef, dur) in near_cases():
        worst = fold(worst, measure(name, coef, dur, candidates=True))
    print("near, worst:", show(worst))
    if "--near-only" in sys.argv:
        return 0
    fam = {}
    for family, name, (coef, dur), exact_drones in family_cases():
        fam[family] = fold(fam.get(family, {}), measure(f"[{family}] {name}", coef, dur,
                                                         family in ("solved", "scales"), exact_drones))
    for family, w in fam.items():
        print(f"{family}, worst:", show(w))
    c = max(w["ratio"] for w in fam.values())
    beyond = max(w["beyond_time_term"] for w in fam.values())
    want = int(np.ceil(10.0 * c))
    capped = [f for f, w in fam.items() if w["capped"]]
    print(f"worst Horner ratio over the families: {c:.3f}; ten times that, rounded up: {want}; C_ROUND_PEAKS in "
          f"tests/limits_exact.py and include/msnap.h: {LE.C_ROUND_PEAKS} ({'as derived' if want == LE.C_ROUND_PEAKS else 'NOT as derived'})")
    print(f"worst of the value at t_peak beyond the time term: {beyond:.3f} x 2^-52 R "
          f"({'within' if beyond <= LE.C_ROUND_PEAKS else 'NOT within'} r_q)")
    print("capped lanes: " + (", ".join(capped) if capped else "none in any family"))
    return 0 if want == LE.C_ROUND_PEAKS and beyond <= LE.C_ROUND_PEAKS else 1


if __name__ == "__main__":
    sys.exit(main())
