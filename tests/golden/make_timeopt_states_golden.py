"""Writes tests/golden/timeopt_states_golden.npz: inputs and reference optima for Context.optimize_times_states.

    python tests/golden/make_timeopt_states_golden.py     (needs scipy; the tests do not; a few minutes on 8 cores)

Drones: durations U(0.5, 2), random-walk waypoints (steps in [-2, 2]), state values |v|, |a| <= 2, |j| <= 4, |s| <= 8
(tests/states_exact.py::STATE_SCALE).  Every group is one call of the GPU test and cycles through the four state
combinations start / end / both / neither:
  * both orders x 1, 2, 3, 10 and 20 segments, four drones each;
  * per order the first segment count that runs as 8-drone tiles with the state images in LDS (40 at order 7, 29 at
    order 9: lds_words below is the library's timeopt_lds_words), 11 drones: a full tile and a tail of 3;
  * one group on a shared grid, one with min_fraction = 0.5 and legs of very different lengths (segments at the floor,
    inputs below it), one with weights (2, 0.5, 1, 3).

Per drone, as tests/golden/make_timeopt_wide_golden.py records them, every figure from the restatement
tests/timeopt_states_ref.py (the dense fp64 collocation solve): J0; J_slsqp (SLSQP on the closed-form gradient),
J_descent (the restatement at tol 1e-8, 2000 steps), J_ref the smaller; J4, gap4, conv4, iters4, solves4 at the GPU
test's settings (tol 1e-4, 500 steps); the prefix of the iteration at max_iter 1 and 3 -- knots, accepted steps, the
smallest Armijo margin, and prefix_sens, the largest |change of a knot| / t[M] under gradients scaled by 1 +- 2e-6 per
segment, and not less than M 2^-52: the knots are running sums of up to M rounded durations, so two fp64 evaluations
of one step differ by that much before any gradient error (with two segments the first step does not depend on the
gradient's size at all, and the measured response is 0).  A run whose margin is below 1e-3 is left out of the prefix
test; at most a quarter may be, and every (order, combination) keeps one.  One segment has nothing to optimise:
J_ref = J0, no SLSQP, no prefix run.  In the min_fraction = 0.5 group the durations are drawn again until one lies below
the floor, so that the start point is a raised one.

Waypoints are rounded to float32 before anything is computed; everything is packed into flat arrays
(tests/timeopt_states_ref.py::unpack_cases reads them)."""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

import make_timeopt_golden as base  # noqa: E402
import make_timeopt_wide_golden as wide  # noqa: E402
import timeopt_ref as R  # noqa: E402
import timeopt_states_ref as S  # noqa: E402
from states_exact import STATE_SCALE  # noqa: E402

W1 = (1.0, 1.0, 1.0, 1.0)
W_MIXED = (2.0, 0.5, 1.0, 3.0)
COMBOS = ("start", "end", "both", "neither")
SEGMENTS = (1, 2, 3, 10, 20)
MARGIN_MIN = wide.MARGIN_MIN
LDS_BYTES = 160 * 1024


def lds_words(order, M, TD):
    """timeopt_lds_words(khalf, M, TD, ends = true) of csrc/msnap_timeopt.hip"""
    k = (order + 1) // 2
    nu, knots = k - 1, M - 1
    tr = 0 if k == 4 else k * 68 * 2
    return tr + TD * ((M + 1) * 4 + (M + 1) + 2 * (M + 1) + 4 * M + nu * nu * knots + 4 * nu * knots) + 2 * TD * 4 * (nu | 1)


def first_td8(order):
    M = 1
    while lds_words(order, M, 16) * 8 <= LDS_BYTES:
        M += 1
    return M


def drone(rng, order, M, combo, uneven=False, t=None):
    nd = (order + 1) // 2 - 1
    while t is None:
        t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, size=M))])
        if uneven and not (np.diff(t) < R.floor_of(t, 0.5)).any():
            t = None
    steps = rng.uniform(-2.0, 2.0, size=(M + 1, 4))
    if uneven:
        steps *= rng.choice([0.1, 1.0, 3.0], size=(M + 1, 1))
    wp = np.cumsum(steps, axis=0)
    scale = np.array(STATE_SCALE[:nd])
    start = rng.uniform(-1.0, 1.0, (4, nd)) * scale if combo in ("start", "both") else None
    end = rng.uniform(-1.0, 1.0, (4, nd)) * scale if combo in ("end", "both") else None
    return wp, t, combo, start, end


def groups():
    """[(order, min_fraction, weights, shared, [(wp, t, combo, start, end), ..])]: one call of the GPU test per entry."""
    rng = np.random.default_rng(20261019)
    out = []
    for order in (7, 9):
        for M in SEGMENTS:
            out.append((order, 0.1, W1, False, [drone(rng, order, M, c) for c in COMBOS]))
    for order in (7, 9):
        M = first_td8(order)
        out.append((order, 0.1, W1, False, [drone(rng, order, M, COMBOS[i % 4]) for i in range(11)]))
    grid = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, size=10))])
    out.append((9, 0.1, W1, True, [drone(rng, 9, 10, c, t=grid) for c in COMBOS]))
    out.append((7, 0.5, W1, False, [drone(rng, 7, 10, c, uneven=True) for c in COMBOS]))
    out.append((7, 0.1, W_MIXED, False, [drone(rng, 7, 10, c) for c in COMBOS]))
    return out


def exact_cost(wp, t, ncoef, w, start, end):
    return S.cost(S.solve(wp, t, start, end, ncoef // 2), np.diff(t), w)


def one_drone(job):
    k, order, mf, w, wp, t, combo, start, end = job
    ncoef = order + 1
    M = len(t) - 1
    Tmin = R.floor_of(t, mf)
    with S.given_states(start, end):
        J0 = exact_cost(wp, R.start_times(t, Tmin), ncoef, w, start, end)
        if M > 1:
            base.W = w                                            # (slsqp reads the module's weights)
            ta = base.slsqp(wp, t, ncoef, mf)
            Ja = exact_cost(wp, ta, ncoef, w, start, end) if np.diff(ta).min() >= Tmin * (1 - 1e-12) else np.inf
        else:
            ta, Ja = t, J0
        rb = R.optimize(wp, t, w, mf, 2000, 1e-8, ncoef, None)
        Jb = exact_cost(wp, rb["t_out"], ncoef, w, start, end)
        r4 = R.optimize(wp, t, w, mf, 500, 1e-4, ncoef, None)
        J4 = exact_cost(wp, r4["t_out"], ncoef, w, start, end)
        Jref = min(Ja, Jb)
        best = ta if Ja <= Jb else rb["t_out"]
        act = np.flatnonzero(np.diff(best) - Tmin <= 1e-6 * Tmin)
        out = dict(J0=J0, J_ref=Jref, J_slsqp=Ja, J_descent=Jb, J4=J4, gap4=(J4 - Jref) / Jref, conv4=r4["pg"] <= 1e-4,
                   active=len(act), iters4=r4["iters"], solves4=r4["solves"], n_below=int((np.diff(t) < Tmin).sum()),
                   p_t=[], p_iters=[], p_trials=[], p_margin=[], prefix_sens=[])
        for mi in (1, 3):
            r, trace = wide.prefix(wp, t, w, mf, mi, ncoef)
            rn, tn = wide.prefix(wp, t, w, mf, mi, ncoef, noise_seed=1000 * k + mi)
            margin = min((m for _, _, m in trace), default=np.inf)
            same = [a for _, a, _ in trace] == [a for _, a, _ in tn]
            assert same or margin < MARGIN_MIN, (k, mi, margin)    # noise of 2e-6 flips no decision 1e-3 away
            out["p_t"].append(r["t_out"])
            out["p_iters"].append(r["iters"])
            out["p_trials"].append(len(trace))
            out["p_margin"].append(margin)
            sens = float(np.abs(rn["t_out"] - r["t_out"]).max() / t[-1]) if same else np.inf
            out["prefix_sens"].append(max(sens, M * 2.0 ** -52))
    print(k, "order", order, "M", M, combo, "mf", mf, "J/J0 %.4g" % (Jref / J0), "a-b %.2e" % ((Ja - Jb) / Jref),
          "gap4 %.2e" % out["gap4"], "conv4", bool(out["conv4"]), "active", out["active"], "below", out["n_below"],
          "iters", r4["iters"], "solves", r4["solves"], "margins %.3g %.3g" % tuple(out["p_margin"]),
          "sens %.2e %.2e" % tuple(out["prefix_sens"]), flush=True)
    return out


def check(z):
    """The conditions the fixture was built for (tests/test_timeopt_states_cpu.py asserts them on the committed file)."""
    seg = np.diff(z["off"]) - 1
    order = z["order"][z["group"]]
    for o in (7, 9):
        have = set(seg[order == o].tolist())
        assert set(SEGMENTS) | {first_td8(o)} <= have, (o, have)
        assert max(np.bincount(z["group"][(order == o) & (seg == first_td8(o))])) == 11
    assert (z["gap4"] >= -1e-12).all()
    assert np.array_equal(z["J_ref"], np.minimum(z["J_slsqp"], z["J_descent"]))
    assert (z["J_ref"][seg > 1] < z["J0"][seg > 1]).all()
    assert z["shared"].sum() == 1 and (np.asarray(z["weights"]) != 1.0).any(axis=1).sum() == 1
    floor = z["min_fraction"][z["group"]] == 0.5
    assert floor.sum() == 4 and (z["active"][floor] > 0).sum() >= 2 and (z["n_below"][floor] > 0).all()
    # the prefix runs: one segment has no run to speak of
    runs = seg > 1
    left_out = (z["p_margin"] < MARGIN_MIN) & runs[:, None]
    assert left_out.sum() <= 0.25 * 2 * runs.sum(), (int(left_out.sum()), int(runs.sum()))
    kept = ~left_out & runs[:, None]
    assert np.isfinite(z["prefix_sens"][kept]).all() and (z["prefix_sens"][kept] > 0).all()
    for o in (7, 9):
        for c in COMBOS:
            assert kept[(order == o) & (z["combo"] == c)].any(), (o, c)
    return int(left_out.sum()), int(2 * runs.sum())


def main():
    jobs, grp = [], []
    gs = groups()
    for gi, (order, mf, w, shared, drones) in enumerate(gs):
        for wp, t, combo, start, end in drones:
            wp = wp.astype(np.float32).astype(np.float64)
            jobs.append((len(jobs), order, mf, w, wp, t, combo, start, end))
            grp.append(gi)
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(one_drone, jobs, chunksize=1)

    def block(x):
        out = np.zeros((4, 4))
        if x is not None:
            out[:, :x.shape[1]] = x
        return out

    col = lambda key, dt=np.float64: np.array([r[key] for r in res], dtype=dt)   # noqa: E731
    data = dict(
        n=np.int64(len(jobs)), group=np.array(grp, dtype=np.int64), order=np.array([g[0] for g in gs], dtype=np.int64),
        min_fraction=np.array([g[1] for g in gs]), weights=np.array([g[2] for g in gs]),
        shared=np.array([g[3] for g in gs], dtype=bool), combo=np.array([j[6] for j in jobs]),
        off=np.concatenate([[0], np.cumsum([len(j[5]) for j in jobs])]).astype(np.int64),
        wp=np.concatenate([j[4] for j in jobs]).astype(np.float32), t=np.concatenate([j[5] for j in jobs]),
        start=np.array([block(j[7]) for j in jobs]), end=np.array([block(j[8]) for j in jobs]),
        p_t1=np.concatenate([r["p_t"][0] for r in res]), p_t3=np.concatenate([r["p_t"][1] for r in res]))
    for key in ("J0", "J_ref", "J_slsqp", "J_descent", "J4", "gap4", "p_margin", "prefix_sens"):
        data[key] = col(key)
    for key in ("active", "iters4", "solves4", "n_below", "p_iters", "p_trials"):
        data[key] = col(key, np.int64)
    data["conv4"] = col("conv4", bool)
    left, runs = check(data)
    for k in np.flatnonzero(~data["conv4"]):
        print("drone", k, "the restatement stopped on max_iter at tol 1e-4: gap4 %.3e" % data["gap4"][k])
    path = os.path.join(HERE, "timeopt_states_golden.npz")
    np.savez_compressed(path, **data)
    sens = data["prefix_sens"]
    print("wrote", path, os.path.getsize(path), "bytes;", len(jobs), "drones;", left, "of", runs,
          "prefix runs left out; max gap4 %.3e" % data["gap4"].max(), "; J_ref / J0 %.3f .. %.3f" %
          ((data["J_ref"] / data["J0"]).min(), (data["J_ref"] / data["J0"]).max()),
          "; prefix_sens max %.3e" % sens[np.isfinite(sens)].max())


if __name__ == "__main__":
    main()
