"""Writes tests/golden/timeopt_wide_golden.npz: the second fixture of Context.optimize_times, for what the first
(make_timeopt_golden.py, left as it is) does not reach -- the 8-drone tile (order 7 above 40 segments, order 9 above
29), segments 64..79 at their floor, inputs that start below the floor, a shared grid, weights that are neither 0 nor 1
-- grouped so that one call per group fills more than one tile and leaves a partial one.

    python tests/golden/make_timeopt_wide_golden.py     (needs scipy; the tests do not; some minutes on 8 cores)

Per drone, as the first fixture: J0, J_slsqp, J_descent (restatement, tol 1e-8, 2000 steps), J_ref = the smaller;
gap4, iters4, solves4 of the restatement at the GPU test's settings (tol 1e-4, 500 steps) with its cost J4 and whether
it stopped on the measure (conv4); active, the highest active segment (top_active, -1: none), the number of input
durations below the floor (n_below).

The prefix of the iteration (step-rule parity): the restatement at max_iter = 1 and 3 with its trace -- knots, exact
cost, accepted steps, trials, and the smallest Armijo margin of the run (a drone whose margin is below 1e-3 is left out
of the prefix test: rounding could flip that decision).  `prefix_sens` is the largest |change of a knot| / t[M] when the
gradient of every trial is scaled per segment by random factors in 1 +- 2e-6, the allowance between the kernel's and
the oracle's cost: what rounding of that size does to the knots, from the reference alone.

Waypoints are rounded to float32 before anything is computed (the file holds them as float32, exactly); everything is
packed into flat arrays (tests/timeopt_ref.py::unpack_cases reads them) to stay under the size cap."""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

import make_timeopt_golden as base  # noqa: E402
import msnap_oracle as oracle  # noqa: E402
import timeopt_ref as R  # noqa: E402

W1 = (1.0, 1.0, 1.0, 1.0)
W_MIXED = (2.0, 0.5, 1.0, 3.0)
TD8 = {7: (41, 49, 72, 80), 9: (30, 58)}       # sizes that run as 8-drone tiles, per order
TD16_LAST = {7: 40, 9: 29}
NOISE = 2e-6
MARGIN_MIN = 1e-3


def squeezed(t, every, rng):
    """Every `every`-th duration times 0.2..0.3, the grid rescaled to the same total."""
    T = np.diff(t)
    T[every - 1::every] *= rng.uniform(0.2, 0.3, size=T[every - 1::every].shape)
    T *= t[-1] / T.sum()
    out = np.concatenate([[0.0], np.cumsum(T)])
    out[-1] = t[-1]
    return out


def groups():
    """[(order, min_fraction, weights, shared, [(wp, t), ..])]: one call of the GPU test per entry."""
    rng = np.random.default_rng(20261017)
    rw = lambda m: base.random_walk(rng, m)                       # noqa: E731
    uw = base.uneven_walk

    def sq(case, every):
        return case[0], squeezed(case[1], every, rng)

    def shared(m, n):
        t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, size=m))])
        t *= 10.0 / t[-1]
        return [(rw(m)[0], t) for _ in range(n)]

    return [
        (7, 0.1, W1, False, [rw(41) for _ in range(11)]),
        (7, 0.5, W1, False, [uw(3, 49), sq(uw(4, 49), 5), sq(rw(49), 7)]),
        (7, 0.5, W1, False, [uw(8, 72), sq(uw(8, 72), 7), sq(uw(9, 72), 5)]),
        (7, 0.5, W1, False, [uw(10, 80), sq(uw(11, 80), 7)]),
        (7, 0.1, W1, False, [rw(40) for _ in range(2)]),
        (9, 0.5, W1, False, [rw(30) for _ in range(6)] + [uw(s, 30) for s in (20, 21, 22)]
         + [sq(uw(23, 30), 5), sq(rw(30), 7)]),
        (9, 0.5, W1, False, [uw(30, 58), sq(uw(31, 58), 7), sq(rw(58), 5)]),
        (9, 0.1, W1, False, [rw(29) for _ in range(2)]),
        (7, 0.1, W1, True, shared(10, 6)),
        (7, 0.1, W1, True, shared(49, 6)),
        (7, 0.1, W_MIXED, False, [rw(41) for _ in range(3)]),
    ]


def exact_cost(wp, t, ncoef, w):
    coef, dur = oracle.solve_batch_fast(wp[None], t[None], ncoef)
    return R.weighted(oracle.snap_cost(coef[0], dur[0]), w)


def prefix(wp, t, w, mf, max_iter, ncoef, noise_seed=None):
    """The restatement's first `max_iter` accepted steps; with a seed, on gradients scaled by 1 +- NOISE per segment."""
    trace, orig = [], R.snap_cost_grad
    if noise_seed is not None:
        rng = np.random.default_rng(noise_seed)
        R.snap_cost_grad = lambda c: (lambda g: g * (1.0 + NOISE * rng.uniform(-1, 1, size=(g.shape[0], 1))))(orig(c))
    try:
        r = R.optimize(wp, t, w, mf, max_iter, 1e-4, ncoef, R.fast_cost, trace=trace)
    finally:
        R.snap_cost_grad = orig
    return r, trace


def one_drone(job):
    k, order, mf, w, wp, t = job
    ncoef = order + 1
    Tmin = R.floor_of(t, mf)
    J0 = exact_cost(wp, R.start_times(t, Tmin), ncoef, w)
    base.W = w                                                    # (slsqp reads the module's weights)
    ta = base.slsqp(wp, t, ncoef, mf)
    Ja = exact_cost(wp, ta, ncoef, w) if np.diff(ta).min() >= Tmin * (1 - 1e-12) else np.inf
    rb = R.optimize(wp, t, w, mf, 2000, 1e-8, ncoef, R.fast_cost)
    Jb = exact_cost(wp, rb["t_out"], ncoef, w)
    r4 = R.optimize(wp, t, w, mf, 500, 1e-4, ncoef, R.fast_cost)
    J4 = exact_cost(wp, r4["t_out"], ncoef, w)
    Jref = min(Ja, Jb)
    best = ta if Ja <= Jb else rb["t_out"]
    act = np.flatnonzero(np.diff(best) - Tmin <= 1e-6 * Tmin)
    out = dict(J0=J0, J_ref=Jref, J_slsqp=Ja, J_descent=Jb, J4=J4, gap4=(J4 - Jref) / Jref, conv4=r4["pg"] <= 1e-4,
               active=len(act), top_active=int(act.max()) if len(act) else -1, iters4=r4["iters"],
               solves4=r4["solves"], n_below=int((np.diff(t) < Tmin).sum()), p_t=[], p_cost=[], p_iters=[],
               p_trials=[], p_margin=[], prefix_sens=[])
    for mi in (1, 3):
        r, trace = prefix(wp, t, w, mf, mi, ncoef)
        rn, tn = prefix(wp, t, w, mf, mi, ncoef, noise_seed=1000 * k + mi)
        margin = min((m for _, _, m in trace), default=np.inf)
        same = [a for _, a, _ in trace] == [a for _, a, _ in tn]
        assert same or margin < MARGIN_MIN, (k, mi, margin)        # noise of 2e-6 flips no decision 1e-3 away
        out["p_t"].append(r["t_out"])
        out["p_cost"].append(exact_cost(wp, r["t_out"], ncoef, w))
        out["p_iters"].append(r["iters"])
        out["p_trials"].append(len(trace))
        out["p_margin"].append(margin)
        out["prefix_sens"].append(float(np.abs(rn["t_out"] - r["t_out"]).max() / t[-1]) if same else np.inf)
    print(k, "order", order, "M", len(t) - 1, "mf", mf, "J/J0 %.4g" % (Jref / J0), "a-b %.2e" % ((Ja - Jb) / Jref),
          "gap4 %.2e" % out["gap4"], "conv4", bool(out["conv4"]), "active", out["active"], "top", out["top_active"],
          "below", out["n_below"], "iters", r4["iters"], "solves", r4["solves"], "margins %.3g %.3g" %
          tuple(out["p_margin"]), "sens %.2e %.2e" % tuple(out["prefix_sens"]), flush=True)
    return out


def check(z):
    """The conditions the fixture was built for (tests/test_timeopt_cpu.py asserts them on the committed file)."""
    n = int(z["n"])
    seg = np.diff(z["off"]) - 1
    order = z["order"][z["group"]]
    assert (z["top_active"] >= 64).sum() >= 2, z["top_active"]
    assert (z["n_below"] >= 3).sum() >= 4, z["n_below"]
    for o in (7, 9):
        have = set(seg[order == o].tolist())
        assert set(TD8[o]) <= have and TD16_LAST[o] in have, (o, have)
        assert max(np.bincount(z["group"][(order == o) & np.isin(seg, TD8[o])])) >= 11
    assert (z["gap4"] >= -1e-12).all()
    assert np.array_equal(z["J_ref"], np.minimum(z["J_slsqp"], z["J_descent"]))
    agree = np.abs(z["J_slsqp"] - z["J_descent"]) <= 1e-6 * z["J_ref"]
    assert agree.sum() >= 0.8 * n, (int(agree.sum()), n)
    left_out = z["p_margin"] < MARGIN_MIN
    assert left_out.any(axis=1).sum() <= 0.1 * n, left_out.sum(axis=0)
    assert np.isfinite(z["prefix_sens"][~left_out]).all() and (z["prefix_sens"][~left_out] > 0).all()
    assert z["shared"].sum() == 2 and (np.asarray(z["weights"]) != 1.0).any(axis=1).sum() == 1
    return agree


def main():
    jobs, grp = [], []
    gs = groups()
    for gi, (order, mf, w, shared, drones) in enumerate(gs):
        for wp, t in drones:
            wp = wp.astype(np.float32).astype(np.float64)
            jobs.append((len(jobs), order, mf, w, wp, t))
            grp.append(gi)
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(one_drone, jobs, chunksize=1)
    col = lambda key, dt=np.float64: np.array([r[key] for r in res], dtype=dt)   # noqa: E731
    data = dict(
        n=np.int64(len(jobs)), group=np.array(grp, dtype=np.int64), order=np.array([g[0] for g in gs], dtype=np.int64),
        min_fraction=np.array([g[1] for g in gs]), weights=np.array([g[2] for g in gs]),
        shared=np.array([g[3] for g in gs], dtype=bool),
        off=np.concatenate([[0], np.cumsum([len(j[5]) for j in jobs])]).astype(np.int64),
        wp=np.concatenate([j[4] for j in jobs]).astype(np.float32), t=np.concatenate([j[5] for j in jobs]),
        p_t1=np.concatenate([r["p_t"][0] for r in res]), p_t3=np.concatenate([r["p_t"][1] for r in res]))
    for key in ("J0", "J_ref", "J_slsqp", "J_descent", "J4", "gap4", "p_cost", "p_margin", "prefix_sens"):
        data[key] = col(key)
    for key in ("active", "top_active", "iters4", "solves4", "n_below", "p_iters", "p_trials"):
        data[key] = col(key, np.int64)
    data["conv4"] = col("conv4", bool)
    agree = check(data)
    for k in np.flatnonzero(~agree):
        print("drone", k, "SLSQP and the descent disagree: J_slsqp %.12g J_descent %.12g, J_ref is the %s" %
              (data["J_slsqp"][k], data["J_descent"][k], "descent's" if data["J_descent"][k] <= data["J_slsqp"][k]
               else "SLSQP's"))
    for k in np.flatnonzero(~data["conv4"]):
        print("drone", k, "the restatement stopped on max_iter at tol 1e-4: gap4 %.3e" % data["gap4"][k])
    path = os.path.join(HERE, "timeopt_wide_golden.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes;", len(jobs), "drones; agree on", int(agree.sum()),
          "; max gap4 %.3e" % data["gap4"].max(), "; min margin %.3g" % data["p_margin"].min(),
          "; prefix_sens max %.3e" % data["prefix_sens"][np.isfinite(data["prefix_sens"])].max())


if __name__ == "__main__":
    main()
