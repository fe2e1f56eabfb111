"""Writes tests/golden/timeopt_periodic_golden.npz: inputs and reference optima for Context.optimize_times_periodic.

    python tests/golden/make_timeopt_periodic_golden.py     (needs scipy; the tests do not; a few minutes on 8 cores)

Every group is one call of the GPU test.  `kind` names what a group is there for:
  * walk      random loops, random-walk waypoints (steps in [-2, 2]: a nonzero lap offset on every axis), durations
              U(0.5, 2): both orders x 2, 3 and 10 segments, three drones each;
  * tile8     per order the first segment count that runs as 8-drone tiles (25 at order 7, 18 at order 9 -- which is
              also msnap_solve_periodic's cap there: lds_words below is the library's timeopt_lds_words), 11 drones: a
              full tile and a tail of 3; durations U(0.7, 1.4) (plain projected gradient is slow from rougher starts at
              these counts);
  * cap       msnap_solve_periodic's cap at order 7, 27 segments, two drones (order 9's is the tile8 group);
  * shared    one group on a shared grid;
  * floor     min_fraction = 0.5 and legs of very different lengths: inputs below the floor, segments at it;
  * weights   weights (2, 0.5, 1, 3);
  * curve     a closed curve (lap offset 0 in x, y, z) with one yaw turn per lap, unevenly spaced, times by chord
              length: 10 segments at order 7, 6 at order 9 (at 8 and 10 the restatement needs more than 500 steps
              there);
  * polygon   regular polygons of 3 and 6 corners, radius 3, one yaw turn per lap, period 12, durations U(0.6, 1.6)
              rescaled to it: the even grid is the optimum by symmetry (J_even is its cost).

Per drone, as tests/golden/make_timeopt_states_golden.py records them, every figure from the restatement
tests/timeopt_periodic_ref.py: J0; J_slsqp (SLSQP on the closed-form gradient), J_descent (the restatement at tol 1e-8,
2000 steps), J_ref the smaller; J4, gap4, conv4, iters4, solves4 at the GPU test's settings (tol 1e-4, 500 steps); the
prefix of the iteration at max_iter 1 and 3 -- knots, accepted steps, the smallest Armijo margin, and prefix_sens, the
largest |change of a knot| / t[M] under gradients scaled by 1 +- 2e-6 per segment, and not less than M 2^-52.

The inputs of a drone are drawn again (at most MAX_DRAWS times, seeded by drone and draw) until the restatement converges
at the GPU settings and both prefix runs keep an Armijo margin of 1e-3; check() then asserts what the fixture is for: at
most 10 % of the drones unconverged, at most 10 % of the prefix runs below the margin, the polygon drones converged and
within 1e-9 of J_even.

Waypoints are rounded to float32 before anything is computed; everything is packed into flat arrays
(tests/timeopt_periodic_ref.py::unpack_cases reads them)."""
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
import timeopt_periodic_ref as PR  # noqa: E402
import timeopt_ref as R  # noqa: E402

W1 = (1.0, 1.0, 1.0, 1.0)
W_MIXED = (2.0, 0.5, 1.0, 3.0)
MARGIN_MIN = wide.MARGIN_MIN
LDS_BYTES = 160 * 1024
SOLVE_CAP = {7: 27, 9: 18}          # msnap_solve_periodic_max_segments
MAX_DRAWS = 24
SEED = 20261020
PERIOD = 12.0


def lds_words(order, M, TD):
    """timeopt_lds_words(khalf, M, TD, kTimeoptRing) of csrc/msnap_timeopt.hip"""
    k = (order + 1) // 2
    nu, knots = k - 1, M - 1
    tr = 0 if k == 4 else k * 68 * 2
    return tr + TD * ((M + 1) * 4 + (M + 1) + 2 * (M + 1) + 4 * M + 2 * (nu * nu * knots + 4 * nu * knots))


def first_td8(order):
    M = 2
    while lds_words(order, M, 16) * 8 <= LDS_BYTES:
        M += 1
    return M


def draw(kind, order, M, rng, t=None):
    """(wp [M+1, 4], t [M+1]) of one drone of a group of this kind; `t` given: the shared grid"""
    if kind == "polygon":
        T = rng.uniform(0.6, 1.6, size=M)
        t = np.concatenate([[0.0], np.cumsum(T * (PERIOD / T.sum()))])
        t[-1] = PERIOD
        th = 2.0 * np.pi * np.arange(M + 1) / M
        wp = np.stack([3.0 * np.cos(th), 3.0 * np.sin(th), np.ones(M + 1), th], axis=1)
        wp[M, :3] = wp[0, :3]
        return wp, t
    if kind == "curve":
        th = np.concatenate([[0.0], np.cumsum(rng.uniform(0.8, 1.25, size=M))])
        th *= 2.0 * np.pi / th[-1]
        wp = np.stack([3.0 * np.cos(th), 2.5 * np.sin(th), 1.0 + 0.3 * np.sin(2.0 * th), th], axis=1)
        wp[M, :3] = wp[0, :3]
        T = np.linalg.norm(np.diff(wp[:, :3], axis=0), axis=1) * rng.uniform(0.9, 1.1, size=M)   # by chord length
        t = np.concatenate([[0.0], np.cumsum(T * (PERIOD / T.sum()))])
        t[-1] = PERIOD
        return wp, t
    lo, hi = (0.7, 1.4) if kind in ("tile8", "cap") else (0.5, 2.0)
    while t is None:
        t = np.concatenate([[0.0], np.cumsum(rng.uniform(lo, hi, size=M))])
        if kind == "floor" and not (np.diff(t) < R.floor_of(t, 0.5)).any():
            t = None
    steps = rng.uniform(-2.0, 2.0, size=(M + 1, 4))
    if kind == "floor":
        steps *= rng.choice([0.1, 1.0, 3.0], size=(M + 1, 1))
    return np.cumsum(steps, axis=0), t


def groups():
    """[(kind, order, M, min_fraction, weights, shared, n_drones)]: one call of the GPU test per entry."""
    out = []
    for order in (7, 9):
        for M in (2, 3, 10):
            out.append(("walk", order, M, 0.1, W1, False, 3))
    for order in (7, 9):
        out.append(("tile8", order, first_td8(order), 0.1, W1, False, 11))
    out.append(("cap", 7, SOLVE_CAP[7], 0.1, W1, False, 2))
    out.append(("shared", 9, 10, 0.1, W1, True, 3))
    out.append(("floor", 7, 10, 0.5, W1, False, 3))
    out.append(("weights", 7, 10, 0.1, W_MIXED, False, 3))
    for order, M in ((7, 10), (9, 6)):
        out.append(("curve", order, M, 0.1, W1, False, 2))
    for order in (7, 9):
        for M in (3, 6):
            out.append(("polygon", order, M, 0.1, W1, False, 2))
    return out


def exact_cost(wp, t, ncoef, w):
    return PR.cost(PR.solve(wp, t, ncoef // 2), np.diff(t), w)


def measure(k, order, mf, w, wp, t):
    ncoef = order + 1
    M = len(t) - 1
    Tmin = R.floor_of(t, mf)
    with PR.on_the_ring():
        J0 = exact_cost(wp, R.start_times(t, Tmin), ncoef, w)
        base.W = w                                            # (slsqp reads the module's weights)
        ta = base.slsqp(wp, t, ncoef, mf)
        Ja = exact_cost(wp, ta, ncoef, w) if np.diff(ta).min() >= Tmin * (1 - 1e-12) else np.inf
        rb = R.optimize(wp, t, w, mf, 2000, 1e-8, ncoef, None)
        Jb = exact_cost(wp, rb["t_out"], ncoef, w)
        r4 = R.optimize(wp, t, w, mf, 500, 1e-4, ncoef, None)
        J4 = exact_cost(wp, r4["t_out"], ncoef, w)
        Jref = min(Ja, Jb)
        best = ta if Ja <= Jb else rb["t_out"]
        act = np.flatnonzero(np.diff(best) - Tmin <= 1e-6 * Tmin)
        even = np.linspace(0.0, t[-1], M + 1)
        even[-1] = t[-1]
        out = dict(J0=J0, J_ref=Jref, J_slsqp=Ja, J_descent=Jb, J4=J4, gap4=(J4 - Jref) / Jref, conv4=r4["pg"] <= 1e-4,
                   active=len(act), iters4=r4["iters"], solves4=r4["solves"], n_below=int((np.diff(t) < Tmin).sum()),
                   J_even=exact_cost(wp, even, ncoef, w), t_even_err=float(np.abs(r4["t_out"] - even).max()),
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
    return out


def one_drone(job):
    k, kind, order, M, mf, w, grid = job
    for attempt in range(MAX_DRAWS):
        rng = np.random.default_rng([SEED, k, attempt])
        wp, t = draw(kind, order, M, rng, grid)
        wp = wp.astype(np.float32).astype(np.float64)
        out = measure(k, order, mf, w, wp, t)
        if out["conv4"] and min(out["p_margin"]) >= MARGIN_MIN:
            break
    out.update(wp=wp, t=t, draws=attempt + 1)
    print(k, kind, "order", order, "M", M, "mf", mf, "draws", attempt + 1, "J/J0 %.4g" % (out["J_ref"] / out["J0"]),
          "a-b %.2e" % ((out["J_slsqp"] - out["J_descent"]) / out["J_ref"]), "gap4 %.2e" % out["gap4"],
          "conv4", bool(out["conv4"]), "active", out["active"], "below", out["n_below"], "iters", out["iters4"],
          "solves", out["solves4"], "margins %.3g %.3g" % tuple(out["p_margin"]),
          "sens %.2e %.2e" % tuple(out["prefix_sens"]), "J4/J_even-1 %.2e" % (out["J4"] / out["J_even"] - 1.0),
          flush=True)
    return out


def check(z):
    """The conditions the fixture was built for (tests/test_timeopt_periodic_cpu.py asserts them on the committed
    file)."""
    seg = np.diff(z["off"]) - 1
    order = z["order"][z["group"]]
    kind = z["kind"][z["group"]]
    n = int(z["n"])
    for o in (7, 9):
        have = set(seg[order == o].tolist())
        assert {2, 3, 10, first_td8(o), SOLVE_CAP[o]} <= have, (o, have)
        assert max(np.bincount(z["group"][(order == o) & (seg == first_td8(o))])) == 11
    assert (z["gap4"] >= -1e-12).all()
    assert np.array_equal(z["J_ref"], np.minimum(z["J_slsqp"], z["J_descent"]))
    assert (z["J_ref"] < z["J0"]).all()
    assert z["shared"].sum() == 1 and (np.asarray(z["weights"]) != 1.0).any(axis=1).sum() == 1
    floor = kind == "floor"
    assert floor.sum() == 3 and (z["active"][floor] > 0).sum() >= 1 and (z["n_below"][floor] > 0).all()
    # lap offsets: nonzero on every axis for the walks, one yaw turn and a closed curve for curve and polygon
    for k in range(n):
        lap = z["wp"][z["off"][k + 1] - 1].astype(np.float64) - z["wp"][z["off"][k]].astype(np.float64)
        if kind[k] in ("curve", "polygon"):
            assert (lap[:3] == 0).all() and abs(lap[3] - 2.0 * np.pi) < 1e-6, (k, lap)
        else:
            assert (lap != 0).all(), (k, lap)
    assert (~z["conv4"]).sum() <= 0.1 * n, int((~z["conv4"]).sum())
    left_out = z["p_margin"] < MARGIN_MIN
    assert left_out.sum() <= 0.1 * 2 * n, int(left_out.sum())
    kept = ~left_out
    assert np.isfinite(z["prefix_sens"][kept]).all() and (z["prefix_sens"][kept] > 0).all()
    poly = kind == "polygon"
    assert poly.sum() == 8 and z["conv4"][poly].all()
    assert (np.abs(z["J4"][poly] / z["J_even"][poly] - 1.0) <= 1e-9).all()
    return int(left_out.sum()), 2 * n


def main():
    jobs, grp = [], []
    gs = groups()
    rng = np.random.default_rng(SEED)
    for gi, (kind, order, M, mf, w, shared, count) in enumerate(gs):
        grid = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, size=M))]) if shared else None
        for _ in range(count):
            jobs.append((len(jobs), kind, order, M, mf, w, grid))
            grp.append(gi)
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(one_drone, jobs, chunksize=1)

    col = lambda key, dt=np.float64: np.array([r[key] for r in res], dtype=dt)   # noqa: E731
    data = dict(
        n=np.int64(len(jobs)), group=np.array(grp, dtype=np.int64), kind=np.array([g[0] for g in gs]),
        order=np.array([g[1] for g in gs], dtype=np.int64), min_fraction=np.array([g[3] for g in gs]),
        weights=np.array([g[4] for g in gs]), shared=np.array([g[5] for g in gs], dtype=bool),
        off=np.concatenate([[0], np.cumsum([len(r["t"]) for r in res])]).astype(np.int64),
        wp=np.concatenate([r["wp"] for r in res]).astype(np.float32), t=np.concatenate([r["t"] for r in res]),
        p_t1=np.concatenate([r["p_t"][0] for r in res]), p_t3=np.concatenate([r["p_t"][1] for r in res]))
    for key in ("J0", "J_ref", "J_slsqp", "J_descent", "J4", "gap4", "J_even", "t_even_err", "p_margin", "prefix_sens"):
        data[key] = col(key)
    for key in ("active", "iters4", "solves4", "n_below", "p_iters", "p_trials", "draws"):
        data[key] = col(key, np.int64)
    data["conv4"] = col("conv4", bool)
    left, runs = check(data)
    for k in np.flatnonzero(~data["conv4"]):
        print("drone", k, "the restatement stopped on max_iter at tol 1e-4: gap4 %.3e" % data["gap4"][k])
    path = os.path.join(HERE, "timeopt_periodic_golden.npz")
    np.savez_compressed(path, **data)
    sens = data["prefix_sens"]
    poly = data["kind"][data["group"]] == "polygon"
    print("wrote", path, os.path.getsize(path), "bytes;", len(jobs), "drones;", left, "of", runs,
          "prefix runs left out; max gap4 %.3e" % data["gap4"].max(), "; J_ref / J0 %.3f .. %.3f" %
          ((data["J_ref"] / data["J0"]).min(), (data["J_ref"] / data["J0"]).max()),
          "; prefix_sens max %.3e" % sens[np.isfinite(sens)].max(),
          "; polygons: J4 / J_even - 1 <= %.2e, |t - even| <= %.2e s" %
          (np.abs(data["J4"][poly] / data["J_even"][poly] - 1.0).max(), data["t_even_err"][poly].max()))


if __name__ == "__main__":
    main()
