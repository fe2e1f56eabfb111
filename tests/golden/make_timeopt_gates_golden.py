"""Writes tests/golden/timeopt_gates_golden.npz: inputs and reference optima for Context.optimize_times_gates.

    python tests/golden/make_timeopt_gates_golden.py     (needs scipy; the tests do not; a few minutes on 8 cores)

Drones as tests/golden/make_timeopt_states_golden.py draws them: durations U(0.5, 2), random-walk waypoints, end-state
and gate values |v|, |a| <= 2, |j| <= 4, |s| <= 8 (tests/states_exact.py::STATE_SCALE).  Every group is one call of the
GPU test and cycles through the four end-state combinations start / end / both / neither:
  * both orders x 2, 3 and 10 segments, four drones each;
  * per order the first segment count that runs as 8-drone tiles (40 at order 7, 29 at order 9: no LDS for the gates,
    so the end-state mode's count), 11 drones: a full tile and a tail of 3;
  * one group on a shared grid, one with min_fraction = 0.5 and legs of very different lengths (an input below the
    floor), one with weights (2, 0.5, 1, 3).
Masks, after tests/gates_exact.py::masks: in every group the drone at place 3 mod 4 carries no gate; a gated drone has
gates at knot 1, at knot 2 (adjacent knots) and at knot M-1, the knots between carry one or, one in two, nothing.  The
gated knots of a group take the non-empty mask values 1 .. 2^(K-1) - 1 in turn, the count running on from group to
group of an order, so that every value occurs in every group with that many gated knots and across the two- and
three-segment groups together.  via holds NaN under every clear bit.

Per drone, as the states fixture records them, every figure from the restatement tests/timeopt_gates_ref.py (the
float64 masked sweep of tests/gates_ref.py): J0; J_slsqp (SLSQP on the closed-form gradient), J_descent (the
restatement at tol 1e-8, 2000 steps), J_ref the smaller; J4, gap4, conv4, iters4, solves4 at the GPU test's settings
(tol 1e-4, 500 steps); the prefix of the iteration at max_iter 1 and 3 -- knots, accepted steps, the smallest Armijo
margin, and prefix_sens, the largest |change of a knot| / t[M] under gradients scaled by 1 +- 2e-6 per segment, and not
less than M 2^-52.  A run whose margin is below 1e-3 is left out of the prefix test; at most a quarter may be, and
every (order, combination) keeps one.  In the min_fraction = 0.5 group the durations are drawn again until one lies
below the floor, so that the start point is a raised one.

The problem is not convex, and with gates the two reference methods can end in different local minima: the descent
converged (measure <= 1e-4) and still SAME_MINIMUM above SLSQP's cost.  Such a drone says nothing about the iteration
-- the optimality margin of the GPU test is 100 x the largest converged gap -- so its waypoints, times, end states and
gate values are drawn again, from a generator of its own (seed, drone, attempt), its masks kept; the log names it.

Waypoints are rounded to float32 before anything is computed; everything is packed into flat arrays
(tests/timeopt_gates_ref.py::unpack_cases reads them)."""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

import make_timeopt_golden as base  # noqa: E402
import make_timeopt_states_golden as states  # noqa: E402
import make_timeopt_wide_golden as wide  # noqa: E402
import timeopt_gates_ref as G  # noqa: E402
import timeopt_ref as R  # noqa: E402
from states_exact import STATE_SCALE  # noqa: E402

W1 = states.W1
W_MIXED = states.W_MIXED
COMBOS = states.COMBOS
SEGMENTS = (2, 3, 10)
MARGIN_MIN = wide.MARGIN_MIN
SEED = 20261021
SAME_MINIMUM = 1e-6      # a converged gap4 above it: the descent and SLSQP found different minima
first_td8 = states.first_td8      # (the gates take no LDS: the end-state mode's tile sizes)


class MaskCycle:
    """the non-empty masks of an order, in turn"""

    def __init__(self, order):
        self.nm = 2 ** ((order + 1) // 2 - 1)
        self.count = 0

    def next(self):
        v = 1 + self.count % (self.nm - 1)
        self.count += 1
        return v


def gate_values(rng, order, fix):
    nd = (order + 1) // 2 - 1
    via = rng.uniform(-1.0, 1.0, (len(fix), 4, nd)) * np.array(STATE_SCALE[:nd])
    used = ((fix[:, None] >> np.arange(nd)[None, :]) & 1).astype(bool)
    return np.where(used[:, None, :], via, np.nan)


def gates(rng, order, M, gated, cycle):
    fix = np.zeros((M - 1,), dtype=np.int32)
    if gated:
        for i in range(1, M):
            if i in (1, 2, M - 1) or rng.random() < 0.5:
                fix[i - 1] = cycle.next()
    return fix, gate_values(rng, order, fix)


def drawn_again(job, attempt):
    """The job of a drone whose reference methods disagreed, with everything but its masks drawn again"""
    k, order, mf, w, wp, t, combo, start, end, fix, via = job
    rng = np.random.default_rng([SEED, k, attempt])
    wp, t, combo, start, end = states.drone(rng, order, len(t) - 1, combo, uneven=mf == 0.5)
    return (k, order, mf, w, wp.astype(np.float32).astype(np.float64), t, combo, start, end, fix,
            gate_values(rng, order, fix))


def groups():
    """[(order, min_fraction, weights, shared, [(wp, t, combo, start, end, fix, via), ..])]: one call of the GPU test
    per entry."""
    rng = np.random.default_rng(SEED)
    cycles = {7: MaskCycle(7), 9: MaskCycle(9)}

    def group(order, M, n, **kw):
        out = []
        for i in range(n):
            d = states.drone(rng, order, M, COMBOS[i % 4], **kw)
            out.append(d + gates(rng, order, M, i % 4 != 3, cycles[order]))
        return out

    out = []
    for order in (7, 9):
        for M in SEGMENTS:
            out.append((order, 0.1, W1, False, group(order, M, 4)))
    for order in (7, 9):
        out.append((order, 0.1, W1, False, group(order, first_td8(order), 11)))
    grid = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, size=10))])
    out.append((9, 0.1, W1, True, group(9, 10, 4, t=grid)))
    out.append((7, 0.5, W1, False, group(7, 10, 4, uneven=True)))
    out.append((7, 0.1, W_MIXED, False, group(7, 10, 4)))
    return out


def exact_cost(wp, t, ncoef, w, start, end, fix, via):
    return G.cost(G.solve(wp, t, start, end, fix, via, ncoef // 2), np.diff(t), w)


def one_drone(job):
    k, order, mf, w, wp, t, combo, start, end, fix, via = job
    ncoef = order + 1
    M = len(t) - 1
    Tmin = R.floor_of(t, mf)
    ec = lambda tk: exact_cost(wp, tk, ncoef, w, start, end, fix, via)      # noqa: E731
    with G.given_gates(start, end, fix, via):
        J0 = ec(R.start_times(t, Tmin))
        base.W = w                                            # (slsqp reads the module's weights)
        ta = base.slsqp(wp, t, ncoef, mf)
        Ja = ec(ta) if np.diff(ta).min() >= Tmin * (1 - 1e-12) else np.inf
        rb = R.optimize(wp, t, w, mf, 2000, 1e-8, ncoef, None)
        Jb = ec(rb["t_out"])
        r4 = R.optimize(wp, t, w, mf, 500, 1e-4, ncoef, None)
        J4 = ec(r4["t_out"])
        Jref = min(Ja, Jb)
        best = ta if Ja <= Jb else rb["t_out"]
        act = np.flatnonzero(np.diff(best) - Tmin <= 1e-6 * Tmin)
        out = dict(J0=J0, J_ref=Jref, J_slsqp=Ja, J_descent=Jb, J4=J4, gap4=(J4 - Jref) / Jref, conv4=r4["pg"] <= 1e-4,
                   active=len(act), act=act, iters4=r4["iters"], solves4=r4["solves"], n_below=int((np.diff(t) < Tmin).sum()),
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
    print(k, "order", order, "M", M, combo, "gated knots", int((fix != 0).sum()), "mf", mf, "J/J0 %.4g" % (Jref / J0),
          "a-b %.2e" % ((Ja - Jb) / Jref), "gap4 %.2e" % out["gap4"], "conv4", bool(out["conv4"]), "active",
          out["active"], "below", out["n_below"], "iters", r4["iters"], "solves", r4["solves"],
          "margins %.3g %.3g" % tuple(out["p_margin"]), "sens %.2e %.2e" % tuple(out["prefix_sens"]), flush=True)
    return out


def check(z):
    """The conditions the fixture was built for (tests/test_timeopt_gates_cpu.py asserts them on the committed file)."""
    seg = np.diff(z["off"]) - 1
    assert np.array_equal(np.diff(z["goff"]), seg - 1)
    order = z["order"][z["group"]]
    ngroups = len(z["order"])
    for o in (7, 9):
        have = set(seg[order == o].tolist())
        assert set(SEGMENTS) | {first_td8(o)} <= have, (o, have)
        assert max(np.bincount(z["group"][(order == o) & (seg == first_td8(o))])) == 11
        nm = 2 ** ((o + 1) // 2 - 1)
        used = set()
        for g in np.flatnonzero(z["order"] == o):
            vals = set()
            for k in np.flatnonzero(z["group"] == g):
                f = z["fix"][z["goff"][k]:z["goff"][k + 1]]
                vals |= set(f[f != 0].tolist())
            n_gated = sum(int((z["fix"][z["goff"][k]:z["goff"][k + 1]] != 0).sum()) for k in np.flatnonzero(z["group"] == g))
            assert n_gated < nm - 1 or vals == set(range(1, nm)), (o, g, vals)
            used |= vals
        assert used == set(range(1, nm)), (o, used)
    for g in range(ngroups):
        ks = np.flatnonzero(z["group"] == g)
        gated = np.array([(z["fix"][z["goff"][k]:z["goff"][k + 1]] != 0).any() for k in ks])
        assert gated.any() and not gated.all(), g                 # some drones in every group carry no gate
        for k in ks[gated]:
            f = z["fix"][z["goff"][k]:z["goff"][k + 1]]
            assert f[0] != 0 and f[-1] != 0 and (len(f) < 2 or f[1] != 0), k      # knot 1, knot M-1, adjacent knots
    nd = (order + 1) // 2 - 1
    for k in range(int(z["n"])):
        f, v = z["fix"][z["goff"][k]:z["goff"][k + 1]], z["via"][z["goff"][k]:z["goff"][k + 1]]
        used = ((f[:, None] >> np.arange(4)[None, :]) & 1).astype(bool)
        assert (f >= 0).all() and (f < 2 ** nd[k]).all()
        assert np.isfinite(v[np.broadcast_to(used[:, None, :], v.shape)]).all()
        assert (np.abs(np.nan_to_num(v)) <= np.array(STATE_SCALE[:4])).all()
    assert (z["gap4"] >= -1e-12).all() and (z["gap4"][z["conv4"]] <= SAME_MINIMUM).all()
    assert np.array_equal(z["J_ref"], np.minimum(z["J_slsqp"], z["J_descent"]))
    assert (z["J_ref"] < z["J0"]).all()
    assert z["shared"].sum() == 1 and (np.asarray(z["weights"]) != 1.0).any(axis=1).sum() == 1
    floor = z["min_fraction"][z["group"]] == 0.5
    assert floor.sum() == 4 and (z["n_below"][floor] > 0).all()
    left_out = z["p_margin"] < MARGIN_MIN
    assert left_out.sum() <= 0.25 * left_out.size, (int(left_out.sum()), left_out.size)
    kept = ~left_out
    assert np.isfinite(z["prefix_sens"][kept]).all() and (z["prefix_sens"][kept] > 0).all()
    for o in (7, 9):
        for c in COMBOS:
            assert kept[(order == o) & (z["combo"] == c)].any(), (o, c)
    return int(left_out.sum()), int(left_out.size)


def main():
    jobs, grp = [], []
    gs = groups()
    for gi, (order, mf, w, shared, drones) in enumerate(gs):
        for wp, t, combo, start, end, fix, via in drones:
            wp = wp.astype(np.float32).astype(np.float64)
            jobs.append((len(jobs), order, mf, w, wp, t, combo, start, end, fix, via))
            grp.append(gi)
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(one_drone, jobs, chunksize=1)
        for attempt in range(1, 6):
            again = [k for k, r in enumerate(res) if r["conv4"] and r["gap4"] > SAME_MINIMUM]
            if not again:
                break
            for k in again:
                assert not gs[grp[k]][3], "a drone of the shared-grid group cannot change its times"
                print("drone", k, "gap4 %.3e with the descent converged: drawn again, attempt" % res[k]["gap4"], attempt)
                jobs[k] = drawn_again(jobs[k], attempt)
            for k, r in zip(again, pool.map(one_drone, [jobs[k] for k in again], chunksize=1)):
                res[k] = r

    def block(x, shape):
        out = np.full(shape, np.nan) if x is not None and x.ndim == 3 else np.zeros(shape)
        if x is not None:
            out[..., :x.shape[-1]] = x
        return out

    col = lambda key, dt=np.float64: np.array([r[key] for r in res], dtype=dt)   # noqa: E731
    data = dict(
        n=np.int64(len(jobs)), group=np.array(grp, dtype=np.int64), order=np.array([g[0] for g in gs], dtype=np.int64),
        min_fraction=np.array([g[1] for g in gs]), weights=np.array([g[2] for g in gs]),
        shared=np.array([g[3] for g in gs], dtype=bool), combo=np.array([j[6] for j in jobs]),
        off=np.concatenate([[0], np.cumsum([len(j[5]) for j in jobs])]).astype(np.int64),
        goff=np.concatenate([[0], np.cumsum([len(j[9]) for j in jobs])]).astype(np.int64),
        wp=np.concatenate([j[4] for j in jobs]).astype(np.float32), t=np.concatenate([j[5] for j in jobs]),
        start=np.array([block(j[7], (4, 4)) for j in jobs]), end=np.array([block(j[8], (4, 4)) for j in jobs]),
        fix=np.concatenate([j[9] for j in jobs]).astype(np.int32),
        via=np.concatenate([block(j[10], (len(j[9]), 4, 4)) for j in jobs]),
        p_t1=np.concatenate([r["p_t"][0] for r in res]), p_t3=np.concatenate([r["p_t"][1] for r in res]))
    for key in ("J0", "J_ref", "J_slsqp", "J_descent", "J4", "gap4", "p_margin", "prefix_sens"):
        data[key] = col(key)
    for key in ("active", "iters4", "solves4", "n_below", "p_iters", "p_trials"):
        data[key] = col(key, np.int64)
    data["conv4"] = col("conv4", bool)
    left, runs = check(data)
    for k in np.flatnonzero(~data["conv4"]):
        print("drone", k, "the restatement stopped on max_iter at tol 1e-4: gap4 %.3e" % data["gap4"][k])
    path = os.path.join(HERE, "timeopt_gates_golden.npz")
    np.savez_compressed(path, **data)
    sens = data["prefix_sens"]
    print("wrote", path, os.path.getsize(path), "bytes;", len(jobs), "drones;", left, "of", runs,
          "prefix runs left out; max gap4 %.3e" % data["gap4"].max(), "; J_ref / J0 %.3f .. %.3f" %
          ((data["J_ref"] / data["J0"]).min(), (data["J_ref"] / data["J0"]).max()),
          "; prefix_sens max %.3e" % sens[np.isfinite(sens)].max())


if __name__ == "__main__":
    main()
