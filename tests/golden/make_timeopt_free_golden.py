"""Writes tests/golden/timeopt_free_golden.npz: inputs and reference optima for Context.optimize_times_free.

    python tests/golden/make_timeopt_free_golden.py     (NumPy only; about a minute on 8 cores)

Drones as tests/golden/make_timeopt_states_golden.py draws them: durations U(0.5, 2), random-walk waypoints (steps in
[-2, 2]), state values within tests/states_exact.py::STATE_SCALE; waypoints rounded to float32 before anything is
computed.  A drone's time weight is f k_0 with k_0 = (2k - 1) J(input times) / t[M] -- the weight at which the input's
total would be stationary if the cost were homogeneous -- and f log-uniform in [0.1, 10] unless said otherwise.  Every
group is one call of the GPU test and cycles through the state combinations start / end / both / neither:
  * "walk": both orders x 1, 2, 3, 10 and 20 segments (2, 2, 2, 4, 2 drones);
  * "tile8": per order the first segment count that runs as 8-drone tiles (40 at order 7, 29 at order 9), 11 drones: a
    full tile and a tail of 3;
  * "cap": the largest segment counts, 79 and 57, two drones each;
  * "shared": one grid for the call; "weights": axis weights (2, 0.5, 1, 3);
  * "below": min_fraction 0.5 and durations drawn until one lies below the floor, so that the start point is a raised
    one and its total is larger than the input's;
  * "span": min_fraction 0.5 and f = 100, 10, 1, 1e-3 in one call.  The first drone's outer legs are a twentieth of
    the others' and it is drawn again until, at the reference, at least 3 but not all of its segments end at the
    floor, the first and the last among them; under the last weight the total grows above the input's.

Per drone, every figure from the restatement tests/timeopt_free_ref.py: F0 at the raised input times; F_ref, the run
at tol 1e-6 (100 x tighter than the GPU test's) and up to 20000 steps, with iters_ref, pg_ref; F4, gap4 = F4 / F_ref - 1,
conv4, iters4, solves4, T4 (the total) at the GPU test's settings (tol 1e-4, 500 steps); `active`, the segments of the
reference within 1e-6 of the floor, with first_active / last_active; the prefix of the iteration at max_iter 1 and 3
-- knots, accepted steps, the smallest Armijo margin, and prefix_sens as make_timeopt_states_golden.py defines it
(the response of the knots to energies off by 2e-6 per segment, not less than M 2^-52).  `delta` is the optimality
margin the GPU test uses: 100 x the largest gap4 over the drones with conv4, not less than 1e-9."""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

import timeopt_free_ref as FR  # noqa: E402
import timeopt_states_ref as S  # noqa: E402
from states_exact import STATE_SCALE  # noqa: E402

W1 = (1.0, 1.0, 1.0, 1.0)
W_MIXED = (2.0, 0.5, 1.0, 3.0)
COMBOS = ("start", "end", "both", "neither")
WALK = ((1, 2), (2, 2), (3, 2), (10, 4), (20, 2))      # (segments, drones)
FIRST_TD8 = {7: 40, 9: 29}
MAX_SEG = {7: 79, 9: 57}
SPAN = (100.0, 10.0, 1.0, 1e-3)
MARGIN_MIN = 1e-3
NOISE = 2e-6
SEED = 20261020


def drone(rng, order, M, combo, uneven=False, t=None, factor=None):
    nd = (order + 1) // 2 - 1
    while t is None:
        t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, size=M))])
        if uneven and not (np.diff(t) < FR.floor_of(t, 0.5)).any():
            t = None
    steps = rng.uniform(-2.0, 2.0, size=(M + 1, 4))
    if uneven:
        steps *= rng.choice([0.1, 1.0, 3.0], size=(M + 1, 1))
    wp = np.cumsum(steps, axis=0)
    scale = np.array(STATE_SCALE[:nd])
    start = rng.uniform(-1.0, 1.0, (4, nd)) * scale if combo in ("start", "both") else None
    end = rng.uniform(-1.0, 1.0, (4, nd)) * scale if combo in ("end", "both") else None
    f = float(10.0 ** rng.uniform(-1.0, 1.0)) if factor is None else factor
    return wp, t, combo, start, end, f


def heavy_drone(rng, order, M, f):
    """A drone whose first and last leg are short, drawn until the weight f k_0 puts the first, the last and at least
    one more segment -- but not every one -- at the floor of min_fraction 0.5."""
    while True:
        wp, t, combo, start, end, _ = drone(rng, order, M, "neither", factor=f)
        leg = np.diff(wp, axis=0)
        leg[0] *= 0.05
        leg[-1] *= 0.05
        wp = np.concatenate([wp[:1], wp[:1] + np.cumsum(leg, axis=0)]).astype(np.float32).astype(np.float64)
        kT = float(f * order * S.cost(S.solve(wp, t, None, None, (order + 1) // 2), np.diff(t), W1) / t[-1])
        r = FR.optimize(wp, t, None, None, W1, kT, 0.5, 20000, 1e-6, order + 1)
        Tmin = FR.floor_of(t, 0.5)
        act = np.flatnonzero(np.diff(r["t_out"]) - Tmin <= 1e-6 * Tmin)
        if 3 <= len(act) < M and 0 in act and M - 1 in act:
            return wp, t, combo, start, end, f


def groups():
    """[(kind, order, min_fraction, weights, shared, [(wp, t, combo, start, end, f), ..])]: one call each"""
    rng = np.random.default_rng(SEED)
    out = []
    c = 0
    for order in (7, 9):
        for M, n in WALK:
            out.append(("walk", order, 0.1, W1, False, [drone(rng, order, M, COMBOS[(c + i) % 4]) for i in range(n)]))
            c += n
    for order in (7, 9):
        out.append(("tile8", order, 0.1, W1, False,
                    [drone(rng, order, FIRST_TD8[order], COMBOS[i % 4]) for i in range(11)]))
    for order in (7, 9):
        out.append(("cap", order, 0.1, W1, False, [drone(rng, order, MAX_SEG[order], COMBOS[2 * i]) for i in range(2)]))
    grid = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, size=10))])
    out.append(("shared", 9, 0.1, W1, True, [drone(rng, 9, 10, cb, t=grid) for cb in COMBOS]))
    out.append(("weights", 7, 0.1, W_MIXED, False, [drone(rng, 7, 10, cb) for cb in COMBOS]))
    out.append(("below", 7, 0.5, W1, False, [drone(rng, 7, 10, cb, uneven=True) for cb in COMBOS]))
    out.append(("span", 9, 0.5, W1, False, [heavy_drone(rng, 9, 10, SPAN[0])] + [drone(rng, 9, 10, "neither", factor=f) for f in SPAN[1:]]))
    return out


def prefix(wp, t, start, end, w, kT, mf, max_iter, ncoef, noise_seed=None):
    """The restatement's first `max_iter` accepted steps; with a seed, on energies scaled by 1 +- NOISE per segment."""
    trace, noise = [], None
    if noise_seed is not None:
        rng = np.random.default_rng(noise_seed)
        noise = lambda g: kT + (g - kT) * (1.0 + NOISE * rng.uniform(-1, 1, size=g.shape))   # noqa: E731
    r = FR.optimize(wp, t, start, end, w, kT, mf, max_iter, 1e-4, ncoef, trace=trace, grad_noise=noise)
    return r, trace


def one_drone(job):
    k, kind, order, mf, w, wp, t, combo, start, end, f = job
    ncoef = order + 1
    M = len(t) - 1
    Tmin = FR.floor_of(t, mf)
    J_in = S.cost(S.solve(wp, t, start, end, ncoef // 2), np.diff(t), w)
    kT = float(f * order * J_in / t[-1])                       # 2k - 1 = order
    ts = FR.start_times(t, Tmin)
    F0 = FR.evaluate(wp, ts, w, kT, ncoef, start, end)[0]
    rr = FR.optimize(wp, t, start, end, w, kT, mf, 20000, 1e-6, ncoef)
    r4 = FR.optimize(wp, t, start, end, w, kT, mf, 500, 1e-4, ncoef)
    Fref = min(rr["cost"], r4["cost"])
    act = np.flatnonzero(np.diff(rr["t_out"]) - Tmin <= 1e-6 * Tmin)
    out = dict(time_weight=kT, factor=f, F0=F0, F_ref=Fref, F4=r4["cost"], gap4=r4["cost"] / Fref - 1.0,
               conv4=r4["pg"] <= 1e-4, conv_ref=rr["pg"] <= 1e-6, pg_ref=rr["pg"], iters_ref=rr["iters"],
               iters4=r4["iters"], solves4=r4["solves"], T4=float(r4["t_out"][-1]), T_ref=float(rr["t_out"][-1]),
               T_start=float(ts[-1]), active=len(act), first_active=bool(0 in act), last_active=bool(M - 1 in act),
               n_below=int((np.diff(t) < Tmin).sum()), p_t=[], p_iters=[], p_trials=[], p_margin=[], prefix_sens=[])
    for mi in (1, 3):
        r, trace = prefix(wp, t, start, end, w, kT, mf, mi, ncoef)
        rn, tn = prefix(wp, t, start, end, w, kT, mf, mi, ncoef, noise_seed=1000 * k + mi)
        margin = min((m for _, _, m in trace), default=np.inf)
        same = [a for _, a, _ in trace] == [a for _, a, _ in tn]
        assert same or margin < MARGIN_MIN, (k, mi, margin)        # noise of 2e-6 flips no decision 1e-3 away
        out["p_t"].append(r["t_out"])
        out["p_iters"].append(r["iters"])
        out["p_trials"].append(len(trace))
        out["p_margin"].append(margin)
        sens = float(np.abs(rn["t_out"] - r["t_out"]).max() / t[-1]) if same else np.inf
        out["prefix_sens"].append(max(sens, M * 2.0 ** -52))
    print(k, kind, "order", order, "M", M, combo, "mf", mf, "f %.3g" % f, "F/F0 %.4g" % (Fref / F0),
          "T %.4g -> %.4g" % (t[-1], out["T_ref"]), "gap4 %.2e" % out["gap4"], "conv4", bool(out["conv4"]),
          "ref", rr["iters"], "%.1e" % rr["pg"], "active", out["active"], out["first_active"], out["last_active"],
          "below", out["n_below"], "iters", r4["iters"], "solves", r4["solves"],
          "margins %.3g %.3g" % tuple(out["p_margin"]), "sens %.2e %.2e" % tuple(out["prefix_sens"]), flush=True)
    return out


def check(z):
    """The conditions the fixture was built for (tests/test_timeopt_free_cpu.py asserts them on the committed file)."""
    n = int(z["n"])
    seg = np.diff(z["off"]) - 1
    order = z["order"][z["group"]]
    kind = z["kind"][z["group"]]
    for o in (7, 9):
        have = set(seg[order == o].tolist())
        assert {1, 2, 3, 10, 20, FIRST_TD8[o], MAX_SEG[o]} <= have, (o, have)
        assert max(np.bincount(z["group"][(order == o) & (seg == FIRST_TD8[o])])) == 11
    assert set(z["combo"].tolist()) == set(COMBOS)
    assert (z["gap4"] >= 0).all() and (z["F_ref"] < z["F0"]).all() and (z["F4"] < z["F0"]).all()
    assert (~z["conv4"]).sum() <= 0.05 * n, int((~z["conv4"]).sum())
    assert z["shared"].sum() == 1 and (np.asarray(z["weights"]) != 1.0).any(axis=1).sum() == 1
    below = kind == "below"
    assert below.sum() == 4 and (z["n_below"][below] > 0).all() and (z["T_start"][below] > z["T_in"][below]).all()
    span = np.flatnonzero(kind == "span")
    tw = z["time_weight"][span]
    assert len(span) == 4 and tw.max() / tw.min() >= 1e3
    heavy, light = span[0], span[-1]
    assert z["active"][heavy] >= 3 and z["first_active"][heavy] and z["last_active"][heavy], z["active"][heavy]
    assert z["active"][heavy] < seg[heavy]
    assert z["T_ref"][light] > z["T_in"][light] and z["T4"][light] > z["T_in"][light]
    runs = np.ones(n, dtype=bool)
    left_out = z["p_margin"] < MARGIN_MIN
    assert left_out.sum() <= 0.25 * 2 * n, int(left_out.sum())
    kept = ~left_out
    assert np.isfinite(z["prefix_sens"][kept]).all() and (z["prefix_sens"][kept] > 0).all()
    for o in (7, 9):
        for c in COMBOS:
            assert kept[(order == o) & (z["combo"] == c)].any(), (o, c)
    return int(left_out.sum()), int(2 * runs.sum())


def main():
    jobs, grp = [], []
    gs = groups()
    for gi, (kind, order, mf, w, shared, drones) in enumerate(gs):
        for wp, t, combo, start, end, f in drones:
            wp = wp.astype(np.float32).astype(np.float64)
            jobs.append((len(jobs), kind, order, mf, w, wp, t, combo, start, end, f))
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
        n=np.int64(len(jobs)), group=np.array(grp, dtype=np.int64), kind=np.array([g[0] for g in gs]),
        order=np.array([g[1] for g in gs], dtype=np.int64), min_fraction=np.array([g[2] for g in gs]),
        weights=np.array([g[3] for g in gs]), shared=np.array([g[4] for g in gs], dtype=bool),
        combo=np.array([j[7] for j in jobs]),
        off=np.concatenate([[0], np.cumsum([len(j[6]) for j in jobs])]).astype(np.int64),
        wp=np.concatenate([j[5] for j in jobs]).astype(np.float32), t=np.concatenate([j[6] for j in jobs]),
        T_in=np.array([j[6][-1] for j in jobs]),
        start=np.array([block(j[8]) for j in jobs]), end=np.array([block(j[9]) for j in jobs]),
        p_t1=np.concatenate([r["p_t"][0] for r in res]), p_t3=np.concatenate([r["p_t"][1] for r in res]))
    for key in ("time_weight", "factor", "F0", "F_ref", "F4", "gap4", "pg_ref", "T4", "T_ref", "T_start", "p_margin",
                "prefix_sens"):
        data[key] = col(key)
    for key in ("active", "iters_ref", "iters4", "solves4", "n_below", "p_iters", "p_trials"):
        data[key] = col(key, np.int64)
    for key in ("conv4", "conv_ref", "first_active", "last_active"):
        data[key] = col(key, bool)
    data["delta"] = np.float64(max(100.0 * float(data["gap4"][data["conv4"]].max()), 1e-9))
    left, runs = check(data)
    for k in np.flatnonzero(~data["conv4"]):
        print("drone", k, "the restatement stopped on max_iter at tol 1e-4: gap4 %.3e" % data["gap4"][k])
    path = os.path.join(HERE, "timeopt_free_golden.npz")
    np.savez_compressed(path, **data)
    sens = data["prefix_sens"]
    print("wrote", path, os.path.getsize(path), "bytes;", len(jobs), "drones in", len(gs), "calls;", left, "of", runs,
          "prefix runs left out; max gap4 %.3e" % data["gap4"].max(), "delta %.3e" % data["delta"],
          "; reference unconverged on", int((~data["conv_ref"]).sum()),
          "; prefix_sens max %.3e" % sens[np.isfinite(sens)].max())


if __name__ == "__main__":
    main()
