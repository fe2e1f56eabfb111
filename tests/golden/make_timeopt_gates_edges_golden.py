"""Writes tests/golden/timeopt_gates_edges_golden.npz: the reference figures of Context.optimize_times_gates at the
caps and edges, on the inputs tests/timeopt_gates_cases.py builds (the file holds no input: only what costs more than
a second or two to compute).

    python tests/golden/make_timeopt_gates_edges_golden.py     (needs scipy; the tests do not; some minutes on 8 cores)

The groups, one call of the GPU test each (tests/timeopt_gates_cases.py::groups):
  * cap7 / cap9: 79 segments at order 7, 57 at order 9 -- msnap_optimize_times_gates_max_segments, where a full
    8-drone tile fills the LDS -- 11 drones, a full tile and a tail of 3.  The end-state combinations cycle start /
    neither / both / end, so that drones 7 and 10, the last of the full tile and the last of the call, carry an `end`
    block; every given state is non-zero.  Drones at place 3 mod 4 carry no gate; a gated drone gates knots 1, 2, M-2,
    M-1, at order 7 also knots 63, 64 and 65 (segments 64 .. are the second word of the free-set bitmask), and one in
    two of the knots between; the mask values cycle through 1 .. 2^(K-1) - 1.
  * cap7_plain / cap9_plain: the same drones without a gate, the end-state mode's problem at its cap.
  * floor7: cap7 with the durations of segments 60, 64, 68, 72 and 76 times 0.15, min_fraction = 0.5: an input below
    the floor on both sides of segment 64.
  * stiff7 / stiff9: tests/gates_cases.py::stiff, six segments alternating 1.5 s and 1.5 / R s.

Per drone, by tests/golden/make_timeopt_gates_golden.py::one_drone (imported, not copied): J0; J_ref, the smaller of
SLSQP and the restatement at tol 1e-8 with 2000 steps; J4, gap4, conv4, iters4, solves4 at tol 1e-4 with 500 steps; the
prefix at max_iter 1 and 3 (knots, accepted steps, trials, smallest Armijo margin, prefix_sens); n_below; the reference's
active set as segment indices (act, aoff).

Conditions, asserted here and again by tests/test_timeopt_gates_edges_cpu.py on the committed file: every non-empty
mask value occurs in each cap group and each gated drone of order 7 has gated knots on both sides of knot 64;
J_ref < J0; gap4 >= -1e-12; a converged drone has gap4 <= 1e-6 -- one that has not (the descent and SLSQP ended in
different minima) is drawn again by make_timeopt_gates_golden.py::drawn_again with its masks kept, and since that rule
draws from a generator the tests cannot run without scipy, the file records such a drone's waypoints (float32, exact),
times, end states and gate values (r_k, r_attempt, r_off, r_goff, r_wp, r_t, r_start, r_end, r_via: the one kind of
input the file holds; tests/timeopt_gates_cases.py::groups(z) puts them in place; a drawn floor7 drone gets the
squeezed segments again, a stiff one keeps its durations); at most a quarter of the prefix runs have a margin below
1e-3; in floor7 every drone has at least 3 durations below the floor, at least
4 drones have an active segment with index >= 64, at least 2 of them gated, and at least one drone has active
segments on both sides of 64.  The drones the restatement stops on max_iter at tol 1e-4 are named in the log; the
GPU test holds them to J4."""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

import make_timeopt_gates_golden as gates  # noqa: E402
import timeopt_gates_cases as TC  # noqa: E402
import timeopt_ref as R  # noqa: E402

MARGIN_MIN = gates.MARGIN_MIN
SAME_MINIMUM = gates.SAME_MINIMUM
NAME = "timeopt_gates_edges_golden.npz"


def drawn_again(job, attempt, name):
    """gates.drawn_again -- everything but the masks from a generator of (seed, drone, attempt) -- and then what the
    drone's group adds to a drawn drone: floor7 its squeezed segments; a stiff group keeps its durations"""
    new = list(gates.drawn_again(job, attempt))
    if name == "floor7":
        new[5] = TC.squeezed(new[5])
    elif name.startswith("stiff"):
        new[5] = job[5]
    return tuple(new)


def check(z, groups):
    """The conditions the fixture was built for"""
    names = [str(x) for x in z["gname"]]
    assert names == [g[0] for g in groups]
    seg = np.diff(z["off"]) - 1
    for gi, (name, order, mf, combos, batch) in enumerate(groups):
        ks = np.flatnonzero(z["group"] == gi)
        assert len(ks) == batch[0].shape[0] and (seg[ks] == batch[0].shape[1] - 1).all(), name
    for order in (7, 9):
        fix = TC.cap(order)[4]
        nm = 2 ** ((order + 1) // 2 - 1)
        assert set(fix[fix != 0].tolist()) == set(range(1, nm)), order
        gated = fix.any(axis=1)
        assert gated.tolist() == [d % 4 != 3 for d in range(TC.N_CAP)]
        if order == 7:      # knot i is column i - 1
            assert (fix[gated][:, :TC.WORD - 1] != 0).any(axis=1).all() and (fix[gated][:, TC.WORD:] != 0).any(axis=1).all()
    assert (z["J_ref"] < z["J0"]).all()
    assert (z["gap4"] >= -1e-12).all() and (z["gap4"][z["conv4"]] <= SAME_MINIMUM).all()
    assert np.array_equal(z["J_ref"], np.minimum(z["J_slsqp"], z["J_descent"]))
    left_out = z["p_margin"] < MARGIN_MIN
    assert left_out.sum() <= 0.25 * left_out.size, (int(left_out.sum()), left_out.size)
    assert np.isfinite(z["prefix_sens"][~left_out]).all() and (z["prefix_sens"][~left_out] > 0).all()
    # the floor group
    gi = names.index("floor7")
    ks = np.flatnonzero(z["group"] == gi)
    fix = groups[gi][4][4]
    assert (z["n_below"][ks] >= 3).all(), z["n_below"][ks]
    acts = [z["act"][z["aoff"][k]:z["aoff"][k + 1]] for k in ks]
    high = np.array([(a >= TC.WORD).any() for a in acts])
    both = np.array([(a >= TC.WORD).any() and (a < TC.WORD).any() for a in acts])
    assert high.sum() >= 4 and (high & fix.any(axis=1)).sum() >= 2 and both.any(), (high, both)
    return int(left_out.sum()), int(left_out.size)


def main():
    groups = TC.groups()
    jobs, grp = [], []
    for gi, (name, order, mf, combos, batch) in enumerate(groups):
        for d, combo in enumerate(combos):
            wp, t, start, end, fix, via = TC.drone_of(batch, combo, d)
            jobs.append((len(jobs), order, mf, TC.W1, wp, t, combo, start, end, fix, via))
            grp.append(gi)
    redrawn = {}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(gates.one_drone, jobs, chunksize=1)
        for attempt in range(1, 9):
            again = [k for k, r in enumerate(res) if r["conv4"] and r["gap4"] > SAME_MINIMUM]
            if not again:
                break
            for k in again:
                print("drone", k, "of", groups[grp[k]][0], "gap4 %.3e with the descent converged: drawn again, attempt" %
                      res[k]["gap4"], attempt)
                jobs[k] = drawn_again(jobs[k], attempt, groups[grp[k]][0])
                redrawn[k] = attempt
            for k, r in zip(again, pool.map(gates.one_drone, [jobs[k] for k in again], chunksize=1)):
                res[k] = r
    assert not [k for k, r in enumerate(res) if r["conv4"] and r["gap4"] > SAME_MINIMUM]

    def block(x, shape, fill):
        out = np.full(shape, fill)
        if x is not None:
            out[..., :x.shape[-1]] = x
        return out

    rk = sorted(redrawn)
    col = lambda key, dt=np.float64: np.array([r[key] for r in res], dtype=dt)   # noqa: E731
    data = dict(
        n=np.int64(len(jobs)), group=np.array(grp, dtype=np.int64), gname=np.array([g[0] for g in groups]),
        order=np.array([g[1] for g in groups], dtype=np.int64), min_fraction=np.array([g[2] for g in groups]),
        off=np.concatenate([[0], np.cumsum([len(j[5]) for j in jobs])]).astype(np.int64),
        aoff=np.concatenate([[0], np.cumsum([len(r["act"]) for r in res])]).astype(np.int64),
        act=np.concatenate([np.asarray(r["act"], dtype=np.int64) for r in res]),
        p_t1=np.concatenate([r["p_t"][0] for r in res]), p_t3=np.concatenate([r["p_t"][1] for r in res]),
        # the drones drawn again: everything but their masks (the waypoints are float32 numbers, held exactly)
        r_k=np.array(rk, dtype=np.int64), r_attempt=np.array([redrawn[k] for k in rk], dtype=np.int64),
        r_off=np.concatenate([[0], np.cumsum([len(jobs[k][5]) for k in rk])]).astype(np.int64),
        r_goff=np.concatenate([[0], np.cumsum([len(jobs[k][9]) for k in rk])]).astype(np.int64),
        r_wp=np.concatenate([jobs[k][4] for k in rk] + [np.zeros((0, 4))]).astype(np.float32),
        r_t=np.concatenate([jobs[k][5] for k in rk] + [np.zeros((0,))]),
        r_start=np.array([block(jobs[k][7], (4, 4), 0.0) for k in rk]).reshape(-1, 4, 4),
        r_end=np.array([block(jobs[k][8], (4, 4), 0.0) for k in rk]).reshape(-1, 4, 4),
        r_via=np.concatenate([block(jobs[k][10], (len(jobs[k][9]), 4, 4), np.nan) for k in rk] + [np.zeros((0, 4, 4))]))
    for key in ("J0", "J_ref", "J_slsqp", "J_descent", "J4", "gap4", "p_margin", "prefix_sens"):
        data[key] = col(key)
    for key in ("iters4", "solves4", "n_below", "p_iters", "p_trials"):
        data[key] = col(key, np.int64)
    data["conv4"] = col("conv4", bool)
    left, runs = check(data, groups)
    for k in np.flatnonzero(~data["conv4"]):
        print("drone", k, "of", groups[grp[k]][0], "the restatement stopped on max_iter at tol 1e-4: gap4 %.3e" %
              data["gap4"][k])
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **data)
    sens = data["prefix_sens"]
    print("wrote", path, os.path.getsize(path), "bytes;", len(jobs), "drones;", left, "of", runs,
          "prefix runs left out; max converged gap4 %.3e" % data["gap4"][data["conv4"]].max(),
          "; J_ref / J0 %.3f .. %.3f" % ((data["J_ref"] / data["J0"]).min(), (data["J_ref"] / data["J0"]).max()),
          "; prefix_sens max %.3e" % sens[np.isfinite(sens)].max(), "; min margin %.3g" % data["p_margin"].min())


if __name__ == "__main__":
    main()
