"""Inputs of tests/golden/chain_bits_*.npz, shared by their recorder (tests/golden/make_chain_bits_golden.py) and
tests/test_chain_bits_gpu.py: the kernels that run the open-chain elimination and tests/rolled_bits_cases.py does not
reach -- gates_solve_kernel<K> (K21) and the rest, end-state and free-total modes of timeopt_kernel<K, MODE> (K8) -- at
the smallest shapes that reach every branch of it, clean and with failed drones injected."""
import os

import numpy as np

ST_TIMES, ST_NONFINITE = 2, 3      # MSNAP_ST_* of include/msnap.h
GUARD = 2                          # drone rows behind the batch that a launch must leave alone
W = (1.0, 1.0, 1.0, 1.0)
MIN_FRACTION, TOL = 0.1, 1e-4
# accepted steps after which a case with max_iter > 0 stops: a small number, and on the long paths the smallest round
# one past the restatement's first rejected trial (its steps double from a quarter of the shortest segment: 8 to 17
# accepted steps come first there)
MAX_ITER, MAX_ITER_WIDE = 5, 20


def _nu(order):
    return (order + 1) // 2 - 1


# ------------------------------------------------------------------------------------------------------------------
# K21: msnap_solve_gates
# ------------------------------------------------------------------------------------------------------------------
GATE_CAP = {7: 47, 9: 32}          # StatesLayout<K>::max_segments()
MASKS = ("none", "all", "mixed")
GATE_BATCHES = ("clean", "faults")


def _gcase(order, m, n, masks, combo="both"):
    return {"kind": "gates", "order": order, "m": m, "n": n, "masks": masks, "combo": combo}


# one gated knot, two knots, the entry's segment limit; every mask pattern at each; once without end states
GATES = [_gcase(o, m, n, k) for o in (7, 9) for m, n in ((2, 17), (3, 17), (GATE_CAP[o], 3)) for k in MASKS]
GATES += [_gcase(o, 3, 17, "mixed", "neither") for o in (7, 9)]


def gate_inputs(c, batch):
    """(wp, t, start, end, fix [n, m-1] int32, via [n, m-1, 4, K-1]) of one batch.  "none": a mask array of zeros (the
    plain step at every knot); "all": every bit at every knot; "mixed": odd knots gated by no drone, even knots by every
    second drone with masks that differ (with one knot, m = 2: that knot counts as even).  Unused values are NaN."""
    from drone_path_planning_python_amd.synthetic import swarm
    order, m, n, nu = c["order"], c["m"], c["n"], _nu(c["order"])
    wp, t = swarm(6100 + 31 * m + order, n, m)
    rng = np.random.default_rng(8800 + 31 * m + order)
    scale = np.array((2.0, 2.0, 4.0, 8.0)[:nu])
    both = rng.uniform(-1.0, 1.0, (2, n, 4, nu)) * scale
    start = both[0] if c["combo"] == "both" else None
    end = both[1] if c["combo"] == "both" else None
    full = (1 << nu) - 1
    fix = np.zeros((n, m - 1), np.int32)
    if c["masks"] == "all":
        fix[:] = full
    elif c["masks"] == "mixed":
        for i in range(m - 1):                        # knot i + 1
            if m == 2 or (i + 1) % 2 == 0:
                for d in range(0, n, 2):
                    fix[d, i] = 1 + (d // 2 + i) % full
    via = rng.uniform(-1.0, 1.0, (n, m - 1, 4, nu)) * scale
    used = ((fix[:, :, None] >> np.arange(nu)[None, None, :]) & 1).astype(bool)      # [n, m-1, nu]
    via = np.where(used[:, :, None, :], via, np.nan)
    if batch == "faults":
        # a mask outside 0 .. 2^NU - 1 on drone 1 (below it at the first knot, above it at the last), a prescribed value
        # that is not finite on the last drone; both next to healthy drones of the same tile
        fix[1, 0] = -1 if c["masks"] != "all" else full + 1
        fix[n - 1, m - 2] |= 1
        via[n - 1, m - 2, 2, 0] = np.inf
    elif batch != "clean":
        raise ValueError(batch)
    return wp, t, start, end, fix, via


def gate_changed(c, batch):
    return {} if batch == "clean" else {1: ST_NONFINITE, c["n"] - 1: ST_NONFINITE}


# ------------------------------------------------------------------------------------------------------------------
# K8: msnap_optimize_times, _states, _free
# ------------------------------------------------------------------------------------------------------------------
MODES = ("rest", "ends", "free")
# the first segment count at which a tile of 16 drones no longer fits 160 KiB of LDS (timeopt_lds_words of
# csrc/msnap_timeopt_kernel.h: 512 M - 224 doubles at order 7, 688 M + 280 at order 9, plus 384 / 640 with the state
# images, against 20480), so that the launch takes 8-drone tiles and lanes 32..63 replay
WIDE = {("rest", 7): 41, ("ends", 7): 40, ("free", 7): 40, ("rest", 9): 30, ("ends", 9): 29, ("free", 9): 29}
TIMEOPT_BATCHES = ("clean", "faults")


def _tcase(mode, order, m, n, max_iter=MAX_ITER, shared=False, combo="both"):
    return {"kind": "timeopt", "mode": mode, "order": order, "m": m, "n": n, "max_iter": max_iter, "shared": shared,
            "combo": "rest" if mode == "rest" else combo}


def _tcases(mode, order):
    out = [_tcase(mode, order, 1, 17), _tcase(mode, order, 2, 17), _tcase(mode, order, 3, 17),
           _tcase(mode, order, 3, 17, max_iter=0), _tcase(mode, order, 3, 17, shared=True),
           _tcase(mode, order, WIDE[mode, order], 9, max_iter=MAX_ITER_WIDE)]
    if mode != "rest":
        out.append(_tcase(mode, order, 3, 17, combo="neither"))
    return out


TIMEOPT = [c for o in (7, 9) for mode in MODES for c in _tcases(mode, o)]
CASES = GATES + TIMEOPT

# Seeds of the K8 cases and, per case, one drone of each tile on which tests/timeopt_ref.py (and its states / free
# siblings) takes at least one accepted and one rejected trial, each decided by more than 1e-6 of the cost
# (make_chain_bits_golden.py --search wrote this table on the CPU; the recorder and the test assert iters >= 1 for these
# drones on the GPU).  Cases that cannot move are absent: max_iter 0, and one segment with the total duration kept.
SEEDS = {
    "rest_o7_m2_n17_it5_rest": 0,
    "rest_o7_m3_n17_it5_rest": 0,
    "rest_o7_m3_n17_it5_shared_rest": 0,
    "rest_o7_m41_n9_it20_rest": 0,
    "ends_o7_m2_n17_it5_both": 0,
    "ends_o7_m3_n17_it5_both": 0,
    "ends_o7_m3_n17_it5_shared_both": 0,
    "ends_o7_m40_n9_it20_both": 0,
    "ends_o7_m3_n17_it5_neither": 0,
    "free_o7_m1_n17_it5_both": 2,
    "free_o7_m2_n17_it5_both": 0,
    "free_o7_m3_n17_it5_both": 0,
    "free_o7_m3_n17_it5_shared_both": 0,
    "free_o7_m40_n9_it20_both": 0,
    "free_o7_m3_n17_it5_neither": 0,
    "rest_o9_m2_n17_it5_rest": 0,
    "rest_o9_m3_n17_it5_rest": 0,
    "rest_o9_m3_n17_it5_shared_rest": 0,
    "rest_o9_m30_n9_it20_rest": 0,
    "ends_o9_m2_n17_it5_both": 0,
    "ends_o9_m3_n17_it5_both": 0,
    "ends_o9_m3_n17_it5_shared_both": 0,
    "ends_o9_m29_n9_it20_both": 0,
    "ends_o9_m3_n17_it5_neither": 0,
    "free_o9_m1_n17_it5_both": 2,
    "free_o9_m2_n17_it5_both": 11,
    "free_o9_m3_n17_it5_both": 14,
    "free_o9_m3_n17_it5_shared_both": 0,
    "free_o9_m29_n9_it20_both": 0,
    "free_o9_m3_n17_it5_neither": 14,
}
MOVERS = {
    "rest_o7_m2_n17_it5_rest": [0, 16],
    "rest_o7_m3_n17_it5_rest": [2, 16],
    "rest_o7_m3_n17_it5_shared_rest": [0, 16],
    "rest_o7_m41_n9_it20_rest": [0, 8],
    "ends_o7_m2_n17_it5_both": [0, 16],
    "ends_o7_m3_n17_it5_both": [2, 16],
    "ends_o7_m3_n17_it5_shared_both": [0, 16],
    "ends_o7_m40_n9_it20_both": [0, 8],
    "ends_o7_m3_n17_it5_neither": [2, 16],
    "free_o7_m1_n17_it5_both": [3, 16],
    "free_o7_m2_n17_it5_both": [3, 16],
    "free_o7_m3_n17_it5_both": [2, 16],
    "free_o7_m3_n17_it5_shared_both": [0, 16],
    "free_o7_m40_n9_it20_both": [0, 8],
    "free_o7_m3_n17_it5_neither": [2, 16],
    "rest_o9_m2_n17_it5_rest": [0, 16],
    "rest_o9_m3_n17_it5_rest": [2, 16],
    "rest_o9_m3_n17_it5_shared_rest": [0, 16],
    "rest_o9_m30_n9_it20_rest": [0, 8],
    "ends_o9_m2_n17_it5_both": [0, 16],
    "ends_o9_m3_n17_it5_both": [2, 16],
    "ends_o9_m3_n17_it5_shared_both": [0, 16],
    "ends_o9_m29_n9_it20_both": [0, 8],
    "ends_o9_m3_n17_it5_neither": [2, 16],
    "free_o9_m1_n17_it5_both": [10, 16],
    "free_o9_m2_n17_it5_both": [6, 16],
    "free_o9_m3_n17_it5_both": [1, 16],
    "free_o9_m3_n17_it5_shared_both": [0, 16],
    "free_o9_m29_n9_it20_both": [0, 8],
    "free_o9_m3_n17_it5_neither": [1, 16],
}


def tile_drones(c):
    return 8 if c["m"] >= WIDE[c["mode"], c["order"]] else 16


def can_move(c):
    return c["max_iter"] > 0 and not (c["m"] == 1 and c["mode"] != "free")


def timeopt_inputs(c, batch, seed=None):
    """(wp, t, start, end, time_weight [n] or None) of one batch."""
    from drone_path_planning_python_amd.synthetic import swarm
    order, m, n, nu = c["order"], c["m"], c["n"], _nu(c["order"])
    if seed is None:
        seed = SEEDS.get(case_id(c), 0)
    wp, t = swarm(9400 + seed, n, m, shared_times=c["shared"])
    rng = np.random.default_rng(9900 + seed)
    scale = np.array((2.0, 2.0, 4.0, 8.0)[:nu])
    both = rng.uniform(-1.0, 1.0, (2, n, 4, nu)) * scale
    kT = 10.0 ** rng.uniform(4.0, 7.0, n)      # (the price of a second, around the cost's own slope: J is 1e5 .. 1e7)
    start = both[0] if c["combo"] == "both" else None
    end = both[1] if c["combo"] == "both" else None
    if batch == "faults":      # a NaN waypoint and a segment that runs backwards, both inside the first tile
        wp[1, m // 2, 1] = np.nan
        j = max(m - 2, 0)
        t[n - 2, j + 1] = t[n - 2, j] - 0.125
    elif batch != "clean":
        raise ValueError(batch)
    return wp, t, start, end, (kT if c["mode"] == "free" else None)


def timeopt_changed(c, batch):
    return {} if batch == "clean" else {1: ST_NONFINITE, c["n"] - 2: ST_TIMES}


# ------------------------------------------------------------------------------------------------------------------
def case_id(c):
    if c["kind"] == "gates":
        return f"gates_o{c['order']}_m{c['m']}_n{c['n']}_{c['masks']}_{c['combo']}"
    return (f"{c['mode']}_o{c['order']}_m{c['m']}_n{c['n']}_it{c['max_iter']}" + ("_shared" if c["shared"] else "") +
            f"_{c['combo']}")


def key(c, batch, field):
    return f"{case_id(c)}/{batch}/{field}"


def golden_path(c):
    name = "chain_bits_gates.npz" if c["kind"] == "gates" else f"chain_bits_timeopt_o{c['order']}.npz"
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)


def batches(c):
    if c["kind"] == "gates":
        return GATE_BATCHES
    return ("clean",) if c["shared"] or c["max_iter"] == 0 else TIMEOPT_BATCHES


def changed(c, batch):
    return gate_changed(c, batch) if c["kind"] == "gates" else timeopt_changed(c, batch)


def fields(c):
    return ("coef", "dur", "status") if c["kind"] == "gates" else ("t_out", "coef", "dur", "status", "cost", "pg",
                                                                   "iters")


def stored_rows(c, batch, field):
    """The drones of `field` the archive holds: all of "clean", elsewhere of the large fields only the changed ones."""
    if batch == "clean" or field not in ("coef", "dur", "t_out"):
        return list(range(c["n"]))
    return sorted(changed(c, batch))


def expected_status(c, batch):
    st = np.zeros(c["n"], np.int32)
    for d, s in changed(c, batch).items():
        st[d] = s
    return st


_SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.int64).view(np.float64)[0]


def run(ctx, c, batch):
    """One launch of the case's entry into sentinel-filled device outputs that are GUARD drones longer than the batch;
    returns {field: numpy array of the batch} after checking that the rows behind it kept the sentinel."""
    import torch
    n, m = c["n"], c["m"]
    dev = torch.device("cuda", ctx.device_id)
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    f64 = lambda *shape: torch.full(shape, _SENTINEL, dtype=torch.float64, device=dev)           # noqa: E731
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)                    # noqa: E731
    out = {"coef": f64(n + GUARD, m, 4, ctx.order + 1), "dur": f64(n + GUARD, m), "status": i32(n + GUARD)}
    if c["kind"] == "gates":
        wp, t, start, end, fix, via = (up(x) for x in gate_inputs(c, batch))
        torch.cuda.synchronize(dev)
        ctx.solve_gates_device(n, m, wp, t, False, start, end, fix, via, out["coef"], out["dur"], out["status"])
    else:
        out.update({"t_out": f64(n + GUARD, m + 1), "cost": f64(n + GUARD, 2), "pg": f64(n + GUARD),
                    "iters": i32(n + GUARD)})
        wp, t, start, end, kT = (up(x) for x in timeopt_inputs(c, batch))
        tail = (MIN_FRACTION, c["max_iter"], TOL, out["t_out"], out["coef"], out["dur"], out["status"], out["cost"],
                out["pg"], out["iters"])
        torch.cuda.synchronize(dev)
        if c["mode"] == "rest":
            ctx.optimize_times_device(n, m, wp, t, c["shared"], W, *tail)
        elif c["mode"] == "ends":
            ctx.optimize_times_states_device(n, m, wp, t, c["shared"], start, end, W, *tail)
        else:
            ctx.optimize_times_free_device(n, m, wp, t, c["shared"], start, end, W, kT, *tail)
    ctx.sync()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    want = np.array([_SENTINEL]).view(np.int64)[0]
    for k, v in out.items():
        behind = v[n:]
        ok = (behind == -7).all() if v.dtype == np.int32 else (behind.view(np.int64) == want).all()
        assert ok, f"{case_id(c)}/{batch}: {k} written past the batch"
    return {k: v[:n] for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def check(c, batch, got, clean):
    """What keeps the archive from hiding a failure: the expected status words, finite results for every healthy drone
    and NaN for every failed one, the untouched drones bit for bit as in the clean batch, and -- K8, clean batches that
    can move -- at least one accepted step on the drones named in MOVERS."""
    what = (case_id(c), batch)
    want = expected_status(c, batch)
    assert np.array_equal(got["status"], want), (what, got["status"].tolist())
    real = [k for k in fields(c) if got[k].dtype == np.float64]
    for k in real:
        assert np.isfinite(got[k][want == 0]).all(), (what, k)
        if k != "dur" or c["kind"] == "timeopt":      # (the solves write a failed drone's durations as they are)
            assert np.isnan(got[k][want != 0]).all(), (what, k)
    if "iters" in got:
        assert (got["iters"][want != 0] == 0).all(), what
        assert (got["iters"] <= c["max_iter"]).all(), what
    same = [d for d in range(c["n"]) if d not in changed(c, batch)]
    for k in fields(c):
        assert np.array_equal(bits(got[k][same]), bits(clean[k][same])), (what, k)
    if c["kind"] == "timeopt" and batch == "clean" and can_move(c):
        movers = MOVERS[case_id(c)]
        assert sorted({d // tile_drones(c) for d in movers}) == list(range(-(-c["n"] // tile_drones(c)))), what
        assert (got["iters"][movers] >= 1).all(), (what, got["iters"].tolist())
