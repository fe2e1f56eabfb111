"""Time allocation with a free total duration on the GPU (include/msnap.h, msnap_optimize_times_free;
csrc/msnap_timeopt_kernel.h, timeopt_kernel<K, kTimeoptFree>): the fixture of tests/golden/make_timeopt_free_golden.py
(floor, monotonicity, the bound on the total, parity with msnap_solve_states, optimality against the fixture's
reference), the prefix of the iteration against the restatement's knots, the end states through msnap_eval_state,
max_iter = 0, one segment, position independence and the entries, the homogeneous case (Euler's identity and the ratios
of msnap_optimize_times), failed drones at the edges of 8-drone tiles, swarm.replan with a time weight,
swarm.replan_within_limits, and the argument errors.

The tests print what they measure before they assert (run with -s)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, norm_rel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import states_exact as SE  # noqa: E402
import timeopt_entry_cases as E  # noqa: E402
import timeopt_free_ref as FR  # noqa: E402
import timeopt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

W1 = (1.0, 1.0, 1.0, 1.0)
ULP4 = 4 * 2.0 ** -52                # the end-state bar of tests/test_states_gpu.py
MARGIN_MIN = 1e-3                    # prefix runs below it were left out by the generator
_Z = {}
_RUN = {}


def _fixture():
    if not _Z:
        z = np.load(os.path.join(GOLDEN_DIR, "timeopt_free_golden.npz"))
        _Z["z"], _Z["cases"] = z, FR.unpack_cases(z)
    return _Z["z"], _Z["cases"]


def _ctx(order, ctx7, ctx9):
    return ctx7 if order == 7 else ctx9


def _group_inputs(drones):
    """One call's arrays for the drones of a group: a drone without a block gets a row of zeros in it"""
    c0 = drones[0]
    nd = (c0["order"] + 1) // 2 - 1
    wp = np.stack([c["wp"] for c in drones])
    t = c0["t"] if c0["shared"] else np.stack([c["t"] for c in drones])
    start = np.stack([np.zeros((4, nd)) if c["start"] is None else c["start"] for c in drones])
    end = np.stack([np.zeros((4, nd)) if c["end"] is None else c["end"] for c in drones])
    kt = np.array([c["time_weight"] for c in drones])
    return wp, t, start, end, kt


def _groups():
    _, cases = _fixture()
    out = {}
    for c in cases:
        out.setdefault(c["group"], []).append(c)
    return out


def _run_group(ctx, g, max_iter=500):
    """The fixture's group g through the host entry at the GPU test's settings, computed once"""
    key = (g, max_iter)
    if key not in _RUN:
        drones = _groups()[g]
        wp, t, start, end, kt = _group_inputs(drones)
        _RUN[key] = ctx.optimize_times_free(wp, t, start, end, drones[0]["weights"], kt, drones[0]["min_fraction"],
                                            max_iter, 1e-4)
    return _RUN[key]


def _weighted_cost(ctx, coef, dur, w):
    c = ctx.snap_cost(coef, dur)
    return np.array([R.weighted(c[d], w) for d in range(c.shape[0])])


def _same(a, b, ia=slice(None), ib=slice(None)):
    return all(np.array_equal(x[ia], y[ib], equal_nan=True) for x, y in zip(a[:4], b[:4])) and \
        all(np.array_equal(a[4][k][ia], b[4][k][ib], equal_nan=True) for k in ("cost", "pg", "iters"))


# ---- 1. the fixture -------------------------------------------------------------------------------------------------
def test_fixture_guarantees_parity_and_optimality(ctx7, ctx9):
    """Every guarantee of the header on every fixture drone; F at both ends of the run against msnap_solve_states's
    solution there; the gap to F_ref within delta = 100 x the restatement's worst converged gap (stored in the fixture:
    6.9e-7); the drones on which the restatement itself stopped on max_iter held to its F (1 + 1e-6).  Measured on an
    MI355X: worst gap 6.879e-9 (the restatement's own), the two max_iter drones at -8.9e-16 of the restatement's F,
    coefficients at the caps within 9.1e-10 of the dense solve, accepted steps mean 94.4."""
    z, cases = _fixture()
    delta = float(z["delta"])
    worst_gap, worst_held, steps = -1.0, -1.0, []
    for g, drones in _groups().items():
        c0 = drones[0]
        ctx = _ctx(c0["order"], ctx7, ctx9)
        w, mf = c0["weights"], c0["min_fraction"]
        wp, t, start, end, kt = _group_inputs(drones)
        t_out, coef, dur, status, info = _run_group(ctx, g)
        N, M = wp.shape[0], wp.shape[1] - 1
        tt = np.tile(t, (N, 1)) if t.ndim == 1 else t
        assert (status == 0).all(), (g, status)
        assert (t_out[:, 0] == 0.0).all() and np.array_equal(dur, t_out[:, 1:] - t_out[:, :-1]), g
        Tmin = mf * tt[:, M] / M
        assert (dur >= Tmin[:, None] * (1 - 1e-12)).all(), (g, dur.min(), Tmin)
        c_0, c_1 = info["cost"][:, 0], info["cost"][:, 1]
        assert (c_1 <= c_0).all(), g
        assert (t_out[:, M] <= c_0 / kt).all(), g
        ts = np.stack([FR.start_times(tt[d], Tmin[d]) for d in range(N)])
        assert (np.abs(c_1 - (_weighted_cost(ctx, coef, dur, w) + kt * t_out[:, M])) <= 1e-9 * c_1).all(), g
        if M <= ctx.solve_states_max_segments():
            # parity with the solve entry at both ends of the run
            cs, ds, ss = ctx.solve_states(wp, ts, start, end)
            ce, de, se = ctx.solve_states(wp, t_out, start, end)
            assert (ss == 0).all() and (se == 0).all()
            assert (np.abs(c_0 - (_weighted_cost(ctx, cs, ds, w) + kt * ts[:, M])) <= 1e-9 * c_0).all(), g
            assert norm_rel(coef, ce) <= 1e-9, (g, norm_rel(coef, ce))
            assert np.array_equal(dur, de)
        else:
            # past msnap_solve_states's own range (47 / 32 segments) the dense fp64 solve of the restatement stands
            # in; at 79 and 57 segments it is not held to 1e-9 anywhere, and the smoke test's 1e-6 is taken
            for d, c in enumerate(drones):
                ref = FR.S.solve(c["wp"], t_out[d], c["start"], c["end"], (c["order"] + 1) // 2)
                print(f"drone {c['k']}: M {M}, coefficients within {norm_rel(coef[d], ref):.2e} of the dense fp64 solve")
                assert norm_rel(coef[d], ref) <= 1e-6
                F0 = FR.evaluate(c["wp"], ts[d], w, kt[d], c["order"] + 1, c["start"], c["end"])[0]
                assert abs(c_0[d] - F0) <= 1e-6 * F0
        for d, c in enumerate(drones):
            k = c["k"]
            gap = c_1[d] / float(z["F_ref"][k]) - 1.0
            print(f"drone {k}: {c['kind']} order {c['order']} M {M} {c['combo']} min_fraction {mf} F/F0 "
                  f"{c_1[d] / c_0[d]:.4g} T {tt[d, M]:.4g} -> {t_out[d, M]:.4g} (restatement {float(z['T4'][k]):.4g}) "
                  f"gap {gap:.3e} pg {info['pg'][d]:.2e} iters {int(info['iters'][d])} ({int(z['iters4'][k])})")
            if bool(z["conv4"][k]):
                worst_gap = max(worst_gap, gap)
                assert c_1[d] <= float(z["F_ref"][k]) * (1 + delta), (k, gap, delta)
            else:       # the restatement itself stopped on max_iter: held to its cost
                held = c_1[d] / float(z["F4"][k]) - 1.0
                worst_held = max(worst_held, held)
                assert c_1[d] <= float(z["F4"][k]) * (1 + 1e-6), (k, held)
            steps.append(int(info["iters"][d]))
    print(f"fixture: delta {delta:.3e}, worst gap to F_ref {worst_gap:.3e}, worst against a max_iter stop "
          f"{worst_held:.3e}, accepted steps mean {np.mean(steps):.1f} max {max(steps)}")


def test_the_floor_is_met_and_the_total_moves_both_ways(ctx7, ctx9):
    """The "below" group starts from raised times whose total exceeds the input's; the heavy drone of the "span" group
    ends with its first, its last and at least one more segment at the floor; its light one with a longer total."""
    z, cases = _fixture()
    for g, drones in _groups().items():
        kind = drones[0]["kind"]
        if kind not in ("below", "span"):
            continue
        ctx = _ctx(drones[0]["order"], ctx7, ctx9)
        wp, t, start, end, kt = _group_inputs(drones)
        M = wp.shape[1] - 1
        mf = drones[0]["min_fraction"]
        Tmin = mf * t[:, M] / M
        if kind == "below":
            r0 = ctx.optimize_times_free(wp, t, start, end, W1, kt, mf, 0, 1e-4)
            want = np.stack([FR.start_times(t[d], Tmin[d]) for d in range(len(drones))])
            assert np.array_equal(r0[0], want) and (r0[0][:, M] > t[:, M]).all()
            assert (r0[4]["iters"] == 0).all() and np.array_equal(r0[4]["cost"][:, 0], r0[4]["cost"][:, 1])
            assert np.array_equal(r0[4]["cost"][:, 0], _run_group(ctx, g)[4]["cost"][:, 0])
        else:
            t_out, _, dur, _, _ = _run_group(ctx, g)
            at = dur - Tmin[:, None] <= 1e-6 * Tmin[:, None]
            print("span: segments at the floor", at.sum(axis=1).tolist(), "totals", t[:, M].tolist(), "->",
                  t_out[:, M].tolist())
            assert at[0, 0] and at[0, M - 1] and 3 <= at[0].sum() < M
            assert t_out[-1, M] > t[-1, M] and t_out[0, M] < t[0, M]
            assert kt.max() / kt.min() >= 1e3


# ---- 2. the prefix of the iteration -----------------------------------------------------------------------------------
def test_prefix_of_the_iteration(ctx7, ctx9):
    """At max_iter 1 and 3 the accepted steps are the restatement's and the knots -- the last one among them -- are
    within 10 x prefix_sens, its own response to energies off by 2e-6, over the runs the generator kept.  Measured on an
    MI355X: 122 runs, knots within 0.000 x prefix_sens."""
    z, cases = _fixture()
    worst, kept = 0.0, 0
    for g, drones in _groups().items():
        ctx = _ctx(drones[0]["order"], ctx7, ctx9)
        for j, mi in enumerate((1, 3)):
            t_out, coef, dur, status, info = _run_group(ctx, g, mi)
            assert (status == 0).all()
            for d, c in enumerate(drones):
                k = c["k"]
                if z["p_margin"][k, j] < MARGIN_MIN:
                    continue
                kept += 1
                assert int(info["iters"][d]) == int(z["p_iters"][k, j]), (k, mi)
                diff = float(np.abs(t_out[d] - c["p_t"][j]).max() / c["t"][-1])
                ratio = diff / float(z["prefix_sens"][k, j])
                worst = max(worst, ratio)
                assert ratio <= 10.0, (k, mi, diff, float(z["prefix_sens"][k, j]))
    print(f"prefix: {kept} runs, worst |dt| / t[M] = {worst:.3f} x prefix_sens")
    assert kept > 100


# ---- 3. the end states ------------------------------------------------------------------------------------------------
def test_the_given_end_states_are_honoured(ctx7, ctx9):
    """eval_state at 0 returns start and wp[0], at sum(dur) end and wp[M], measured as tests/test_timeopt_states_gpu.py
    measures them: the start relative, the end in units of the Horner sum's scale, both at 4 * 2^-52."""
    worst0, worst1, over = 0.0, 0.0, []
    for g, drones in _groups().items():
        order = drones[0]["order"]
        ctx = _ctx(order, ctx7, ctx9)
        K = (order + 1) // 2
        wp, t, start, end, kt = _group_inputs(drones)
        t_out, coef, dur, status, info = _run_group(ctx, g)
        N, M = wp.shape[0], wp.shape[1] - 1
        assert np.array_equal(coef[:, 0, :, 0], wp[:, 0, :])
        p0, d0 = ctx.eval_state(coef, dur, np.zeros(N))
        assert np.array_equal(p0, wp[:, 0, :])
        rel = np.abs(d0 - start) / np.where(start == 0, 1.0, np.abs(start))
        worst0 = max(worst0, rel.max())
        if not (rel <= ULP4).all():
            over.append((g, "start", rel.max() / 2.0 ** -52))
        total = np.zeros(N)
        for i in range(M):
            total = total + dur[:, i]
        p1, d1 = ctx.eval_state(coef, dur, total)
        assert np.isfinite(d1).all()
        T = dur[:, -1]
        last = np.abs(coef[:, -1])
        for q in range(0, K):
            want = wp[:, M, :] if q == 0 else end[:, :, q - 1]
            got = p1 if q == 0 else d1[:, :, q - 1]
            scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
            r = np.abs(got - want) / np.maximum(np.abs(want), scale)
            worst1 = max(worst1, r.max())
            if not (r <= ULP4).all():
                over.append((g, "end", q, r.max() / 2.0 ** -52))
    print(f"end states: start within {worst0 / 2.0 ** -52:.2f} ulp, end within {worst1 / 2.0 ** -52:.2f} ulp of its scale")
    assert not over, over


# ---- 4. one segment, max_iter 0 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_one_segment_is_a_real_problem(ctx7, ctx9, order):
    """One duration between two given states: it moves, F falls, and the result is msnap_solve_states's for it."""
    ctx = _ctx(order, ctx7, ctx9)
    wp, t, start, end = SE.case(order, 1)
    J = _weighted_cost(ctx, *ctx.solve_states(wp, t, start, end)[:2], W1)
    kt = order * J / t[:, 1] * np.where(np.arange(len(J)) % 2 == 0, 4.0, 0.25)
    r = ctx.optimize_times_free(wp, t, start, end, W1, kt)
    assert (r[3] == 0).all() and (r[4]["iters"] > 0).all()
    assert (r[0][:, 1] != t[:, 1]).all() and (r[4]["cost"][:, 1] < r[4]["cost"][:, 0]).all()
    print(f"order {order}, one segment: T {np.round(t[:4, 1], 3).tolist()} -> {np.round(r[0][:4, 1], 3).tolist()}, "
          f"iters {r[4]['iters'][:4].tolist()}")
    ce, de, se = ctx.solve_states(wp, r[0], start, end)
    assert np.array_equal(r[2], de) and np.array_equal(r[1], ce), norm_rel(r[1], ce)
    r0 = ctx.optimize_times_free(wp, t, start, end, W1, kt, max_iter=0)
    assert np.array_equal(r0[0], t) and (r0[4]["iters"] == 0).all()
    assert np.array_equal(r0[4]["cost"][:, 0], r0[4]["cost"][:, 1])
    assert np.array_equal(r0[4]["cost"][:, 0], r[4]["cost"][:, 0])


# ---- 5. position independence, entries, capture ---------------------------------------------------------------------
def test_the_eight_drone_tile_groups(ctx7, ctx9):
    """The groups above the 16-drone LDS limit (11 drones: a full 8-drone tile and a tail of 3): every drone alone gives
    the bits it gives in the group."""
    seen = set()
    for g, drones in _groups().items():
        if drones[0]["kind"] != "tile8":
            continue
        order = drones[0]["order"]
        ctx = _ctx(order, ctx7, ctx9)
        assert drones[0]["wp"].shape[0] - 1 == {7: 40, 9: 29}[order] and len(drones) == 11
        seen.add(order)
        wp, t, start, end, kt = _group_inputs(drones)
        whole = _run_group(ctx, g)
        for d in (0, 7, 8, 10):
            one = ctx.optimize_times_free(wp[d:d + 1], t[d:d + 1], start[d:d + 1], end[d:d + 1], W1, kt[d:d + 1], 0.1, 500,
                                          1e-4)
            assert _same(whole, one, slice(d, d + 1)), (g, d)
    assert seen == {7, 9}


def test_position_independence_entries_and_capture(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    wp, t, start, end = SE.case(7, 10, N=50)
    kt = 10.0 ** np.random.default_rng(5).uniform(2.0, 5.0, 50)
    one = ctx7.optimize_times_free(wp[5:6], t[5:6], start[5:6], end[5:6], W1, kt[5:6])
    assert one[3][0] == 0 and one[4]["iters"][0] > 2
    for n, pos in ((50, 25), (17, 16)):
        w2, t2, s2, e2, k2 = wp[:n].copy(), t[:n].copy(), start[:n].copy(), end[:n].copy(), kt[:n].copy()
        w2[pos], t2[pos], s2[pos], e2[pos], k2[pos] = wp[5], t[5], start[5], end[5], kt[5]
        assert _same(ctx7.optimize_times_free(w2, t2, s2, e2, W1, k2), one, slice(pos, pos + 1)), (n, pos)
    # NULL against blocks of zeros, a number against an array: the same bits
    zero = np.zeros_like(start[:17])
    a = ctx7.optimize_times_free(wp[:17], t[:17], None, None, W1, 300.0)
    assert _same(a, ctx7.optimize_times_free(wp[:17], t[:17], zero, zero, W1, np.full(17, 300.0)))
    # the host entry without its optional outputs, each state block given and NULL, against the device entry (one full
    # 16-drone tile and a tail of one)
    w3, t3, s3, e3 = SE.case(7, 3, N=17)
    for states in ((s3, e3), (s3, None), (None, e3), (None, None)):
        E.assert_host_entry_without_optionals_is_the_device_entry(ctx7, "_free", w3, t3, states, (kt[:17].copy(),))
    # the device entry, eager and inside a captured graph, on a context of its own
    dev = torch.device("cuda", 0)
    n, m = 17, 10
    host = ctx7.optimize_times_free(wp[:n], t[:n], start[:n], end[:n], W1, kt[:n])
    dw, dt = torch.from_numpy(wp[:n]).to(dev), torch.from_numpy(t[:n]).to(dev)
    ds, de = torch.from_numpy(start[:n]).to(dev), torch.from_numpy(end[:n]).to(dev)
    dk = torch.from_numpy(kt[:n]).to(dev)
    o_t = torch.empty((n, m + 1), dtype=torch.float64, device=dev)
    o_c = torch.empty((n, m, 4, 8), dtype=torch.float64, device=dev)
    o_d = torch.empty((n, m), dtype=torch.float64, device=dev)
    o_s = torch.empty((n,), dtype=torch.int32, device=dev)
    o_j = torch.empty((n, 2), dtype=torch.float64, device=dev)
    o_p = torch.empty((n,), dtype=torch.float64, device=dev)
    o_i = torch.empty((n,), dtype=torch.int32, device=dev)
    outs = (o_t, o_c, o_d, o_s, o_j, o_p, o_i)

    def result():
        return tuple(x.cpu().numpy() for x in (o_t, o_c, o_d, o_s)) + \
            ({"cost": o_j.cpu().numpy(), "pg": o_p.cpu().numpy(), "iters": o_i.cpu().numpy()},)

    def call(ctx):
        ctx.optimize_times_free_device(n, m, dw, dt, 0, ds, de, W1, dk, 0.1, 200, 1e-4, *outs)

    side = torch.cuda.Stream()
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            call(ctx)                                   # once outside the capture (msnap.h, "Stream capture")
            side.synchronize()
            assert _same(result(), host)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                call(ctx)
            ctx.set_stream(side.cuda_stream)
            for x in outs:
                x.zero_()
            g.replay()
            side.synchronize()
            assert _same(result(), host)
        del g


# ---- 6. the homogeneous case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_homogeneous_case_euler_and_the_ratios_of_optimize_times(ctx7, ctx9, order):
    """Both state blocks zero, no floor active: at return |(2k - 1) J - k_T t_out[M]| <= tol sqrt(M) F (derived from the
    stopping measure), and the ratios dur / t_out[M] are msnap_optimize_times's: the rest-to-rest J of the free result's
    durations rescaled to the fixed entry's total is within (1 + delta) of the fixed entry's cost[1].  Measured on an
    MI355X: the miss is 0.02 .. 0.23 of the bound, the rescaled cost within 3.9e-8 of cost[1] (delta 6.9e-7)."""
    from drone_path_planning_python_amd.synthetic import swarm
    ctx = _ctx(order, ctx7, ctx9)
    delta = float(_fixture()[0]["delta"])
    wp, t = swarm(2, 6, 10)
    M, tol = 10, 1e-4
    fixed = ctx.optimize_times(wp, t, W1, 0.01, 2000, tol)
    assert (fixed[3] == 0).all() and (fixed[4]["pg"] <= tol).all()
    kt = order * fixed[4]["cost"][:, 0] / t[:, M] * np.array([0.1, 0.3, 1.0, 1.0, 3.0, 10.0])
    free = ctx.optimize_times_free(wp, t, None, None, W1, kt, 0.01, 2000, tol)
    assert (free[3] == 0).all() and (free[4]["pg"] <= tol).all(), free[4]["pg"]
    Tmin = 0.01 * t[:, M] / M
    assert (free[2] > Tmin[:, None] * (1 + 1e-6)).all()
    T, F = free[0][:, M], free[4]["cost"][:, 1]
    J = F - kt * T
    miss, bound = np.abs(order * J - kt * T), tol * np.sqrt(M) * F
    print(f"order {order}: |(2k-1) J - k_T T| / bound {np.round(miss / bound, 4).tolist()}, totals "
          f"{np.round(t[:, M], 3).tolist()} -> {np.round(T, 3).tolist()}")
    assert (miss <= bound).all()
    knots = free[0] * (t[:, M] / T)[:, None]
    knots[:, M] = t[:, M]
    c, d, s = ctx.solve_batch(wp, knots)
    Jr = _weighted_cost(ctx, c, d, W1)
    rel = Jr / fixed[4]["cost"][:, 1] - 1.0
    print(f"    rescaled to the fixed total: J / cost[1] - 1 = {rel.tolist()} (delta {delta:.3e})")
    assert (s == 0).all() and (Jr <= fixed[4]["cost"][:, 1] * (1 + delta)).all()


# ---- 7. failed drones ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 11])
def test_failed_drones_at_the_edges_of_an_eight_drone_tile(ctx7, n):
    """A NaN waypoint (status 3), non-increasing times (status 2) and a time weight that is zero, negative, infinite or
    NaN (status 3) at the first and last place of a full (n = 8) and of a partial (n = 11: places 8 and 10) 8-drone tile:
    NaN outputs, every other drone untouched."""
    wp, t, start, end = SE.case(7, 40, N=n)
    kt = np.full(n, 2.0e3)
    good = ctx7.optimize_times_free(wp, t, start, end, W1, kt, max_iter=3)
    assert (good[3] == 0).all() and (good[4]["iters"] > 0).all()
    first, last = (0, 7) if n == 8 else (8, 10)
    for faults in (("wp", "t"), ("t", "wp"), (0.0, -1.0), (np.inf, np.nan)):
        w2, t2, k2 = wp.copy(), t.copy(), kt.copy()
        want = {}
        for d, f in zip((first, last), faults):
            if f == "wp":
                w2[d, 17, 2], want[d] = np.nan, 3
            elif f == "t":
                t2[d, 5], want[d] = t2[d, 4], 2
            else:
                k2[d], want[d] = f, 3
        bad = ctx7.optimize_times_free(w2, t2, start, end, W1, k2, max_iter=3)
        keep = np.array([d not in want for d in range(n)])
        for d, code in want.items():
            assert bad[3][d] == code, (faults, d, bad[3])
            assert np.isnan(bad[0][d]).all() and np.isnan(bad[1][d]).all() and np.isnan(bad[2][d]).all()
            assert np.isnan(bad[4]["cost"][d]).all() and np.isnan(bad[4]["pg"][d]) and bad[4]["iters"][d] == 0
        assert _same(bad, good, keep, keep), faults


# ---- 8. swarm.replan with a time weight, swarm.replan_within_limits --------------------------------------------------
def _flying_swarm(torch, comp, seed=8):
    """Example 08's eight drones, left at 40 % of the flight for three new waypoints"""
    from drone_path_planning_python_amd import synthetic
    dev = comp.device
    wp, t = synthetic.swarm(8, 8, 6)
    coef, dur, st = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    t_r = 0.4 * dur.sum(dim=1)
    steps = torch.from_numpy(np.random.default_rng(seed).uniform(-2.0, 2.0, (8, 3, 4))).to(dev)
    pos_r, _ = comp.eval_state(coef, dur, t_r)
    return coef, dur, t_r, (pos_r[:, None, :] + torch.cumsum(steps, dim=1)).clone()


def test_replan_with_a_time_weight(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute, replan
    with Context(device_id=0, order=7, max_segments=16) as dctx:
        comp = DeviceCompute(dctx, torch)
        coef, dur, t_r, wp_new = _flying_swarm(torch, comp)
        t_new = torch.tensor([1.5, 3.0, 4.5], dtype=torch.float64, device=comp.device)
        c0, d0, s0, _ = replan(comp, coef, dur, t_r, wp_new, t_new, optimize={"max_iter": 200})
        c0, d0 = c0.cpu().numpy().copy(), d0.cpu().numpy().copy()
        out = []
        for kw in (30.0, torch.full((8,), 3000.0, dtype=torch.float64, device=comp.device)):
            c1, d1, s1, (pos, deriv) = replan(comp, coef, dur, t_r, wp_new, t_new,
                                              optimize={"time_weight": kw, "max_iter": 200, "tol": 1e-4})
            torch.cuda.synchronize()
            assert (s1.cpu().numpy() == 0).all()
            out.append((c1.cpu().numpy().copy(), d1.cpu().numpy().copy()))
        with pytest.raises(ValueError):
            replan(comp, coef, dur, t_r, wp_new, t_new, optimize={"time_weight": 1.0, "steps": 3})
        pos, deriv = pos.cpu().numpy(), deriv.cpu().numpy()
    assert (np.abs(d0.sum(axis=1) - 4.5) <= 1e-14).all()                       # without a time weight the last time is kept
    totals = [d.sum(axis=1) for _, d in out]
    print("replan: totals at time weight 30", np.round(totals[0], 3).tolist(), "at 3000", np.round(totals[1], 3).tolist())
    assert (totals[1] < totals[0]).all() and (np.abs(totals[0] - 4.5) > 1e-3).all()
    for c1, d1 in out:
        # the hand-over: position bit for bit, derivatives 1 .. K-1 within the start bar of tests/test_states_gpu.py
        assert c1.shape == (8, 3, 4, 8) and np.array_equal(c1[:, 0, :, 0], pos)
        p, dd = ctx7.eval_state(c1, d1, np.zeros(8))
        assert np.array_equal(p, pos)
        rel = np.abs(dd - deriv) / np.where(deriv == 0, 1.0, np.abs(deriv))
        print(f"replan: derivatives continue within {rel.max() / 2.0 ** -52:.2f} ulp")
        assert dd.shape == (8, 4, 3) and (rel <= ULP4).all()


def test_replan_within_limits(ctx7):
    """Eight drones and a guess of 1.5 s for three legs of a few metres each, limits 22 m/s and 60 m/s^2.  Every feasible
    drone's certified peaks are within the limits; the path of its violating weight, when there is one, exceeds a limit;
    a drone whose start speed is above v_max (drone 2 leaves at 25.4 m/s) or whose start acceleration is above a_max
    (drone 1: 118 m/s^2) is reported as not feasible.  Drones 3 .. 6 are within both limits on evenly spaced knots
    anywhere between 2.25 s and 12 s in all (the dense fp64 solve: peaks at most 14.7 m/s and 39.6 m/s^2 at 2.25 s, less
    beyond), a range of 5 in the total and so of 5^8 in the weight, which steps of a factor 4 cannot miss."""
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import PEAK_MARGIN, DeviceCompute, replan, replan_within_limits
    limits = np.array([22.0, 60.0, 0.0, 0.0])
    with Context(device_id=0, order=7, max_segments=16) as dctx:
        comp = DeviceCompute(dctx, torch)
        dev = comp.device
        coef, dur, t_r, wp_new = _flying_swarm(torch, comp)
        t_new = torch.tensor([0.5, 1.0, 1.5], dtype=torch.float64, device=dev)
        _, deriv = comp.eval_state(coef, dur, t_r)
        v0 = torch.linalg.norm(deriv[:, :3, 0], dim=1).cpu().numpy()
        a0 = torch.linalg.norm(deriv[:, :3, 1], dim=1).cpu().numpy()
        hopeless = (v0 > limits[0]) | (a0 > limits[1])
        assert hopeless[1] and hopeless[2] and hopeless.sum() == 2, (v0, a0)
        c, d, st, _ = replan(comp, coef, dur, t_r, wp_new, t_new)
        before = comp.dynamic_peaks(c, d)[0].cpu().numpy().copy()
        c, d, st, (pos, der), info = replan_within_limits(comp, coef, dur, t_r, wp_new, t_new, limits, rounds=8)
        c, d = c.clone(), d.clone()
        peaks = comp.dynamic_peaks(c, d)[0].cpu().numpy().copy()
        assert (st.cpu().numpy() == 0).all() and np.array_equal(peaks, info["peaks"].cpu().numpy())
        feas, kt, kv = info["feasible"], info["time_weight"], info["violating_weight"]
        totals = d.sum(dim=1).cpu().numpy()
        print("replan_within_limits: limits", limits.tolist())
        for k in range(8):
            print(f"  drone {k}: start {v0[k]:.2f} m/s {a0[k]:.2f} m/s^2, feasible {bool(feas[k])} weight {kt[k]:.4g} "
                  f"violating {kv[k]:.4g} total {totals[k]:.3f} s, speed {before[k, 0]:.2f} -> {peaks[k, 0]:.3f}, "
                  f"acceleration {before[k, 1]:.2f} -> {peaks[k, 1]:.3f}")
        assert not feas[hopeless].any() and feas[3:7].all()
        upper = peaks * (1.0 + PEAK_MARGIN)
        assert (upper[feas][:, :2] <= limits[None, :2]).all()
        # the hand-over of the kept paths
        p, dd = ctx7.eval_state(c.cpu().numpy(), d.cpu().numpy(), np.zeros(8))
        assert np.array_equal(p, pos.cpu().numpy())
        ref = der.cpu().numpy()
        assert (np.abs(dd - ref) <= ULP4 * np.where(ref == 0, 1.0, np.abs(ref))).all()
        # the violating weight's path exceeds a limit
        fin = np.isfinite(kv)
        assert fin.any()
        kw = torch.from_numpy(np.where(fin, kv, kt)).to(dev)
        c2, d2, s2, _ = replan(comp, coef, dur, t_r, wp_new, t_new, optimize={"time_weight": kw})
        p2 = comp.dynamic_peaks(c2, d2)[0].cpu().numpy() * (1.0 + PEAK_MARGIN)
        assert ((p2[:, :2] > limits[None, :2]).any(axis=1))[fin].all()
        with pytest.raises(ValueError):
            replan_within_limits(comp, coef, dur, t_r, wp_new, t_new, [1.0, -1.0, 0.0, 0.0])


# ---- 9. argument errors --------------------------------------------------------------------------------------------------
def test_argument_errors(ctx7, ctx9):
    from drone_path_planning_python_amd._lib import MsnapError
    for ctx in (ctx7, ctx9):
        wp, t, start, end = SE.case(ctx.order, 3, N=2)
        for kw in ({"weights": (1, -1, 1, 1)}, {"min_fraction": 0.0}, {"min_fraction": 1.5}, {"max_iter": -1},
                   {"tol": -1.0}, {"weights": (1, np.nan, 1, 1)}):
            with pytest.raises(MsnapError) as e:
                ctx.optimize_times_free(wp, t, start, end, **kw)
            assert e.value.code == -1, kw
        top = ctx.optimize_times_free_max_segments()
        assert top == {7: 79, 9: 57}[ctx.order]
        with pytest.raises(MsnapError) as e:
            ctx.optimize_times_free(np.zeros((1, top + 2, 4)), np.arange(top + 2.0))
        assert e.value.code == -4
        nd = (ctx.order + 1) // 2 - 1
        empty = ctx.optimize_times_free(np.zeros((0, 4, 4)), np.arange(4.0), np.zeros((0, 4, nd)), None)
        assert empty[0].shape == (0, 4) and empty[1].shape == (0, 3, 4, ctx.ncoef)
        # a NULL time_weight on the device entry
        import torch
        dev = torch.device("cuda", 0)
        x = torch.zeros(64, dtype=torch.float64, device=dev)
        with pytest.raises(MsnapError) as e:
            ctx.optimize_times_free_device(1, 1, x, x, 0, None, None, W1, None, 0.1, 1, 1e-4, x, x, x, x)
        assert e.value.code == -1
