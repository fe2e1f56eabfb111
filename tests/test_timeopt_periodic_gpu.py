"""Time allocation on closed loops on the GPU (include/msnap.h, msnap_optimize_times_periodic;
csrc/msnap_timeopt_periodic.hip, timeopt_kernel<K, kTimeoptRing>): the fixture of
tests/golden/make_timeopt_periodic_golden.py (floor, parity with msnap_solve_periodic at both ends of the run,
optimality against the fixture's reference), the prefix of the iteration against the restatement's knots, max_iter = 0,
the seam through msnap_eval_state, the regular polygons, rotation of the cut, bit-identity over positions, tiles, entries
and scale, failed drones, the argument errors and the wrappers.

The tests print what they measure before they assert (run with -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, norm_rel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_exact as PE  # noqa: E402
import states_exact as SE  # noqa: E402
import timeopt_entry_cases as E  # noqa: E402
import timeopt_periodic_ref as PR  # noqa: E402
import timeopt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

W1 = (1.0, 1.0, 1.0, 1.0)
ULP4 = 4 * 2.0 ** -52                # the seam bar of tests/test_periodic_gpu.py
MARGIN_MIN = 1e-3                    # prefix runs below it are left out
FIRST_TD8 = {7: 25, 9: 18}           # the first segment count that runs as 8-drone tiles
_Z = {}
_RUN = {}


def _fixture():
    if not _Z:
        z = np.load(os.path.join(GOLDEN_DIR, "timeopt_periodic_golden.npz"))
        _Z["z"], _Z["cases"] = z, PR.unpack_cases(z)
    return _Z["z"], _Z["cases"]


def _ctx(order, ctx7, ctx9):
    return ctx7 if order == 7 else ctx9


def _group_inputs(drones):
    c0 = drones[0]
    wp = np.stack([c["wp"] for c in drones])
    t = c0["t"] if c0["shared"] else np.stack([c["t"] for c in drones])
    return wp, t


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
        wp, t = _group_inputs(drones)
        _RUN[key] = ctx.optimize_times_periodic(wp, t, drones[0]["weights"], drones[0]["min_fraction"], max_iter, 1e-4)
    return _RUN[key]


def _delta(z):
    """The optimality margin as tests/test_timeopt_states_gpu.py takes it: 100 x the restatement's largest gap over the
    drones on which it converged (the others are held to the restatement's own cost)."""
    return max(100.0 * float(z["gap4"][z["conv4"]].max()), 1e-9)


def _weighted_cost(ctx, coef, dur, w):
    c = ctx.snap_cost(coef, dur)
    return np.array([R.weighted(c[d], w) for d in range(c.shape[0])])


def _same(a, b, ia=slice(None), ib=slice(None)):
    return all(np.array_equal(x[ia], y[ib], equal_nan=True) for x, y in zip(a[:4], b[:4])) and \
        all(np.array_equal(a[4][k][ia], b[4][k][ib], equal_nan=True) for k in ("cost", "pg", "iters"))


def _knot_times(dur):
    """[N, M+1] running sums as msnap_eval_flat accumulates them"""
    ends = np.zeros((dur.shape[0], dur.shape[1] + 1))
    for i in range(dur.shape[1]):
        ends[:, i + 1] = ends[:, i] + dur[:, i]
    return ends


def _over_scale(diff, want, scale):
    """|diff| / max(|want|, scale); an axis that does not move has scale 0 and must agree exactly"""
    den = np.maximum(np.abs(want), scale)
    return np.where(den > 0, np.abs(diff) / np.where(den > 0, den, 1.0), np.where(diff == 0, 0.0, np.inf))


def _seam_ulps(ctx, wp, coef, dur):
    """The largest |state at sum(dur) - state at 0| (position: against wp[M]) over max(|value|, the Horner sum's scale)"""
    K = coef.shape[-1] // 2
    M = dur.shape[1]
    p0, d0 = ctx.eval_state(coef, dur, np.zeros(wp.shape[0]))
    p1, d1 = ctx.eval_state(coef, dur, _knot_times(dur)[:, -1])
    assert np.isfinite(d0).all() and np.isfinite(d1).all() and np.array_equal(p0, wp[:, 0])
    T = dur[:, -1]
    last = np.abs(coef[:, -1])
    worst = 0.0
    for q in range(K):
        scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
        want = wp[:, M] if q == 0 else d0[:, :, q - 1]
        got = p1 if q == 0 else d1[:, :, q - 1]
        worst = max(worst, float(_over_scale(got - want, want, scale).max()))
    return worst


# ---- 1. the fixture -------------------------------------------------------------------------------------------------
def test_fixture_floor_parity_and_optimality(ctx7, ctx9):
    """Measured on an MI355X: delta 7.9e-8; worst gap to J_ref 7.9e-10; no drone of the fixture is one of the
    restatement's max_iter stops; coef is bit for bit msnap_solve_periodic's at t_out on every drone (the bar is 1e-9);
    accepted steps mean 99.7, max 500 (the two order-9 hexagons stop on max_iter at pg 2.7e-4 / 1.9e-4, below J_ref (1 +
    delta) all the same: DESIGN.md K16)."""
    z, cases = _fixture()
    delta = _delta(z)
    worst_gap, worst_held, worst_coef, steps = -1.0, -1.0, 0.0, []
    for g, drones in _groups().items():
        c0 = drones[0]
        ctx = _ctx(c0["order"], ctx7, ctx9)
        w, mf = c0["weights"], c0["min_fraction"]
        wp, t = _group_inputs(drones)
        t_out, coef, dur, status, info = _run_group(ctx, g)
        N, M = wp.shape[0], wp.shape[1] - 1
        tt = np.tile(t, (N, 1)) if t.ndim == 1 else t
        assert (status == 0).all(), (g, status)
        assert (t_out[:, 0] == 0.0).all() and np.array_equal(t_out[:, M], tt[:, M]), g
        assert np.array_equal(dur, t_out[:, 1:] - t_out[:, :-1]), g
        Tmin = mf * tt[:, M] / M
        assert (dur >= Tmin[:, None] * (1 - 1e-12)).all(), (g, dur.min(), Tmin)
        c_0, c_1 = info["cost"][:, 0], info["cost"][:, 1]
        assert (c_1 <= c_0).all(), g
        # parity with the solve entry at both ends of the run
        ts = np.stack([R.start_times(tt[d], Tmin[d]) for d in range(N)])
        cs, ds, ss = ctx.solve_periodic(wp, ts)
        ce, de, se = ctx.solve_periodic(wp, t_out)
        assert (ss == 0).all() and (se == 0).all()
        assert (np.abs(c_0 - _weighted_cost(ctx, cs, ds, w)) <= 1e-9 * c_0).all(), g
        assert (np.abs(c_1 - _weighted_cost(ctx, ce, de, w)) <= 1e-9 * c_1).all(), g
        worst_coef = max(worst_coef, norm_rel(coef, ce))
        assert norm_rel(coef, ce) <= 1e-9, (g, norm_rel(coef, ce))
        assert np.array_equal(dur, de)
        for d, c in enumerate(drones):
            k = c["k"]
            gap = c_1[d] / float(z["J_ref"][k]) - 1.0
            print(f"drone {k}: {c['kind']} order {c['order']} M {M} min_fraction {mf} J/J0 {c_1[d] / c_0[d]:.4g} "
                  f"gap {gap:.3e} pg {info['pg'][d]:.2e} iters {int(info['iters'][d])}")
            if bool(z["conv4"][k]):
                worst_gap = max(worst_gap, gap)
                assert c_1[d] <= float(z["J_ref"][k]) * (1 + delta), (k, gap, delta)
            else:       # the restatement itself stopped on max_iter: held to its cost
                held = c_1[d] / float(z["J4"][k]) - 1.0
                worst_held = max(worst_held, held)
                assert c_1[d] <= float(z["J4"][k]) * (1 + 1e-6), (k, held)
            steps.append(int(info["iters"][d]))
    print(f"fixture: delta {delta:.3e}, worst gap to J_ref {worst_gap:.3e}, worst against a max_iter stop "
          f"{worst_held:.3e}, coef against solve_periodic at t_out {worst_coef:.3e}, accepted steps mean "
          f"{np.mean(steps):.1f} max {max(steps)}")


# ---- 2. the prefix of the iteration -----------------------------------------------------------------------------------
def test_prefix_of_the_iteration(ctx7, ctx9):
    """At max_iter 1 and 3 the accepted steps are the restatement's and the knots its knots within 10 x prefix_sens, its
    own response to gradients off by 2e-6, over the runs with an Armijo margin of at least 1e-3.  Measured on an
    MI355X: 126 runs (none left out), worst 0.200 x prefix_sens."""
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
    assert kept > 0


# ---- 3. max_iter = 0 ---------------------------------------------------------------------------------------------------
def test_no_step_returns_the_raised_input_times(ctx7, ctx9):
    for g, drones in _groups().items():
        c0 = drones[0]
        if c0["kind"] not in ("walk", "floor", "shared"):
            continue
        ctx = _ctx(c0["order"], ctx7, ctx9)
        wp, t = _group_inputs(drones)
        t_out, coef, dur, status, info = _run_group(ctx, g, 0)
        N, M = wp.shape[0], wp.shape[1] - 1
        tt = np.tile(t, (N, 1)) if t.ndim == 1 else t
        want = np.stack([R.start_times(tt[d], R.floor_of(tt[d], c0["min_fraction"])) for d in range(N)])
        assert (status == 0).all() and (info["iters"] == 0).all()
        assert np.array_equal(info["cost"][:, 0], info["cost"][:, 1])
        if c0["kind"] == "floor":
            # raised: the restatement's knots to rounding -- each is a running sum of up to M durations, and a duration
            # is one fma in the kernel and a product and a sum here; a feasible input is taken bit for bit
            assert not np.array_equal(want, tt)
            assert (np.abs(t_out - want) <= 2 * M * 2.0 ** -52 * tt[:, -1:]).all(), np.abs(t_out - want).max()
            assert np.array_equal(t_out[:, M], tt[:, M]) and (t_out[:, 0] == 0).all()
        else:
            assert np.array_equal(t_out, tt)
        ce, de, se = ctx.solve_periodic(wp, t_out)
        assert np.array_equal(dur, de) and norm_rel(coef, ce) <= 1e-9


# ---- 4. the seam --------------------------------------------------------------------------------------------------------
def test_the_seam_through_the_evaluator(ctx7, ctx9):
    """msnap_eval_state at the sum of dur against itself at 0 and against wp[M], within 4 * 2^-52 of the evaluation
    scale, on every group of the fixture -- both caps among them; coef[..., 0] is wp bit for bit.  Measured on an
    MI355X: 0.98 ulp."""
    worst, over, seen = 0.0, [], set()
    for g, drones in _groups().items():
        ctx = _ctx(drones[0]["order"], ctx7, ctx9)
        wp, t = _group_inputs(drones)
        t_out, coef, dur, status, info = _run_group(ctx, g)
        M = wp.shape[1] - 1
        seen.add((drones[0]["order"], M))
        assert np.array_equal(coef[:, :, :, 0], wp[:, :M, :]), g
        r = _seam_ulps(ctx, wp, coef, dur)
        worst = max(worst, r)
        if not r <= ULP4:
            over.append((g, drones[0]["order"], M, r / 2.0 ** -52))
    print(f"seam within {worst / 2.0 ** -52:.2f} ulp of its scale")
    assert {(7, PE.MAX_SEG[7]), (9, PE.MAX_SEG[9])} <= seen
    assert not over, over


# ---- 5. regular polygons ---------------------------------------------------------------------------------------------------
def test_regular_polygons_return_to_the_even_grid(ctx7, ctx9):
    """cost[1] <= J(even) (1 + delta), J(even) from solve_periodic and snap_cost on the even grid.  Measured on an MI355X:
    J / J(even) - 1 between -2.1e-11 and 6.4e-10, |t - even| <= 4.0e-5 s (delta 7.9e-8)."""
    z, cases = _fixture()
    delta = _delta(z)
    n, worst, worst_t = 0, -1.0, 0.0
    for g, drones in _groups().items():
        if drones[0]["kind"] != "polygon":
            continue
        ctx = _ctx(drones[0]["order"], ctx7, ctx9)
        wp, t = _group_inputs(drones)
        M = wp.shape[1] - 1
        t_out, coef, dur, status, info = _run_group(ctx, g)
        even = np.tile(t[0, -1] * np.arange(M + 1) / M, (wp.shape[0], 1))
        even[:, -1] = t[:, -1]
        ce, de, se = ctx.solve_periodic(wp, even)
        J_even = _weighted_cost(ctx, ce, de, W1)
        rel = info["cost"][:, 1] / J_even - 1.0
        worst, worst_t, n = max(worst, rel.max()), max(worst_t, np.abs(t_out - even).max()), n + wp.shape[0]
        print(f"polygon order {drones[0]['order']} M {M}: J / J(even) - 1 {rel.tolist()}, max |t - even| "
              f"{np.abs(t_out - even).max():.2e} s, iters {info['iters'].tolist()}")
        assert (info["cost"][:, 1] <= J_even * (1 + delta)).all(), (g, rel, delta)
    print(f"polygons: {n} drones, worst J / J(even) - 1 = {worst:.3e} (delta {delta:.3e}), |t - even| <= {worst_t:.2e} s")
    assert n == 8


# ---- 6. rotation of the cut --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_where_the_loop_is_cut_does_not_matter(ctx7, ctx9, order):
    """One 10-segment loop cut at knots 0, 1 and M-1: the final costs agree within delta.  Measured on an MI355X:
    1.0e-14 (order 7, 30 steps each), 9.3e-13 (order 9, 109 steps each)."""
    z, cases = _fixture()
    delta = _delta(z)
    ctx = _ctx(order, ctx7, ctx9)
    c = next(c for c in cases if c["order"] == order and c["kind"] == "walk" and len(c["t"]) == 11)
    M = 10
    costs = []
    for j in (0, 1, M - 1):
        wp, t = PE.rotate(c["wp"], c["t"], j)
        r = ctx.optimize_times_periodic(wp[None], t[None], W1, 0.1, 500, 1e-4)
        assert r[3][0] == 0
        costs.append(float(r[4]["cost"][0, 1]))
        print(f"order {order}: cut at knot {j}: J {costs[-1]:.12g} iters {int(r[4]['iters'][0])} pg {r[4]['pg'][0]:.2e}")
    spread = (max(costs) - min(costs)) / min(costs)
    print(f"order {order}: the three cuts agree within {spread:.3e} (delta {delta:.3e})")
    assert spread <= delta


# ---- 7. bit-identity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_position_tile_entry_and_scale(ctx7, ctx9, order):
    import torch
    from drone_path_planning_python_amd import Context
    ctx = _ctx(order, ctx7, ctx9)
    # 16-drone tiles: a full tile and a tail of one; 8-drone tiles: a full tile and a tail of three
    for M, n, places in ((10, 17, (0, 15, 16)), (FIRST_TD8[order], 11, (0, 7, 8, 10))):
        wp, t = PE.case(order, M, N=n)
        whole = ctx.optimize_times_periodic(wp, t, W1, 0.1, 40, 1e-4)
        assert (whole[3] == 0).all() and (whole[4]["iters"] > 0).all()
        for d in places:
            one = ctx.optimize_times_periodic(wp[d:d + 1], t[d:d + 1], W1, 0.1, 40, 1e-4)
            assert _same(whole, one, slice(d, d + 1)), (M, d)
        # the same drone first and last
        w2, t2 = wp.copy(), t.copy()
        w2[0], t2[0], w2[n - 1], t2[n - 1] = wp[3], t[3], wp[3], t[3]
        moved = ctx.optimize_times_periodic(w2, t2, W1, 0.1, 40, 1e-4)
        assert _same(moved, whole, slice(0, 1), slice(3, 4)) and _same(moved, whole, slice(n - 1, n), slice(3, 4)), M
        # waypoints x 4: every quantity of the iteration scales by a power of two
        big = ctx.optimize_times_periodic(4.0 * wp, t, W1, 0.1, 40, 1e-4)
        assert np.array_equal(big[0], whole[0]) and np.array_equal(big[2], whole[2])
        assert np.array_equal(big[4]["iters"], whole[4]["iters"]) and np.array_equal(big[4]["pg"], whole[4]["pg"])
        assert np.array_equal(big[4]["cost"], 16.0 * whole[4]["cost"])
    # host entry against device entry (the last shape: 8-drone tiles)
    dev = torch.device("cuda", 0)
    nc = order + 1
    dw, dt = torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev)
    outs = (torch.empty((n, M + 1), dtype=torch.float64, device=dev),
            torch.empty((n, M, 4, nc), dtype=torch.float64, device=dev),
            torch.empty((n, M), dtype=torch.float64, device=dev), torch.empty((n,), dtype=torch.int32, device=dev),
            torch.empty((n, 2), dtype=torch.float64, device=dev), torch.empty((n,), dtype=torch.float64, device=dev),
            torch.empty((n,), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    with Context(device_id=0, order=order, max_segments=32) as dctx:
        dctx.optimize_times_periodic_device(n, M, dw, dt, 0, W1, 0.1, 40, 1e-4, *outs)
        dctx.sync()
    o = [x.cpu().numpy() for x in outs]
    assert _same(tuple(o[:4]) + ({"cost": o[4], "pg": o[5], "iters": o[6]},), whole)
    # the host entry without its optional outputs against the device entry (one full 16-drone tile and a tail of one)
    E.assert_host_entry_without_optionals_is_the_device_entry(ctx, "_periodic", *PE.case(order, 3, N=17))


# ---- 8. failed drones --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_failed_drones_at_the_edges_of_a_tile(ctx7, ctx9, order):
    """A NaN waypoint (status 3), non-increasing times and t[0] != 0 (status 2), each at the first and last place of a
    full and of a partial tile of both sizes: NaN outputs and iters 0 there, every other drone bitwise what it is
    without them."""
    ctx = _ctx(order, ctx7, ctx9)
    for M, sizes in ((10, (16, 13)), (FIRST_TD8[order], (8, 5))):
        for n in sizes:
            wp, t = PE.case(order, M, N=n)
            good = ctx.optimize_times_periodic(wp, t, W1, 0.1, 30, 1e-4)
            assert (good[3] == 0).all()
            for kind, code in (("nan", 3), ("order", 2), ("t0", 2)):
                w2, t2 = wp.copy(), t.copy()
                for d in (0, n - 1):
                    if kind == "nan":
                        w2[d, M if d else 1, 2] = np.nan          # (the last waypoint is read too)
                    elif kind == "order":
                        t2[d, 2] = t2[d, 1]
                    else:
                        t2[d] = t2[d] + 0.25
                bad = ctx.optimize_times_periodic(w2, t2, W1, 0.1, 30, 1e-4)
                assert bad[3][0] == code and bad[3][n - 1] == code and (bad[3][1:n - 1] == 0).all(), (M, n, kind, bad[3])
                for d in (0, n - 1):
                    assert np.isnan(bad[0][d]).all() and np.isnan(bad[1][d]).all() and np.isnan(bad[2][d]).all()
                    assert np.isnan(bad[4]["cost"][d]).all() and np.isnan(bad[4]["pg"][d]) and bad[4]["iters"][d] == 0
                assert _same(bad, good, slice(1, n - 1), slice(1, n - 1)), (M, n, kind)


# ---- 9. arguments ------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx7, ctx9):
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd._lib import MsnapError
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    for ctx in (ctx7, ctx9):
        lib, order = ctx._lib, ctx.order
        cap = lib.msnap_optimize_times_periodic_max_segments(order)
        assert cap >= lib.msnap_solve_periodic_max_segments(order) == PE.MAX_SEG[order]
        assert cap == {7: 48, 9: 33}[order] == ctx.optimize_times_periodic_max_segments()
        assert lib.msnap_optimize_times_periodic_max_segments(5) == -3       # MSNAP_EORDER
        w = np.ones(4)

        def call(M, wp=True, weights=w, mf=0.1, mi=5, tol=1e-4, h=ctx._h, n=2):
            wpl = np.cumsum(np.ones((2, M + 1, 4)), axis=1) ** 2
            tl = np.tile(np.arange(M + 1.0), (2, 1))
            outs = (np.full((2, M + 1), 7.0), np.full((2, M, 4, order + 1), 7.0), np.full((2, M), 7.0),
                    np.full((2,), 7, dtype=np.int32), np.full((2, 2), 7.0), np.full((2,), 7.0),
                    np.full((2,), 7, dtype=np.int32))
            rc = lib.msnap_optimize_times_periodic(h, n, M, vp(wpl) if wp else None, vp(tl), 0,
                                                   None if weights is None else vp(weights), mf, mi, tol,
                                                   *[vp(o) for o in outs])
            return rc, all((o == 7).all() for o in outs)

        # one segment, one above the cap: refused, nothing written
        for M in (1, cap + 1):
            assert call(M) == (-4, True), M                                    # MSNAP_ESEGMENTS
        assert call(cap)[0] == 0 and call(2) == (0, False)
        for kw in ({"weights": np.array([1.0, -1.0, 1.0, 1.0])}, {"weights": np.array([1.0, np.nan, 1.0, 1.0])},
                   {"weights": np.array([1.0, np.inf, 1.0, 1.0])}, {"weights": None}, {"mf": 0.0}, {"mf": 1.5},
                   {"mi": -1}, {"tol": -1.0}, {"tol": np.nan}, {"wp": False}, {"h": None}, {"n": -1}):
            assert call(3, **kw) == (-1, True), kw                               # MSNAP_EINVAL
        assert call(3, n=0, wp=False) == (0, True)                               # a no-op
        with pytest.raises(MsnapError) as e:
            ctx.optimize_times_periodic(np.zeros((1, 2, 4)), np.arange(2.0))
        assert e.value.code == -4
        empty = ctx.optimize_times_periodic(np.zeros((0, 4, 4)), np.arange(4.0))
        assert empty[0].shape == (0, 4) and empty[1].shape == (0, 3, 4, ctx.ncoef)
    # above the context's max_segments
    with Context(device_id=0, order=7, max_segments=16) as small:
        assert small.optimize_times_periodic_max_segments() == 16
        with pytest.raises(MsnapError) as e:
            small.optimize_times_periodic(np.zeros((1, 18, 4)), np.arange(18.0))
        assert e.value.code == -4


# ---- 10. wrappers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_the_wrappers_and_the_example_pipeline(ctx7, ctx9, order):
    """Context and DeviceCompute against the ctypes call, bit for bit; then the pipeline of
    examples/12_loop_time_allocation.py on 8 drones with 5 segments.  Measured on an MI355X: allocated / even cost
    0.45-0.47 (order 7), 0.32-0.34 (order 9); the join_loop hand-over within 0.66 / 0.64 ulp of its scale."""
    import torch
    from drone_path_planning_python_amd import Context, synthetic
    from drone_path_planning_python_amd.swarm import DeviceCompute, join_loop
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    dev = torch.device("cuda", 0)
    n, M = 8, 5
    wp, t = synthetic.patrol_circuits(n, M)
    assert t.shape == (M + 1,) and np.array_equal(wp[:, M, :3], wp[:, 0, :3])
    legs = np.linalg.norm(np.diff(wp[0, :, :3], axis=0), axis=1)
    assert legs.max() > 2.0 * legs.min()                    # an uneven circuit
    w = np.array([1.0, 1.0, 1.0, 0.5])
    # the ctypes call
    outs = (np.empty((n, M + 1)), np.empty((n, M, 4, 2 * K)), np.empty((n, M)), np.empty((n,), dtype=np.int32),
            np.empty((n, 2)), np.empty((n,)), np.empty((n,), dtype=np.int32))
    rc = ctx._lib.msnap_optimize_times_periodic(ctx._h, n, M, vp(wp), vp(t), 1, vp(w), 0.1, 200, 1e-4,
                                                *[vp(o) for o in outs])
    assert rc == 0 and (outs[3] == 0).all()
    raw = tuple(outs[:4]) + ({"cost": outs[4], "pg": outs[5], "iters": outs[6]},)
    assert _same(ctx.optimize_times_periodic(wp, t, w, 0.1, 200, 1e-4), raw)
    with Context(device_id=0, order=order, max_segments=16) as dctx:
        comp = DeviceCompute(dctx, torch)
        dwp, dt = torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev)
        r = comp.optimize_times_periodic(dwp, dt, tuple(w), 0.1, 200, 1e-4)
        torch.cuda.synchronize()
        got = tuple(x.cpu().numpy() for x in r[:4]) + ({k: v.cpu().numpy() for k, v in r[4].items()},)
        assert _same(got, raw)
        # the example's pipeline: even times against allocated times, then join_loop onto the allocated loops
        ec, ed, es = comp.solve_periodic(dwp, dt)
        torch.cuda.synchronize()
        J_even = _weighted_cost(ctx, ec.cpu().numpy(), ed.cpu().numpy(), w)
        J_alloc = _weighted_cost(ctx, got[1], got[2], w)
        print(f"order {order}: allocated / even cost {np.round(J_alloc / J_even, 4).tolist()}, iters {got[4]['iters'].tolist()}")
        assert (J_alloc < J_even).all() and np.array_equal(got[4]["cost"][:, 1] <= got[4]["cost"][:, 0], np.ones(n, bool))
        wpa, ta, _, _ = SE.case(order, 6, N=n)
        pc, pd, st = comp.solve_states(torch.from_numpy(wpa).to(dev), torch.from_numpy(ta).to(dev))
        lc, ld = r[1], r[2]
        t_r = 0.4 * pd.sum(dim=1)
        pos_r, _ = comp.eval_state(pc, pd, t_r)
        via = (0.5 * (pos_r.clone() + dwp[:, 0]))[:, None, :]
        t_via = torch.tensor([3.0, 6.0], dtype=torch.float64, device=dev)
        jc, jd, jst, (pos, deriv) = join_loop(comp, pc, pd, t_r, lc, ld, via, t_via)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and (jst.cpu().numpy() == 0).all()
        jc, jd = jc.cpu().numpy(), jd.cpu().numpy()
    # the hand-over onto the loop: the joining path ends in the allocated loop's state at 0
    lp, ldv = ctx.eval_state(got[1], got[2], np.zeros(n))
    p1, d1 = ctx.eval_state(jc, jd, _knot_times(jd)[:, -1])
    T = jd[:, -1]
    last = np.abs(jc[:, -1])
    worst = 0.0
    for q in range(K):
        scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
        want = lp if q == 0 else ldv[:, :, q - 1]
        got_q = p1 if q == 0 else d1[:, :, q - 1]
        worst = max(worst, float(_over_scale(got_q - want, want, scale).max()))
    print(f"order {order}: state at the join_loop hand-over continuous within {worst / 2.0 ** -52:.2f} ulp of its scale")
    assert worst <= ULP4
