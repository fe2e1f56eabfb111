"""Replanning in flight on the GPU (include/msnap.h, "replanning in flight"): msnap_solve_states
against the 60-digit collocation of tests/states_exact.py and against the properties a boundary-state solve must have,
msnap_eval_state against its NumPy restatement and msnap_eval_flat, and swarm.replan."""
import ctypes
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import states_exact as SE  # noqa: E402
from conftest import norm_rel  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT_BAR = 1e-10                   # HIP kernels against 60-digit solutions (tests/test_solve_gpu.py)
FORM_BAR = {7: 1e-11, 9: 1e-9}      # two solve forms against each other (test_twisted_and_one_sided_kernels_agree)
ULP4 = 4 * 2.0 ** -52


def _ctx(order, ctx7, ctx9):
    return ctx7 if order == 7 else ctx9


def _seg_counts(order):
    return [1, 2, 3, 10, SE.MAX_SEG[order]]


_SOLVED = {}


def _solved(ctx, order, M):
    """{combo: (coef, dur, status)} of case(order, M): solved once, shared by the tests below"""
    key = (order, M)
    if key not in _SOLVED:
        wp, t, start, end = SE.case(order, M)
        _SOLVED[key] = {c: ctx.solve_states(wp, t, *SE.combo_states(c, start, end)) for c in SE.COMBOS}
    return _SOLVED[key]


def _knot_times(dur):
    """[N, M+1] running sums as msnap_eval_flat accumulates them"""
    ends = np.zeros((dur.shape[0], dur.shape[1] + 1))
    for i in range(dur.shape[1]):
        ends[:, i + 1] = ends[:, i] + dur[:, i]
    return ends


# ---- 1. against the exact reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("which", range(5))
def test_against_the_exact_reference(ctx7, ctx9, order, which):
    ctx = _ctx(order, ctx7, ctx9)
    assert ctx.solve_states_max_segments() == SE.MAX_SEG[order]
    M = _seg_counts(order)[which]
    ref = SE.reference(order, M)
    got = _solved(ctx, order, M)
    wp, t, _, _ = SE.case(order, M)
    errs = {}
    for c in SE.COMBOS:
        coef, dur, status = got[c]
        assert (status == 0).all(), (c, status)
        assert np.array_equal(dur, t[:, 1:] - t[:, :-1])
        errs[c] = norm_rel(coef, ref[c])
    print(f"order {order} M {M}: norm_rel vs 60 digits", errs)
    assert max(errs.values()) <= EXACT_BAR, errs


# ---- 2. zero states = the existing solve -------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_zero_states_are_the_rest_to_rest_solve(ctx7, ctx9, order):
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    for M in _seg_counts(order):
        wp, t, _, _ = SE.case(order, M)
        zeros = np.zeros((wp.shape[0], 4, K - 1))
        a = ctx.solve_states(wp, t)
        b = ctx.solve_states(wp, t, zeros, zeros)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        coef, dur, status = ctx.solve_batch(wp, t)
        assert (a[2] == 0).all() and (status == 0).all() and np.array_equal(a[1], dur)
        err = norm_rel(a[0], coef)
        print(f"order {order} M {M}: zero states vs msnap_solve_batch ({ctx.last_kernel()})", err)
        assert err <= FORM_BAR[order], (M, err)


# ---- 3. principle of optimality ----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_a_replan_from_a_state_of_an_optimal_path_stays_on_it(ctx7, ctx9, order):
    ctx = _ctx(order, ctx7, ctx9)
    M, i = 10, 4
    wp, t, _, _ = SE.case(order, M)
    A, durA, st = ctx.solve_states(wp, t)
    assert (st == 0).all()
    ends = _knot_times(durA)
    # from the knot: the remaining waypoints and times
    pos, deriv = ctx.eval_state(A, durA, ends[:, i])
    wp2 = np.concatenate([pos[:, None, :], wp[:, i + 1:]], axis=1)
    t2 = np.concatenate([np.zeros((wp.shape[0], 1)), t[:, i + 1:] - t[:, i:i + 1]], axis=1)
    B, durB, st = ctx.solve_states(wp2, t2, start=deriv)
    assert (st == 0).all()
    err = norm_rel(B, A[:, i:])
    print(f"order {order}: replan from knot {i} vs the path's own segments", err)
    assert err <= FORM_BAR[order], err
    # from the middle of segment i, on one time grid for the batch so that the instants match
    ts = t[0]
    A, durA, st = ctx.solve_states(wp, ts)
    assert (st == 0).all()
    t_r = ts[i] + 0.5 * (ts[i + 1] - ts[i])
    pos, deriv = ctx.eval_state(A, durA, np.full(wp.shape[0], t_r))
    wp2 = np.concatenate([pos[:, None, :], wp[:, i + 1:]], axis=1)
    t2 = np.concatenate([[0.0], ts[i + 1:] - t_r])
    B, durB, st = ctx.solve_states(wp2, t2, start=deriv)
    assert (st == 0).all()
    s = np.linspace(0.0, 0.999 * t2[-1], 32)
    pa = ctx.eval_flat(A, durA, t_r + s)[:, :, [0, 1, 2, 12]]
    pb = ctx.eval_flat(B, durB, s)[:, :, [0, 1, 2, 12]]
    assert np.isfinite(pa).all() and np.isfinite(pb).all()
    gap = np.abs(pa - pb).max()
    print(f"order {order}: replan from the middle of segment {i}: position gap", gap, "of", np.abs(pa).max())
    assert gap <= 1e-10 * np.abs(pa).max()


# ---- 4. the start and the end are honoured ------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_the_given_start_is_honoured(ctx7, ctx9, order):
    """coef[0][a][0] is wp[0][a] bit for bit, and at tq = 0 msnap_eval_state returns each given derivative within
    4 * 2^-52 relative: the budget is the constant 1/q!, one product and the multiply by 3 on the way back (those by 1,
    2 and 4 are exact).  Measured on an MI355X: 0.67 ulp (order 7), 0.66 ulp (order 9)."""
    ctx = _ctx(order, ctx7, ctx9)
    worst, over = 0.0, []
    for M in _seg_counts(order):
        wp, t, start, end = SE.case(order, M)
        for c in SE.COMBOS:
            coef, dur, status = _solved(ctx, order, M)[c]
            s0 = SE.combo_states(c, start, end)[0]
            s0 = np.zeros_like(start) if s0 is None else s0
            assert np.array_equal(coef[:, 0, :, 0], wp[:, 0, :])
            _, d0 = ctx.eval_state(coef, dur, np.zeros(wp.shape[0]))
            rel = np.abs(d0 - s0) / np.where(s0 == 0, 1.0, np.abs(s0))
            worst = max(worst, rel.max())
            if not (rel <= ULP4).all():
                over.append((M, c, rel.max() / 2.0 ** -52))
    print(f"order {order}: start within {worst / 2.0 ** -52:.2f} ulp")
    assert not over, over            # (segments, combination, ulp)


@pytest.mark.parametrize("order", [7, 9])
def test_the_given_end_is_honoured(ctx7, ctx9, order):
    """At the sum of the durations (as msnap_eval_flat accumulates it) msnap_eval_state returns each given end
    derivative within 4 * 2^-52 relative, with the state's scale as the absolute floor: the scale of the Horner sum that
    yields the value, sum_j |d_j| T^j over the coefficients d of the derivative being evaluated on the last segment.
    recover_segment alone misses this (its upper coefficients are cancelling sums with constants of 10^2 .. 10^3 and a
    rounded 1/T: 9 ulp with one segment, 231 / 1322 ulp on the longest paths, where the evaluator's local time is not
    the last duration bit for bit either); the kernel therefore takes one refinement step on the last segment's end
    conditions at the evaluator's own local time (refine_end).  Measured on an MI355X: 1.28 ulp (order 7), 1.40 ulp
    (order 9)."""
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    worst, over = 0.0, []
    for M in _seg_counts(order):
        wp, t, start, end = SE.case(order, M)
        for c in SE.COMBOS:
            coef, dur, status = _solved(ctx, order, M)[c]
            s1 = SE.combo_states(c, start, end)[1]
            s1 = np.zeros_like(end) if s1 is None else s1
            total = _knot_times(dur)[:, -1]
            p1, d1 = ctx.eval_state(coef, dur, total)
            assert np.isfinite(d1).all()
            T = dur[:, -1]
            last = np.abs(coef[:, -1])                                   # [N, 4, NC]
            for q in range(1, K):
                scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
                floor = np.maximum(np.abs(s1[:, :, q - 1]), scale)
                r = np.abs(d1[:, :, q - 1] - s1[:, :, q - 1]) / floor
                worst = max(worst, r.max())
                if not (r <= ULP4).all():
                    over.append((M, c, q, r.max() / 2.0 ** -52))
    print(f"order {order}: end within {worst / 2.0 ** -52:.2f} ulp of its scale")
    assert not over, over            # (segments, combination, derivative, ulp)


# ---- 5. time reversal --------------------------------------------------------------------------------------------
def _reversed_in_time(coef, dur):
    """coefficients of p(T - s) per segment, segments in reverse order, expanded in mpmath and rounded once"""
    N, M, _, NC = coef.shape
    out = np.empty_like(coef)
    for d in range(N):
        for i in range(M):
            T = mp.mpf(float(dur[d, i]))
            for a in range(4):
                c = [mp.mpf(float(v)) for v in coef[d, i, a]]
                for j in range(NC):
                    v = sum((c[k] * mp.binomial(k, j) * T ** (k - j) for k in range(j, NC)), mp.mpf(0))
                    out[d, M - 1 - i, a, j] = float(v * (-1) ** j)
    return out


@pytest.mark.parametrize("order", [7, 9])
def test_time_reversal(ctx7, ctx9, order):
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    M, N = 5, 6
    rng = np.random.default_rng(500 + order)
    dur = rng.integers(32, 129, (N, M)) / 64.0                 # dyadic in [0.5, 2]: both running sums are exact
    t = np.concatenate([np.zeros((N, 1)), np.cumsum(dur, axis=1)], axis=1)
    tr = np.concatenate([np.zeros((N, 1)), np.cumsum(dur[:, ::-1], axis=1)], axis=1)
    wp = np.cumsum(rng.uniform(-2.0, 2.0, (N, M + 1, 4)), axis=1)
    e = rng.uniform(-1.0, 1.0, (N, 4, K - 1)) * np.array(SE.STATE_SCALE[:K - 1])
    sign = np.array([(-1.0) ** q for q in range(1, K)])
    fwd, dur_f, st = ctx.solve_states(wp, t, end=e)
    assert (st == 0).all() and np.array_equal(dur_f, dur)
    bwd, dur_b, st = ctx.solve_states(np.ascontiguousarray(wp[:, ::-1]), tr, start=e * sign)
    assert (st == 0).all() and np.array_equal(dur_b, dur[:, ::-1])
    err = norm_rel(_reversed_in_time(bwd, dur_b), fwd)
    print(f"order {order}: a path against the reversal of the reversed problem", err)
    assert err <= FORM_BAR[order], err


# ---- 6. linearity, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_scaling_by_four_is_exact(ctx7, ctx9, order):
    ctx = _ctx(order, ctx7, ctx9)
    wp, t, start, end = SE.case(order, 10)
    coef, dur, status = _solved(ctx, order, 10)["both"]
    c4, d4, s4 = ctx.solve_states(4.0 * wp, t, 4.0 * start, 4.0 * end)
    assert np.array_equal(c4, 4.0 * coef) and np.array_equal(d4, dur) and np.array_equal(s4, status)


# ---- 7. tiles and independence -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_tiles_position_independence_and_guarded_device_buffers(ctx7, ctx9, order):
    import torch
    from drone_path_planning_python_amd import Context
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    wp, t, start, end = SE.case(order, 3, N=33)
    alone = [ctx.solve_states(wp[d:d + 1], t[d:d + 1], start[d:d + 1], end[d:d + 1]) for d in range(33)]
    dev = torch.device("cuda", 0)
    G, fill = 256, -7.25e300
    with Context(device_id=0, order=order, max_segments=16) as dctx:
        for n in (1, 15, 16, 17, 33):
            coef, dur, status = ctx.solve_states(wp[:n], t[:n], start[:n], end[:n])
            for d in range(n):
                assert np.array_equal(coef[d], alone[d][0][0]) and np.array_equal(dur[d], alone[d][1][0]), (n, d)
                assert status[d] == alone[d][2][0] == 0
            # the device entry, every output between guard words
            ins = [torch.from_numpy(np.ascontiguousarray(x[:n])).to(dev) for x in (wp, t, start, end)]
            gc = torch.full((coef.size + 2 * G,), fill, dtype=torch.float64, device=dev)
            gd = torch.full((dur.size + 2 * G,), fill, dtype=torch.float64, device=dev)
            gs = torch.full((n + 2 * G,), -77, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()              # (the fills above run on torch's stream, the solve on the context's)
            dctx.solve_states_device(n, 3, ins[0], ins[1], False, ins[2], ins[3], gc[G:G + coef.size],
                                     gd[G:G + dur.size], gs[G:G + n])
            dctx.sync()
            gc, gd, gs = gc.cpu().numpy(), gd.cpu().numpy(), gs.cpu().numpy()
            for g, arr, f in ((gc, coef, fill), (gd, dur, fill), (gs, status, -77)):
                assert (g[:G] == f).all() and (g[G + arr.size:] == f).all(), n
                assert np.array_equal(g[G:G + arr.size], arr.reshape(-1)), n
    assert K - 1 == start.shape[2]


# ---- 8. failures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_failed_drones_and_refused_calls(ctx7, ctx9, order):
    from drone_path_planning_python_amd import _lib
    ctx = _ctx(order, ctx7, ctx9)
    wp, t, start, end = SE.case(order, 10)
    clean = _solved(ctx, order, 10)["both"]
    s = start.copy()
    s[5, 2, 1] = np.nan
    coef, dur, status = ctx.solve_states(wp, t, s, end)
    assert status[5] == 3 and np.isnan(coef[5]).all()
    keep = np.arange(wp.shape[0]) != 5
    assert (status[keep] == 0).all() and np.array_equal(coef[keep], clean[0][keep]) and np.array_equal(dur, clean[1])
    e = end.copy()
    e[16, 0, 0] = np.inf
    assert ctx.solve_states(wp, t, start, e)[2].tolist() == [0] * 16 + [3]
    t2 = t.copy()
    t2[3] += 0.1                                   # t[0] = 0.1
    t2[9, 4] = t2[9, 3]                            # not increasing
    coef, dur, status = ctx.solve_states(wp, t2, start, end)
    assert status[3] == 2 and status[9] == 2 and np.isnan(coef[3]).all() and np.isnan(coef[9]).all()
    keep = ~np.isin(np.arange(wp.shape[0]), (3, 9))
    assert (status[keep] == 0).all() and np.array_equal(coef[keep], clean[0][keep])
    # one segment above the cap: refused, nothing written
    M = SE.MAX_SEG[order] + 1
    wpl, tl = np.zeros((2, M + 1, 4)), np.tile(np.arange(M + 1.0), (2, 1))
    coef = np.full((2, M, 4, order + 1), 7.0)
    dur = np.full((2, M), 7.0)
    st = np.full((2,), 7, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = ctx._lib.msnap_solve_states(ctx._h, 2, M, vp(wpl), vp(tl), 0, None, None, vp(coef), vp(dur), vp(st))
    assert rc == -4                                # MSNAP_ESEGMENTS
    assert (coef == 7.0).all() and (dur == 7.0).all() and (st == 7).all()
    with pytest.raises(_lib.MsnapError):
        ctx.solve_states(wpl, tl)
    rc = ctx._lib.msnap_solve_states(ctx._h, 2, 3, None, vp(tl), 0, None, None, vp(coef), vp(dur), vp(st))
    assert rc == -1                                # MSNAP_EINVAL
    assert ctx._lib.msnap_solve_states(ctx._h, 0, 3, None, None, 0, None, None, None, None, None) == 0


# ---- 9. msnap_eval_state -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_eval_state_is_its_restatement_and_eval_flat(ctx7, ctx9, order):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute
    ctx = _ctx(order, ctx7, ctx9)
    N, M = 33, 10
    wp, t, start, end = SE.case(order, M, N=N)
    coef, dur, status = ctx.solve_states(wp, t, start, end)
    assert (status == 0).all()
    ends = _knot_times(dur)
    rng = np.random.default_rng(9)
    tq = rng.uniform(0.0, 1.0, N) * ends[:, -1]
    tq[0] = 0.0
    for k in range(1, M + 1):
        tq[k] = ends[k, k]                       # every knot time, the last one included
    tq[12], tq[13], tq[14] = -1e-12, np.nextafter(ends[13, -1], np.inf), np.nan
    tq[15] = ends[15, -1]
    pos, deriv = ctx.eval_state(coef, dur, tq)
    want_pos, want_deriv = SE.eval_state_np(coef, dur, tq)
    assert np.array_equal(pos, want_pos, equal_nan=True) and np.array_equal(deriv, want_deriv, equal_nan=True)
    assert np.isnan(pos[12:15]).all() and np.isnan(deriv[12:15]).all()
    assert np.isfinite(np.delete(pos, [12, 13, 14], axis=0)).all()
    flat = ctx.eval_flat(coef, dur, tq)          # [N, S = N, 13]: drone d at its own time is flat[d, d]
    own = flat[np.arange(N), np.arange(N)]
    assert np.array_equal(own[:, 0:3], pos[:, :3], equal_nan=True) and np.array_equal(own[:, 12], pos[:, 3], equal_nan=True)
    assert np.array_equal(own[:, 3:6], deriv[:, :3, 0], equal_nan=True)
    assert np.array_equal(own[:, 6:9], deriv[:, :3, 1], equal_nan=True)
    # the device entry gives the same bits
    with Context(device_id=0, order=order, max_segments=16) as dctx:
        comp = DeviceCompute(dctx, torch)
        dev = torch.device("cuda", 0)
        p, dv = comp.eval_state(torch.from_numpy(coef).to(dev), torch.from_numpy(dur).to(dev), torch.from_numpy(tq).to(dev))
        torch.cuda.synchronize()
        assert np.array_equal(p.cpu().numpy(), pos, equal_nan=True) and np.array_equal(dv.cpu().numpy(), deriv, equal_nan=True)


# ---- 10. the checks compose ---------------------------------------------------------------------------------------
def test_the_peaks_see_the_start_speed_and_a_swarm_replans(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute, replan
    for M in _seg_counts(7):
        _, _, start, _ = SE.case(7, M)
        v0 = np.sqrt((start[:, :3, 0] ** 2).sum(axis=1))
        for c in ("start", "both"):
            coef, dur, _ = _solved(ctx7, 7, M)[c]
            peak, t_peak, status = ctx7.dynamic_peaks(coef, dur)
            assert (status == 0).all()
            assert (peak[:, 0] >= v0 * (1 - 1e-9) - 1e-12).all(), (M, c)
    # a 16-drone swarm leaves its paths at 40 % of their duration for three new waypoints
    wp, t, _, _ = SE.case(7, 10, N=16)
    rng = np.random.default_rng(10)
    with Context(device_id=0, order=7, max_segments=16) as dctx:
        comp = DeviceCompute(dctx, torch)
        dev = torch.device("cuda", 0)
        coef, dur, st = comp.solve_states(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        t_r = 0.4 * dur.sum(dim=1)
        wp_new = torch.from_numpy(np.cumsum(rng.uniform(-2.0, 2.0, (16, 3, 4)), axis=1)).to(dev)
        t_new = torch.tensor([1.0, 2.5, 3.5], dtype=torch.float64, device=dev)
        c2, d2, st2, (pos, deriv) = replan(comp, coef, dur, t_r, wp_new, t_new)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and (st2.cpu().numpy() == 0).all()
        want_pos, want_deriv = ctx7.eval_state(coef.cpu().numpy(), dur.cpu().numpy(), t_r.cpu().numpy())
        assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(deriv.cpu().numpy(), want_deriv)
        c2 = c2.cpu().numpy()
        assert np.array_equal(c2[:, 0, :, 0], want_pos) and c2.shape == (16, 3, 4, 8)
        assert np.array_equal(d2.cpu().numpy(), np.tile([1.0, 1.5, 1.0], (16, 1)))
        # a drone whose t_r lies beyond its path comes back failed, the others as before
        t_r2 = t_r.clone()
        t_r2[7] = dur[7].sum() + 1.0
        c3, d3, st3, _ = replan(comp, coef, dur, t_r2, wp_new, t_new)
        torch.cuda.synchronize()
        st3, c3 = st3.cpu().numpy(), c3.cpu().numpy()
        assert st3[7] == 3 and np.isnan(c3[7]).all() and (np.delete(st3, 7) == 0).all()
        assert np.array_equal(np.delete(c3, 7, axis=0), np.delete(c2, 7, axis=0))
