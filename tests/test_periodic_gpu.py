"""Closed-loop paths on the GPU (include/msnap.h, "closed-loop paths"): msnap_solve_periodic against
the 60-digit reference of tests/periodic_exact.py, with msnap_solve_states at the reference's seam state as the
yardstick, against the properties a periodic minimum must have, and through the wrappers."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_exact as PE  # noqa: E402
import states_exact as SE  # noqa: E402
from conftest import norm_rel  # noqa: E402

pytestmark = pytest.mark.gpu

ABS_BAR = {7: 1e-10, 9: 1e-9}       # EXACT_BAR and the order-9 figure of FORM_BAR in tests/test_states_gpu.py
FLOOR = 1e-13
ULP4 = 4 * 2.0 ** -52


def _ctx(order, ctx7, ctx9):
    return ctx7 if order == 7 else ctx9


def _offset_counts(order):
    return list(PE.SEG_COUNTS) + [PE.MAX_SEG[order]]


_SOLVED, _BAR = {}, {}


def _solved(ctx, order, M, kind="offset"):
    """(coef, dur, status) of case(order, M, kind): solved once, shared by the tests below"""
    key = (order, M, kind)
    if key not in _SOLVED:
        _SOLVED[key] = ctx.solve_periodic(*PE.case(order, M, kind=kind))
    return _SOLVED[key]


def _bar(ctx, order, M, kind="offset"):
    """(bar, yardstick): the yardstick is msnap_solve_states on the same inputs, given the reference's exact seam state
    as start and end, scored against the reference by the same metric.  One more block solve and a second recurrence of
    the same length and conditioning should roughly double the error: the bar is 4 x the yardstick, never below 1e-13."""
    key = (order, M, kind)
    if key not in _BAR:
        wp, t = PE.case(order, M, kind=kind)
        ref, seam = PE.reference(order, M, kind)
        coef, _, status = ctx.solve_states(wp, t, seam, seam)
        assert (status == 0).all()
        yard = norm_rel(coef, ref)
        _BAR[key] = (max(4.0 * yard, FLOOR), yard)
    return _BAR[key]


def _knot_times(dur):
    """[N, M+1] running sums as msnap_eval_flat accumulates them"""
    ends = np.zeros((dur.shape[0], dur.shape[1] + 1))
    for i in range(dur.shape[1]):
        ends[:, i + 1] = ends[:, i] + dur[:, i]
    return ends


# ---- 1. against 60 digits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("which", range(6))
def test_against_the_exact_reference(ctx7, ctx9, order, which):
    """Measured on an MI355X (norm_rel against 60 digits; in brackets the yardstick, msnap_solve_states at the exact seam
    state): order 7 at M = 2 / 3 / 10 / 27 2.7e-13 / 3.1e-13 / 2.4e-13 / 2.7e-13 (2.4e-13 / 5.8e-13 / 3.9e-13 / 3.1e-13),
    order 9 at M = 2 / 3 / 10 / 18 1.6e-11 / 4.5e-12 / 2.5e-11 / 1.5e-11 (1.0e-11 / 1.5e-11 / 5.5e-11 / 1.4e-11); shared
    times and the closed case at M = 10: 2.0e-13, 2.0e-13 (order 7), 6.5e-12, 1.3e-11 (order 9).  DESIGN.md §5 K15 has the
    table, and the figures of the kernel without its refinement step (order 9, M = 2: 4.0e-11)."""
    ctx = _ctx(order, ctx7, ctx9)
    assert ctx.solve_periodic_max_segments() == PE.MAX_SEG[order]
    M, kind = PE.gpu_cases(order)[which]
    wp, t = PE.case(order, M, kind=kind)
    ref, _ = PE.reference(order, M, kind)
    coef, dur, status = _solved(ctx, order, M, kind)
    assert (status == 0).all(), status
    assert np.array_equal(dur, np.broadcast_to(np.diff(t), dur.shape))
    err = norm_rel(coef, ref)
    bar, yard = _bar(ctx, order, M, kind)
    print(f"order {order} M {M} {kind}: norm_rel vs 60 digits {err:.3e}; msnap_solve_states at the exact seam state "
          f"{yard:.3e}; bar {bar:.3e}")
    assert err <= bar, (err, yard)
    assert err <= ABS_BAR[order], err


# ---- 2. the seam as the evaluator sees it ------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_the_seam_through_the_evaluator(ctx7, ctx9, order):
    """msnap_eval_state at the sum of the durations against itself at 0: derivatives 1..K-1 within 4 * 2^-52 of
    max(|value|, sum_j |d_j| T^j), d the coefficients of the derivative being evaluated on the last segment; the
    position there against wp[M] within the same bound; coef[i][a][0] is wp[i][a] bit for bit.  Measured on an MI355X:
    1.07 ulp (order 7), 1.10 ulp (order 9)."""
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    worst, over = 0.0, []
    for M, kind in [(M, "offset") for M in _offset_counts(order)] + [(10, "closed")]:
        wp, t = PE.case(order, M, kind=kind)
        if kind == "closed":
            assert np.array_equal(wp[:, M, :3], wp[:, 0, :3]) and np.array_equal(wp[:, M, 3], wp[:, 0, 3] + 2 * np.pi)
        else:
            assert (wp[:, M] != wp[:, 0]).all()              # a nonzero lap offset on every axis
        coef, dur, status = _solved(ctx, order, M, kind)
        assert (status == 0).all()
        assert np.array_equal(coef[:, :, :, 0], wp[:, :M, :])
        p0, d0 = ctx.eval_state(coef, dur, np.zeros(wp.shape[0]))
        p1, d1 = ctx.eval_state(coef, dur, _knot_times(dur)[:, -1])
        assert np.isfinite(d0).all() and np.isfinite(d1).all() and np.array_equal(p0, wp[:, 0])
        T = dur[:, -1]
        last = np.abs(coef[:, -1])                                       # [N, 4, NC]
        for q in range(K):
            scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
            want = wp[:, M] if q == 0 else d0[:, :, q - 1]
            got = p1 if q == 0 else d1[:, :, q - 1]
            r = np.abs(got - want) / np.maximum(np.abs(want), scale)
            worst = max(worst, r.max())
            if not (r <= ULP4).all():
                over.append((M, kind, q, r.max() / 2.0 ** -52))
    print(f"order {order}: seam within {worst / 2.0 ** -52:.2f} ulp of its scale")
    assert not over, over            # (segments, case, derivative, ulp)


# ---- 3. consistency with the boundary-state solve ----------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_the_boundary_state_solve_at_the_seam_state_reproduces_the_loop(ctx7, ctx9, order):
    ctx = _ctx(order, ctx7, ctx9)
    for M in _offset_counts(order):
        wp, t = PE.case(order, M)
        coef, dur, _ = _solved(ctx, order, M)
        _, d0 = ctx.eval_state(coef, dur, np.zeros(wp.shape[0]))
        c2, _, st = ctx.solve_states(wp, t, d0, d0)
        assert (st == 0).all()
        err = norm_rel(c2, coef)
        bar, _ = _bar(ctx, order, M)
        print(f"order {order} M {M}: msnap_solve_states at the loop's own seam state vs the loop {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (M, err)


# ---- 4. optimality ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_any_other_seam_state_costs_more(ctx7, ctx9, order):
    """In exact arithmetic a perturbation of 0.01 per entry already raises the cost by at least 5e-5 of its value on
    these distributions; rounding in msnap_snap_cost cannot decide a comparison at +-0.1."""
    ctx = _ctx(order, ctx7, ctx9)
    for M in _offset_counts(order):
        wp, t = PE.case(order, M)
        coef, dur, _ = _solved(ctx, order, M)
        J = ctx.snap_cost(coef, dur)
        _, d0 = ctx.eval_state(coef, dur, np.zeros(wp.shape[0]))
        rng = np.random.default_rng(4000 + 100 * order + M)
        for k in range(3):
            s = d0 + rng.uniform(-0.1, 0.1, d0.shape)
            c2, d2, st = ctx.solve_states(wp, t, s, s)
            assert (st == 0).all()
            J2 = ctx.snap_cost(c2, d2)
            assert (J2 > J).all(), (M, k, ((J2 - J) / J).min())


# ---- 5. rotation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_starting_the_loop_at_another_knot_permutes_the_segments(ctx7, ctx9, order):
    ctx = _ctx(order, ctx7, ctx9)
    for M in _offset_counts(order):
        wp, t = PE.case(order, M)
        coef, dur, _ = _solved(ctx, order, M)
        lap = wp[:, M] - wp[:, 0]
        bar, _ = _bar(ctx, order, M)
        for j in sorted({1, M - 1}):
            wp2, t2 = PE.rotate(wp, t, j)
            c2, d2, st = ctx.solve_periodic(wp2, t2)
            assert (st == 0).all()
            want = np.concatenate([coef[:, j:], coef[:, :j]], axis=1).copy()
            want[:, M - j:, :, 0] += lap[:, None, :]         # the segments after the seam carry the lap offset in c[0]
            assert np.array_equal(c2[:, :, :, 0], wp2[:, :M])
            err = norm_rel(c2, want)
            print(f"order {order} M {M}: started at knot {j} vs the loop's own segments {err:.3e} (bar {bar:.3e})")
            assert err <= bar, (M, j, err)


# ---- 6. batch independence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_tiles_position_independence_and_guarded_device_buffers(ctx7, ctx9, order):
    import torch
    from drone_path_planning_python_amd import Context
    ctx = _ctx(order, ctx7, ctx9)
    wp, t = PE.case(order, 3, N=33)
    alone = [ctx.solve_periodic(wp[d:d + 1], t[d:d + 1]) for d in range(33)]
    dev = torch.device("cuda", 0)
    G, fill = 256, -7.25e300
    with Context(device_id=0, order=order, max_segments=16) as dctx:
        for n in (1, 16, 17, 33):
            coef, dur, status = ctx.solve_periodic(wp[:n], t[:n])
            for d in range(n):
                assert np.array_equal(coef[d], alone[d][0][0]) and np.array_equal(dur[d], alone[d][1][0]), (n, d)
                assert status[d] == alone[d][2][0] == 0
            # the device entry, every output between guard words
            ins = [torch.from_numpy(np.ascontiguousarray(x[:n])).to(dev) for x in (wp, t)]
            gc = torch.full((coef.size + 2 * G,), fill, dtype=torch.float64, device=dev)
            gd = torch.full((dur.size + 2 * G,), fill, dtype=torch.float64, device=dev)
            gs = torch.full((n + 2 * G,), -77, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()              # (the fills above run on torch's stream, the solve on the context's)
            dctx.solve_periodic_device(n, 3, ins[0], ins[1], False, gc[G:G + coef.size], gd[G:G + dur.size],
                                       gs[G:G + n])
            dctx.sync()
            gc, gd, gs = gc.cpu().numpy(), gd.cpu().numpy(), gs.cpu().numpy()
            for g, arr, f in ((gc, coef, fill), (gd, dur, fill), (gs, status, -77)):
                assert (g[:G] == f).all() and (g[G + arr.size:] == f).all(), n
                assert np.array_equal(g[G:G + arr.size], arr.reshape(-1)), n


# ---- 7. status and arguments ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_failed_drones_and_refused_calls(ctx7, ctx9, order):
    from drone_path_planning_python_amd import _lib
    ctx = _ctx(order, ctx7, ctx9)
    M = 10
    wp, t = PE.case(order, M, N=16)                    # one full tile
    solo = [ctx.solve_periodic(wp[d:d + 1], t[d:d + 1]) for d in range(16)]

    def check(wp_, t_, d_bad, code):
        coef, dur, status = ctx.solve_periodic(wp_, t_)
        assert status[d_bad] == code and np.isnan(coef[d_bad]).all(), (d_bad, code, status)
        for d in range(16):
            if d != d_bad:
                assert status[d] == 0 and np.array_equal(coef[d], solo[d][0][0]), (d_bad, d)
        assert np.array_equal(dur, np.diff(t_), equal_nan=True)          # written for every drone

    w2 = wp.copy()
    w2[5, M, 2] = np.nan                               # the last waypoint is read too
    check(w2, t, 5, 3)
    t2 = t.copy()
    t2[11, 4] = np.nan
    check(wp, t2, 11, 3)
    t2 = t.copy()
    t2[9, 4] = t2[9, 3]
    check(wp, t2, 9, 2)
    t2 = t.copy()
    t2[3] += 0.1                                       # t[0] = 0.1
    check(wp, t2, 3, 2)
    # one segment, and one above the cap: refused, nothing written
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    for Mx in (1, PE.MAX_SEG[order] + 1):
        wpl, tl = np.zeros((2, Mx + 1, 4)), np.tile(np.arange(Mx + 1.0), (2, 1))
        coef = np.full((2, Mx, 4, order + 1), 7.0)
        dur = np.full((2, Mx), 7.0)
        st = np.full((2,), 7, dtype=np.int32)
        rc = ctx._lib.msnap_solve_periodic(ctx._h, 2, Mx, vp(wpl), vp(tl), 0, vp(coef), vp(dur), vp(st))
        assert rc == -4                                # MSNAP_ESEGMENTS
        assert (coef == 7.0).all() and (dur == 7.0).all() and (st == 7).all()
        with pytest.raises(_lib.MsnapError):
            ctx.solve_periodic(wpl, tl)
    rc = ctx._lib.msnap_solve_periodic(ctx._h, 2, 3, None, vp(tl), 0, vp(coef), vp(dur), vp(st))
    assert rc == -1                                    # MSNAP_EINVAL
    assert ctx._lib.msnap_solve_periodic(ctx._h, 0, 3, None, None, 0, None, None, None) == 0


# ---- 8. wrappers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_the_torch_wrapper_and_join_loop(ctx7, ctx9, order):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute, join_loop
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    dev = torch.device("cuda", 0)
    with Context(device_id=0, order=order, max_segments=16) as dctx:
        comp = DeviceCompute(dctx, torch)
        for kind in ("offset", "shared"):
            wp, t = PE.case(order, 10, kind=kind)
            coef, dur, status = _solved(ctx, order, 10, kind)
            c, d, s = comp.solve_periodic(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
            torch.cuda.synchronize()
            assert np.array_equal(c.cpu().numpy(), coef) and np.array_equal(d.cpu().numpy(), dur)
            assert np.array_equal(s.cpu().numpy(), status)
        # eight drones leave rest-to-rest paths at 40 % of the flight and join eight loops through two waypoints
        n = 8
        wpa, ta, _, _ = SE.case(order, 10, N=n)
        wpl, tl = PE.case(order, 6, N=n, kind="closed")
        pc, pd, st = comp.solve_states(torch.from_numpy(wpa).to(dev), torch.from_numpy(ta).to(dev))
        lc, ld, lst = comp.solve_periodic(torch.from_numpy(wpl).to(dev), torch.from_numpy(tl).to(dev))
        t_r = 0.4 * pd.sum(dim=1)
        rng = np.random.default_rng(80 + order)
        via = torch.from_numpy(np.cumsum(rng.uniform(-2.0, 2.0, (n, 2, 4)), axis=1)).to(dev)
        t_via = torch.tensor([1.0, 2.5, 3.5], dtype=torch.float64, device=dev)
        jc, jd, jst, (pos, deriv) = join_loop(comp, pc, pd, t_r, lc, ld, via, t_via)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and (lst.cpu().numpy() == 0).all() and (jst.cpu().numpy() == 0).all()
        jc, jd = jc.cpu().numpy(), jd.cpu().numpy()
        assert jc.shape == (n, 3, 4, 2 * K) and np.array_equal(jd, np.tile([1.0, 1.5, 1.0], (n, 1)))
        # at its start the joining path has the old path's state at t_r ...
        want_pos, want_deriv = ctx.eval_state(pc.cpu().numpy(), pd.cpu().numpy(), t_r.cpu().numpy())
        assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(deriv.cpu().numpy(), want_deriv)
        p0, d0 = ctx.eval_state(jc, jd, np.zeros(n))
        assert np.array_equal(p0, want_pos)
        assert (np.abs(d0 - want_deriv) <= ULP4 * np.abs(want_deriv)).all()
        # ... and at its end the loop's state at 0, within the bound the header states for an end state
        lp, ldv = ctx.eval_state(lc.cpu().numpy(), ld.cpu().numpy(), np.zeros(n))
        p1, d1 = ctx.eval_state(jc, jd, _knot_times(jd)[:, -1])
        T = jd[:, -1]
        last = np.abs(jc[:, -1])
        for q in range(K):
            scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
            want = lp if q == 0 else ldv[:, :, q - 1]
            got = p1 if q == 0 else d1[:, :, q - 1]
            r = np.abs(got - want) / np.maximum(np.abs(want), scale)
            assert (r <= ULP4).all(), (q, r.max() / 2.0 ** -52)
