"""Prescribed derivatives at interior waypoints on the GPU (include/msnap.h, "gates"):
msnap_solve_gates against the 60-digit collocation of tests/gates_exact.py, against msnap_solve_states where the two
must agree, and against the properties a gate must have."""
import ctypes
import os
import sys
from math import factorial

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gates_exact as GE  # noqa: E402
import states_exact as SE  # noqa: E402
from conftest import norm_rel  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT_BAR = 1e-10                   # the bar tests/test_states_gpu.py holds msnap_solve_states to
FORM_BAR = {7: 1e-11, 9: 1e-9}      # two solve forms against each other (tests/test_states_gpu.py)
ULP4 = 4 * 2.0 ** -52


def _ctx(order, ctx7, ctx9):
    return ctx7 if order == 7 else ctx9


_SOLVED = {}


def _solved(ctx, order, M):
    """(coef, dur, status) of GE.case(order, M), both end states given: solved once, shared by the tests below"""
    key = (order, M)
    if key not in _SOLVED:
        wp, t, start, end, fix, via = GE.case(order, M)
        _SOLVED[key] = ctx.solve_gates(wp, t, start, end, fix, via)
    return _SOLVED[key]


def _used(fix, K):
    """[N, M-1, K-1] bool: derivative q (index q-1) is prescribed at that knot"""
    return ((fix[:, :, None] >> np.arange(K - 1)) & 1).astype(bool)


# ---- 1. against the exact reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("which", range(4))
def test_against_the_exact_reference(ctx7, ctx9, order, which):
    ctx = _ctx(order, ctx7, ctx9)
    assert ctx.solve_gates_max_segments() == GE.MAX_SEG[order] >= 20
    M = GE.GPU_SEGMENTS[order][which]
    wp, t, _, _, _, _ = GE.case(order, M)
    coef, dur, status = _solved(ctx, order, M)
    assert (status == 0).all(), status
    assert np.array_equal(dur, t[:, 1:] - t[:, :-1])
    err = norm_rel(coef, GE.reference(order, M))
    print(f"order {order} M {M}: norm_rel vs 60 digits", err)
    assert err <= EXACT_BAR, err


# ---- 2. no gates = msnap_solve_states, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_no_gates_is_solve_states_bit_for_bit(ctx7, ctx9, order):
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    for M in (1, 2, 10, GE.MAX_SEG[order]):
        wp, t, start, end = SE.case(order, M)
        want = ctx.solve_states(wp, t, start, end)
        assert (want[2] == 0).all()
        null = ctx.solve_gates(wp, t, start, end)
        zero = ctx.solve_gates(wp, t, start, end, np.zeros((wp.shape[0], M - 1), dtype=np.int32),
                               np.full((wp.shape[0], M - 1, 4, K - 1), np.nan))
        for x, y, z in zip(want, null, zero):
            assert np.array_equal(x, y) and np.array_equal(x, z), M
        # and without end states
        for x, y in zip(ctx.solve_states(wp, t), ctx.solve_gates(wp, t)):
            assert np.array_equal(x, y), M


# ---- 3. a full gate decouples the two sides ------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_a_full_gate_is_the_two_solves_of_its_halves(ctx7, ctx9, order):
    """Times on a dyadic grid (multiples of 1/8 s), so the right half's times t - t[g] are exact.  What differs between
    the two is rounding, and the left half's refine_end: FORM_BAR."""
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    M, N = 10, GE.N_CASE
    rng = np.random.default_rng(2100 + order)
    dur = rng.integers(4, 17, (N, M)) / 8.0
    t = np.concatenate([np.zeros((N, 1)), np.cumsum(dur, axis=1)], axis=1)
    wp, _, start, end = SE.case(order, M)
    v = rng.uniform(-1.0, 1.0, (N, 4, K - 1)) * np.array(SE.STATE_SCALE[:K - 1])
    for g in (1, 5, 9):
        fix = np.zeros((N, M - 1), dtype=np.int32)
        fix[:, g - 1] = 2 ** (K - 1) - 1
        via = np.full((N, M - 1, 4, K - 1), np.nan)
        via[:, g - 1] = v
        coef, d, status = ctx.solve_gates(wp, t, start, end, fix, via)
        left = ctx.solve_states(np.ascontiguousarray(wp[:, :g + 1]), np.ascontiguousarray(t[:, :g + 1]), start, v)
        right = ctx.solve_states(np.ascontiguousarray(wp[:, g:]), t[:, g:] - t[:, g:g + 1], v, end)
        assert (status == 0).all() and (left[2] == 0).all() and (right[2] == 0).all()
        assert np.array_equal(d, np.concatenate([left[1], right[1]], axis=1)) and np.array_equal(d, dur)
        err = norm_rel(coef, np.concatenate([left[0], right[0]], axis=1))
        print(f"order {order}: full gate at knot {g} vs the two halves", err)
        assert err <= FORM_BAR[order], (g, err)


# ---- 4. the gate is honoured -------------------------------------------------------------------------------------
def _worst_jump(coef, dur, K, which):
    """The largest jump of a derivative 1..K-1 across an interior knot, over the (drone, knot, derivative) selected by
    `which` [N, M-1, K-1], exact (mpmath) on the float64 coefficients, in units of the scale of the Horner sum that
    yields the left-hand value: sum_j |d_j| T^j over the coefficients d of that derivative on the arriving segment."""
    worst = mp.mpf(0)
    N, M = dur.shape
    for d in range(N):
        for i in range(1, M):
            T = dur[d, i - 1]
            for q in range(1, K):
                if not which[d, i - 1, q - 1]:
                    continue
                for a in range(4):
                    left = SE.eval_state_mp(coef[d, i - 1, a], T, q)
                    right = SE.eval_state_mp(coef[d, i, a], 0.0, q)
                    scale = sum(SE.falling(j, q) * abs(coef[d, i - 1, a, j]) * T ** (j - q) for j in range(q, 2 * K))
                    worst = max(worst, abs(left - right) / mp.mpf(float(scale)))
    return float(worst)


@pytest.mark.parametrize("order", [7, 9])
def test_the_gate_is_honoured_on_both_sides(ctx7, ctx9, order):
    """Leaving segment: coef[i][a][q] * q! is the prescribed value within 4 * 2^-52 relative -- row c of G is zero and
    z[c] = g[c] exactly, so u_i[c] is the value itself; the budget is the constant 1/q!, one product and the multiply on
    the way back.  Arriving segment: it meets the value as every interior knot's continuity is met -- both come out of
    recover_segment from the same u_i -- so the jump of derivatives 1..K-1 across the gated knots may be at most twice
    the worst jump across the interior knots of msnap_solve_states' output on the same waypoints, times and end states.
    Measured on an MI355X, in units of 2^-52 of the Horner sum's scale, M = 10: order 7 gated 228 against
    4688 ungated, order 9 gated 17 736 against 152 665 (the upper coefficients of recover_segment are cancelling sums
    with constants of 10^2 .. 10^3: tests/test_states_gpu.py, test_the_given_end_is_honoured); the prescribed values
    on the leaving segments within 0.66 ulp at both orders."""
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    M = 10
    wp, t, start, end, fix, via = GE.case(order, M)
    coef, dur, status = _solved(ctx, order, M)
    assert (status == 0).all()
    used = _used(fix, K)
    assert used.any()
    worst = 0.0
    for q in range(1, K):
        sel = used[:, :, q - 1]                                          # [N, M-1]
        got = coef[:, 1:, :, q][sel] * float(factorial(q))               # [n, 4]
        want = via[:, :, :, q - 1][sel]
        assert np.isfinite(want).all()
        rel = np.abs(got - want) / np.abs(want)
        worst = max(worst, rel.max())
    print(f"order {order}: leaving segments within {worst / 2.0 ** -52:.2f} ulp of the prescribed values")
    assert worst <= ULP4, worst / 2.0 ** -52
    gated = _worst_jump(coef, dur, K, used | used.any(axis=2, keepdims=True))      # every derivative at a gated knot
    plain = ctx.solve_states(wp, t, start, end)
    ungated = _worst_jump(plain[0], plain[1], K, np.ones_like(used))
    print(f"order {order}: worst jump across gated knots {gated / 2.0 ** -52:.2f} ulp of scale, across the interior "
          f"knots of solve_states {ungated / 2.0 ** -52:.2f}")
    assert gated <= 2.0 * ungated, (gated, ungated)


# ---- 5. tiles and independence -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_tiles_position_independence_and_guarded_device_buffers(ctx7, ctx9, order):
    import torch
    from drone_path_planning_python_amd import Context
    ctx = _ctx(order, ctx7, ctx9)
    M = 3
    wp, t, start, end, fix, via = GE.case(order, M, N=33)
    alone = [ctx.solve_gates(wp[d:d + 1], t[d:d + 1], start[d:d + 1], end[d:d + 1], fix[d:d + 1], via[d:d + 1])
             for d in range(33)]
    # a drone moved within the batch: the batch reversed
    rev = ctx.solve_gates(*(np.ascontiguousarray(x[::-1]) for x in (wp, t, start, end, fix, via)))
    dev = torch.device("cuda", 0)
    G, fill = 256, -7.25e300
    with Context(device_id=0, order=order, max_segments=16) as dctx:
        for n in (1, 16, 17, 33):
            coef, dur, status = ctx.solve_gates(wp[:n], t[:n], start[:n], end[:n], fix[:n], via[:n])
            for d in range(n):
                assert np.array_equal(coef[d], alone[d][0][0]) and np.array_equal(dur[d], alone[d][1][0]), (n, d)
                assert status[d] == alone[d][2][0] == 0
                assert np.array_equal(coef[d], rev[0][32 - d]) and rev[2][32 - d] == 0
            # the device entry, every output between guard words
            ins = [torch.from_numpy(np.ascontiguousarray(x[:n])).to(dev) for x in (wp, t, start, end, fix, via)]
            gc = torch.full((coef.size + 2 * G,), fill, dtype=torch.float64, device=dev)
            gd = torch.full((dur.size + 2 * G,), fill, dtype=torch.float64, device=dev)
            gs = torch.full((n + 2 * G,), -77, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()              # (the fills above run on torch's stream, the solve on the context's)
            dctx.solve_gates_device(n, M, ins[0], ins[1], False, ins[2], ins[3], ins[4], ins[5], gc[G:G + coef.size],
                                    gd[G:G + dur.size], gs[G:G + n])
            dctx.sync()
            gc, gd, gs = gc.cpu().numpy(), gd.cpu().numpy(), gs.cpu().numpy()
            for g, arr, f in ((gc, coef, fill), (gd, dur, fill), (gs, status, -77)):
                assert (g[:G] == f).all() and (g[G + arr.size:] == f).all(), n
                assert np.array_equal(g[G:G + arr.size], arr.reshape(-1)), n


# ---- 6. failures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_failed_drones_and_refused_calls(ctx7, ctx9, order):
    from drone_path_planning_python_amd import _lib
    ctx = _ctx(order, ctx7, ctx9)
    K = (order + 1) // 2
    M = 10
    wp, t, start, end, fix, via = GE.case(order, M)
    clean = _solved(ctx, order, M)
    N = wp.shape[0]
    used = _used(fix, K)

    def one_failed(f, v, d):
        coef, dur, status = ctx.solve_gates(wp, t, start, end, f, v)
        keep = np.arange(N) != d
        assert status[d] == 3 and np.isnan(coef[d]).all(), status
        assert (status[keep] == 0).all() and np.array_equal(coef[keep], clean[0][keep]) and np.array_equal(dur, clean[1])

    # a NaN / Inf under a set bit fails that drone only
    d, i, q = next((d, i, q) for d in range(4, N) for i in range(M - 1) for q in range(K - 1) if used[d, i, q])
    for bad in (np.nan, np.inf):
        v = via.copy()
        v[d, i, 2, q] = bad
        one_failed(fix, v, d)
    # anything under a clear bit does not: NaN there already; Inf and numbers change nothing
    v = via.copy()
    v[np.isnan(via)] = np.inf
    v[0, 0] = 1e300                                    # (drone 0, knot 1: the empty mask)
    assert fix[0, 0] == 0
    for x, y in zip(ctx.solve_gates(wp, t, start, end, fix, v), clean):
        assert np.array_equal(x, y)
    # a mask outside 0 .. 2^(K-1) - 1
    for bad in (2 ** (K - 1), -1):
        f = fix.copy()
        f[16, M - 2] = bad
        one_failed(f, via, 16)
    # one segment above the cap: refused, nothing written
    Mc = GE.MAX_SEG[order] + 1
    wpl, tl = np.zeros((2, Mc + 1, 4)), np.tile(np.arange(Mc + 1.0), (2, 1))
    coef = np.full((2, Mc, 4, order + 1), 7.0)
    dur = np.full((2, Mc), 7.0)
    st = np.full((2,), 7, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = ctx._lib.msnap_solve_gates(ctx._h, 2, Mc, vp(wpl), vp(tl), 0, None, None, None, None, vp(coef), vp(dur), vp(st))
    assert rc == -4                                # MSNAP_ESEGMENTS
    assert (coef == 7.0).all() and (dur == 7.0).all() and (st == 7).all()
    with pytest.raises(_lib.MsnapError):
        ctx.solve_gates(wpl, tl)
    # a mask without values
    f2 = np.zeros((2, 2), dtype=np.int32)
    for entry in (ctx._lib.msnap_solve_gates, ctx._lib.msnap_solve_gates_device):
        rc = entry(ctx._h, 2, 3, vp(wpl), vp(tl), 0, None, None, vp(f2), None, vp(coef), vp(dur), vp(st))
        assert rc == -1                            # MSNAP_EINVAL
    assert (coef == 7.0).all() and (dur == 7.0).all() and (st == 7).all()
    assert ctx._lib.msnap_solve_gates(ctx._h, 0, 3, None, None, 0, None, None, None, None, None, None, None) == 0


# ---- 7. a swarm replans through a gate ----------------------------------------------------------------------------
def test_a_swarm_replans_through_a_gate(ctx7):
    """The bar of test 4, on the replan's own problem: the arriving segment meets the gate velocity within twice the
    worst jump across the interior knots of the same replan without gates (exact, on the float64 coefficients);
    msnap_eval_state adds its own rounding, 4 * 2^-52 of the Horner sum's scale (tests/test_states_cpu.py)."""
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute, replan
    n = 8
    wp, t, _, _ = SE.case(7, 10, N=n)
    rng = np.random.default_rng(2107)
    gate_v = np.zeros((n, 4))
    gate_v[:, :3] = rng.uniform(1.0, 2.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))      # 1.7 .. 3.5 m/s through the gate
    with Context(device_id=0, order=7, max_segments=16) as dctx:
        comp = DeviceCompute(dctx, torch)
        dev = torch.device("cuda", 0)
        coef, dur, st = comp.solve_states(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        t_r = 0.4 * dur.sum(dim=1)
        wp_new = torch.from_numpy(np.cumsum(rng.uniform(-2.0, 2.0, (n, 3, 4)), axis=1)).to(dev)
        t_new = torch.tensor([1.0, 2.5, 3.5], dtype=torch.float64, device=dev)
        fix = torch.tensor([[1, 0]] * n, dtype=torch.int32, device=dev)                  # velocity at the first new waypoint
        via = torch.full((n, 2, 4, 3), float("nan"), dtype=torch.float64, device=dev)
        via[:, 0, :, 0] = torch.from_numpy(gate_v).to(dev)
        with pytest.raises(ValueError):
            replan(comp, coef, dur, t_r, wp_new, t_new, optimize={}, gates=(fix, via))
        c0, d0, st0, _ = replan(comp, coef, dur, t_r, wp_new, t_new)
        c0, d0 = c0.clone(), d0.clone()
        c2, d2, st2, (pos, deriv) = replan(comp, coef, dur, t_r, wp_new, t_new, gates=(fix, via))
        _, s_gate = comp.eval_state(c2, d2, torch.full((n,), 1.0, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and (st0.cpu().numpy() == 0).all() and (st2.cpu().numpy() == 0).all()
        c0, d0, c2, d2, s_gate = (x.cpu().numpy() for x in (c0, d0, c2, d2, s_gate))
    assert np.array_equal(d2, np.tile([1.0, 1.5, 1.0], (n, 1))) and np.array_equal(c2[:, 0, :, 0], pos.cpu().numpy())
    # leaving segment: the value itself
    assert (np.abs(c2[:, 1, :, 1] - gate_v) <= ULP4 * np.abs(gate_v)).all()
    # arriving segment, exact and through the evaluator
    ungated = _worst_jump(c0, d0, 4, np.ones((n, 2, 3), dtype=bool))
    for d in range(n):
        for a in range(4):
            scale = sum(j * abs(c2[d, 0, a, j]) * 1.0 ** (j - 1) for j in range(1, 8))
            exact = abs(SE.eval_state_mp(c2[d, 0, a], 1.0, 1) - mp.mpf(float(gate_v[d, a]))) / mp.mpf(float(scale))
            assert exact <= 2.0 * ungated, (d, a, float(exact), ungated)
            assert abs(s_gate[d, a, 0] - gate_v[d, a]) <= (2.0 * ungated + ULP4) * scale, (d, a)
    peak, t_peak, status = ctx7.dynamic_peaks(c2, d2)
    speed = np.sqrt((gate_v[:, :3] ** 2).sum(axis=1))
    assert (status == 0).all() and (peak[:, 0] >= speed * (1 - 1e-9)).all(), (peak[:, 0], speed)
