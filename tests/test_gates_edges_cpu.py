"""The edges of msnap_solve_gates on the CPU (include/msnap.h, "gates"): every builder of
tests/gates_cases.py has the structure tests/test_gates_edges_gpu.py relies on, and the NumPy restatement of the masked
sweep (tests/gates_ref.py) reaches the 60-digit reference on it at the bar the kernel is then held to -- the bar is
shown reachable in float64 before the kernel meets it.  Measured figures stand in the docstrings; every test prints
its own."""
import os
import sys
from math import factorial

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gates_cases as GC  # noqa: E402
import gates_exact as GE  # noqa: E402
import gates_ref as GR  # noqa: E402
import states_exact as SE  # noqa: E402
from conftest import norm_rel  # noqa: E402

EXACT_BAR = 1e-10                   # the bar tests/test_gates_gpu.py holds msnap_solve_gates to
ORDERS = [7, 9]


def _restated(case, K):
    wp, t, start, end, fix, via = case
    if fix is None:
        fix = np.zeros((wp.shape[0], wp.shape[1] - 2), dtype=np.int32)
        via = np.full(fix.shape + (4, K - 1), np.nan)
    return GR.solve_batch(wp, t, start, end, fix, via, K)


def _values_sit_under_the_bits(fix, via, K):
    used = np.broadcast_to(GC.used_bits(fix, K)[:, :, None, :], via.shape)
    assert np.isfinite(via[used]).all() and np.isnan(via[~used]).all()
    assert (np.nan_to_num(np.abs(via)) <= np.array(SE.STATE_SCALE[:K - 1])).all()


# ---- A. sparse tiles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_sparse_tiles(order):
    """Restatement against 60 digits: 6.6e-13 at order 7, 4.7e-12 at order 9."""
    K = GC.half(order)
    case = wp, t, start, end, fix, via = GC.sparse(order)
    assert wp.shape == (33, 7, 4) and t.shape == (33, 7) and fix.shape == (33, 5) and fix.dtype == np.int32
    gating = [np.flatnonzero(fix[:16, i]).tolist() for i in range(5)]       # tile 0, knots 1 .. 5
    assert gating == [[3], [], [15], [], [0, 8]], gating
    assert fix[3, 0] == 2 ** (K - 1) - 1 and fix[15, 2] == 1
    assert 0 < fix[0, 4] != fix[8, 4] > 0
    assert (fix[16:32] == 0).all() and np.isnan(via[16:32]).all()          # tile 1: nothing, but fix is not NULL
    assert (fix[32] != 0).tolist() == [False, True, False, True, False]    # tile 2: knots 2 and 4
    # within tile 0 a plain step is followed by a masked one and the other way round, twice each
    any_gate = (fix[:16] != 0).any(axis=0).tolist()
    assert any_gate == [True, False, True, False, True]
    assert (fix == 0).all(axis=1).sum() == 33 - 5
    _values_sit_under_the_bits(fix, via, K)
    err = norm_rel(_restated(case, K), GC.exact(("sparse", order), case))
    print(f"order {order}: sparse tiles, restatement vs 60 digits", err)
    assert err <= EXACT_BAR, err


# ---- B. shared times ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_shared_times(order):
    """Restatement against 60 digits: 6.6e-13 at order 7, 1.5e-12 at order 9."""
    K = GC.half(order)
    case = wp, t, start, end, fix, via = GC.shared(order)
    assert t.shape == (7,) and t[0] == 0.0 and (np.diff(t) > 0).all()
    assert np.array_equal(fix, GC.sparse_masks(order)) and np.array_equal(via, GC.sparse(order)[5], equal_nan=True)
    tiled = (wp, np.tile(t, (33, 1)), start, end, fix, via)
    assert np.array_equal(_restated(case, K), _restated(tiled, K))
    err = norm_rel(_restated(case, K), GC.exact(("shared", order), case))
    print(f"order {order}: shared times, restatement vs 60 digits", err)
    assert err <= EXACT_BAR, err


# ---- C. rest ends ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_rest_ends(order):
    """Restatement against 60 digits, (rest, rest) / (given, rest) / (rest, given): 1.3e-13, 1.5e-13, 1.2e-13 at order
    7; 7.7e-13, 5.3e-13, 8.5e-13 at order 9."""
    K = GC.half(order)
    errs = []
    for combo in GC.REST_COMBOS:
        case = wp, t, start, end, fix, via = GC.rest(order, combo)
        assert (start is not None, end is not None) == combo
        assert np.array_equal(fix, GE.masks(order, GC.M_EDGE)) and (fix != 0).any(axis=0).all()
        zero = np.zeros((wp.shape[0], 4, K - 1))
        explicit = (wp, t, zero if start is None else start, zero if end is None else end, fix, via)
        assert np.array_equal(_restated(case, K), _restated(explicit, K))
        errs.append(norm_rel(_restated(case, K), GC.exact(("rest", order, combo), case)))
    print(f"order {order}: rest ends {GC.REST_COMBOS}, restatement vs 60 digits", errs)
    assert max(errs) <= EXACT_BAR, errs


# ---- D. prescribed zeros --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_prescribed_zeros(order):
    """Restatement against 60 digits: 8.4e-14 at order 7, 7.9e-13 at order 9 (the reference does not see a zero's sign);
    its leaving segments hold the zeros exactly."""
    K = GC.half(order)
    ref = None
    for zero in (0.0, -0.0):
        case = wp, t, start, end, fix, via = GC.zeros(order, zero)
        used = GC.used_bits(fix, K)
        assert used.any(axis=(0, 1)).all()                                  # every derivative is prescribed somewhere
        at = np.broadcast_to(used[:, :, None, :], via.shape)
        assert (via[at] == 0.0).all() and (np.signbit(via[at]) == np.signbit(zero)).all() and np.isnan(via[~at]).all()
        if ref is None:
            ref = GC.exact(("zeros", order), case)
        coef = _restated(case, K)
        for q in range(1, K):
            assert (coef[:, 1:, :, q][used[:, :, q - 1]] == 0.0).all()
        err = norm_rel(coef, ref)
        print(f"order {order}: prescribed {zero!r}, restatement vs 60 digits", err)
        assert err <= EXACT_BAR, err


# ---- E. every knot fully gated --------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M", GC.FULL_SEGMENTS)
def test_every_knot_fully_gated(order, M):
    """Each segment is the Hermite interpolant of its two knots' states.  Against the 60-digit interpolant (a 2K x 2K
    solve per segment, nothing of gates_exact): the collocation of gates_exact agrees bit for bit (both round the
    same number once), the restatement is within 1.4e-15 (order 7, M 2), 1.6e-15 (7, 5), 2.3e-15 (9, 2), 1.6e-15 (9, 5)."""
    K = GC.half(order)
    case = wp, t, start, end, fix, via = GC.full(order, M)
    assert fix.shape == (GE.N_CASE, M - 1) and (fix == 2 ** (K - 1) - 1).all() and np.isfinite(via).all()
    assert (np.abs(via) > 0).all()                                          # (relative bars divide by these)
    want = GC.hermite_batch(wp, t, GC.knot_states(start, end, via), K)
    agree = norm_rel(GC.exact(("full", order, M), case), want)
    coef = _restated(case, K)
    err = norm_rel(coef, want)
    print(f"order {order} M {M}: fully gated -- gates_exact vs the interpolant {agree}, restatement vs the interpolant {err}")
    assert agree <= 2.0 ** -52, agree
    assert err <= EXACT_BAR, err
    states = GC.knot_states(start, end, via)
    for q in range(1, K):
        got = coef[:, :, :, q] * float(factorial(q))
        assert (np.abs(got - states[:, :-1, :, q - 1]) <= 4 * 2.0 ** -52 * np.abs(states[:, :-1, :, q - 1])).all()


# ---- F. a fault at every knot ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M", GC.FAULT_SEGMENTS)
def test_a_fault_at_every_knot(order, M):
    """The clean batch of the failure test is E's with 16 drones; restatement against 60 digits on it: 5.6e-16 (order
    7, M 2), 6.9e-16 (7, 5), 3.6e-15 (9, 2), 1.0e-15 (9, 5)."""
    K = GC.half(order)
    clean, fix, via, faulted = GC.faults(order, M, "all")
    assert faulted.all() and clean[0].shape[0] == 16
    kinds, knots = set(), set()
    for d in range(16):
        knot, axis, q, kind = GC.fault_of(order, M, d)
        kinds.add(kind)
        knots.add(knot)
        bad_mask = not (0 <= fix[d, knot - 1] < 2 ** (K - 1))
        bad_value = ~np.isfinite(via[d])
        assert bad_mask + int(bad_value.sum()) == 1 and bad_mask == kind.startswith("mask")      # exactly one fault
        assert bad_mask or bad_value[knot - 1, axis, q]
        others = np.delete(np.arange(M - 1), knot - 1)
        assert np.array_equal(fix[d, others], clean[4][d, others])
    assert kinds == set(GC.FAULT_KINDS) and knots == set(range(1, M))        # knot 1 and knot M-1 among them
    if M == 5:                                                              # and every kind at the first and last knot
        assert {GC.fault_of(order, M, d)[3] for d in range(16) if GC.fault_of(order, M, d)[0] == 1} >= {"nan", "mask -1"}
        assert {GC.fault_of(order, M, d)[3] for d in range(16) if GC.fault_of(order, M, d)[0] == 4} >= {"+inf", "-inf"}
    _, fix_odd, via_odd, odd = GC.faults(order, M, "odd")
    assert odd.tolist() == [d % 2 == 1 for d in range(16)]
    assert np.array_equal(fix_odd[::2], clean[4][::2]) and np.array_equal(via_odd[::2], clean[5][::2])
    err = norm_rel(_restated(clean, K), GC.exact(("faults", order, M), clean))
    print(f"order {order} M {M}: the clean batch of the failures, restatement vs 60 digits", err)
    assert err <= EXACT_BAR, err


# ---- G. stiff durations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_stiff_durations(order):
    """Durations alternating 1.5 s and 1.5 / R s, R = 30 at order 7 and 10 at order 9.  Restatement against 60 digits:
    7.2e-13 at order 7, 1.5e-11 at order 9; without gates on the same times 3.1e-12 and 3.0e-10 -- the gates shorten
    the chain the error travels along, and the ungated figure at order 9 is why R stays at 10 there.  (Even drones begin
    with the long segment, odd ones with the short one.)"""
    K = GC.half(order)
    case = wp, t, start, end, fix, via = GC.stiff(order)
    dur = np.diff(t, axis=1)
    R = GC.STIFF_RATIO[order]
    assert np.allclose(dur.max(axis=1), 1.5) and np.allclose(dur.max(axis=1) / dur.min(axis=1), R)
    assert np.allclose(np.maximum(dur[:, 1:] / dur[:, :-1], dur[:, :-1] / dur[:, 1:]), R)      # every knot is stiff
    assert dur[0, 0] == 1.5 and dur[1, 1] == 1.5
    assert np.array_equal(fix, GE.masks(order, GC.M_EDGE))
    err = norm_rel(_restated(case, K), GC.exact(("stiff", order), case))
    plain = (wp, t, start, end, None, None)
    err_plain = norm_rel(_restated(plain, K), GC.exact(("stiff plain", order), plain))
    print(f"order {order}: durations 1.5 s and 1.5 / {R:g} s, restatement vs 60 digits {err}, without gates {err_plain}")
    assert err <= EXACT_BAR, err


# ---- H. translation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("gated", [True, False])
def test_translation(order, gated):
    """2^22 m away on every axis.  The restatement has no refine_end: coefficients 1 .. are the untranslated solve's bit
    for bit, and against 60 digits (coefficients 1 .. only, the constant would drown them): 4.4e-13 / 4.4e-13 at order 7
    gated / not, 5.4e-12 / 9.6e-12 at order 9."""
    K = GC.half(order)
    near, far = GC.translated(order, gated)
    assert (near[4] is not None) == gated
    assert np.array_equal(near[0] / GC.GRID, np.round(near[0] / GC.GRID)) and np.abs(near[0]).max() < 16.0
    assert np.array_equal(far[0] - GC.FAR, near[0])                                              # the offset is exact
    assert np.array_equal(np.diff(far[0], axis=1), np.diff(near[0], axis=1))                     # and so is every step
    a, b = _restated(near, K), _restated(far, K)
    assert np.array_equal(b[..., 0], far[0][:, :-1]) and np.array_equal(b[..., 1:], a[..., 1:])
    ref = GC.exact(("far", order, gated), far)
    assert np.array_equal(ref[..., 0], far[0][:, :-1])
    err = norm_rel(b[..., 1:], ref[..., 1:])
    print(f"order {order} gated {gated}: translated by 2^22 m, restatement vs 60 digits over coefficients 1 ..", err)
    assert err <= EXACT_BAR, err


# ---- I. symmetries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_symmetries(order):
    """The transformed problems are what the GPU test says they are: the 60-digit solution of the problem scaled in
    value is 4 times the original's, of the one scaled in time the original's with coefficient j times 4^-j, both bit
    for bit (one rounding of an exactly scaled number); the reversed problem's is the reversal, to the reference's own
    rounding, checked through the states at every knot.  Restatement against 60 digits on all four: 9.0e-13 at order 7,
    1.3e-11 at order 9 at worst."""
    K = GC.half(order)
    case = GC.dyadic(order)
    dur = np.diff(case[1], axis=1)
    assert np.array_equal(dur * 64, np.round(dur * 64)) and dur.min() >= 0.5 and dur.max() <= 2.0
    assert np.array_equal(case[4], GC.sparse_masks(order))
    ref = GC.exact(("dyadic", order), case)
    inv = (wp4, t4, s4, e4, f4, v4) = GC.scaled_in_value(case)
    assert np.array_equal(v4[~np.isnan(v4)], 4.0 * case[5][~np.isnan(v4)]) and np.array_equal(f4, case[4])
    ref_v = GC.exact(("dyadic x4", order), inv)
    assert np.array_equal(ref_v, 4.0 * ref)
    int_ = GC.scaled_in_time(case, order)
    assert np.array_equal(int_[1], 4.0 * case[1])
    assert np.array_equal(np.nan_to_num(int_[5][..., K - 2]), np.nan_to_num(case[5][..., K - 2]) * 4.0 ** -(K - 1))
    ref_t = GC.exact(("dyadic t4", order), int_)
    assert np.array_equal(ref_t, ref * 4.0 ** -np.arange(2.0 * K))
    rev = GC.reversed_in_time(case, order)
    assert np.array_equal(np.diff(rev[1], axis=1), dur[:, ::-1]) and np.array_equal(rev[4], case[4][:, ::-1])
    assert np.array_equal(rev[1][:, -1], case[1][:, -1])                                  # both running sums are exact
    assert np.array_equal(np.nan_to_num(rev[5][:, :, :, 0]), -np.nan_to_num(case[5][:, ::-1, :, 0]))
    assert np.array_equal(np.nan_to_num(rev[5][:, :, :, 1]), np.nan_to_num(case[5][:, ::-1, :, 1]))
    back = GC.reversed_in_time(rev, order)
    for x, y in zip(back, case):
        assert np.array_equal(x, y, equal_nan=True)
    ref_r = GC.exact(("dyadic reversed", order), rev)
    # p(T - s) of every segment of the reversed solution, through its values: derivative q at the knots
    for d in (0, 3, 32):
        for i in range(GC.M_EDGE):
            for a in range(4):
                c = ref_r[d, GC.M_EDGE - 1 - i, a]
                for q in range(K):
                    fwd = SE.eval_state_mp(ref[d, i, a], 0.0, q)
                    bwd = SE.eval_state_mp(c, dur[d, i], q) * (-1) ** q
                    # (the rounding of the reversed solution's coefficients, carried through the sum at T)
                    scale = sum(SE.falling(j, q) * abs(c[j]) * dur[d, i] ** (j - q) for j in range(q, 2 * K))
                    assert abs(fwd - bwd) <= 4 * 2.0 ** -52 * scale, (d, i, a, q)
    errs = [norm_rel(_restated(c, K), r) for c, r in ((case, ref), (inv, ref_v), (int_, ref_t), (rev, ref_r))]
    print(f"order {order}: dyadic times; as given, x4 in value, x4 in time, reversed: restatement vs 60 digits", errs)
    assert max(errs) <= EXACT_BAR, errs
