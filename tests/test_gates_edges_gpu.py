"""The edges of msnap_solve_gates on the GPU (include/msnap.h, "gates"), on the inputs of
tests/gates_cases.py -- tests/test_gates_edges_cpu.py holds their structure and shows every bar reachable in float64:
the plain / masked switch inside a tile, shared times, rest ends, prescribed zeros, every knot fully gated, a bad value
or mask at every knot, stiff duration ratios, waypoints far from the origin, and the exact symmetries with gates
carried along.  The bars are tests/test_gates_gpu.py's."""
import os
import sys
from math import factorial

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gates_cases as GC  # noqa: E402
import states_exact as SE  # noqa: E402
from conftest import norm_rel  # noqa: E402
from test_gates_gpu import EXACT_BAR, FORM_BAR, ULP4, _worst_jump  # noqa: E402
from test_states_gpu import _knot_times, _reversed_in_time  # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS = [7, 9]


def _ctx(order, ctx7, ctx9):
    return ctx7 if order == 7 else ctx9


def _same(x, y):
    """(coef, dur, status) bit for bit"""
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


def _rows(case, sel):
    """the drones `sel` of a batch (a 1-D t is shared and stays)"""
    return tuple(x if x is None or x.ndim == 1 else np.ascontiguousarray(x[sel]) for x in case)


def _on_device(order, case, shared_times):
    """msnap_solve_gates_device on a context of its own -> (coef, dur, status) as NumPy arrays"""
    import torch
    from drone_path_planning_python_amd import Context
    wp, t, start, end, fix, via = case
    N, M = wp.shape[0], wp.shape[1] - 1
    dev = torch.device("cuda", 0)
    ins = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in case]
    coef = torch.full((N, M, 4, order + 1), -7.25e300, dtype=torch.float64, device=dev)
    dur = torch.full((N, M), -7.25e300, dtype=torch.float64, device=dev)
    status = torch.full((N,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                  # (the fills run on torch's stream, the solve on the context's)
    with Context(device_id=0, order=order, max_segments=16) as dctx:
        dctx.solve_gates_device(N, M, ins[0], ins[1], shared_times, ins[2], ins[3], ins[4], ins[5], coef, dur, status)
        dctx.sync()
    return coef.cpu().numpy(), dur.cpu().numpy(), status.cpu().numpy()


# ---- A. the plain / masked switch inside a tile ---------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_sparse_tiles_switch_between_the_plain_and_the_masked_step(ctx7, ctx9, order):
    """Tile 0 takes the masked step at knots 1, 3, 5 and the plain one at 2 and 4; tile 1 has fix != NULL and no gate;
    drone 32 is gated at knots 2 and 4.  Every drone is itself solved alone, bit for bit -- alone, the 28 drones without
    a gate take the plain step at every knot, in the batch 12 of them sit beside a gated neighbour -- and a drone without
    a gate has msnap_solve_states' bits: masked terms are selected, never multiplied in.  The same with the batch
    reversed, where drone 32 shares tile 0 with fifteen ungated drones, drones 15, 8 and 3 share tile 1 with drone 16 and
    drone 0 is the lone one.  Measured on an MI355X against 60 digits: 2.9e-13 at order 7, 3.9e-12 at order 9."""
    ctx = _ctx(order, ctx7, ctx9)
    case = wp, t, start, end, fix, via = GC.sparse(order)
    N = wp.shape[0]
    ungated = (fix == 0).all(axis=1)
    got = ctx.solve_gates(*case)
    assert (got[2] == 0).all(), got[2]
    assert np.array_equal(got[1], t[:, 1:] - t[:, :-1])
    for d in range(N):
        assert _same(ctx.solve_gates(*_rows(case, slice(d, d + 1))), [x[d:d + 1] for x in got]), d
    plain = ctx.solve_states(wp, t, start, end)
    assert np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])
    assert np.array_equal(got[0][ungated], plain[0][ungated])
    assert not any(np.array_equal(got[0][d], plain[0][d]) for d in np.flatnonzero(~ungated))     # (the gates act)
    err = norm_rel(got[0], GC.exact(("sparse", order), case))
    print(f"order {order}: sparse tiles vs 60 digits", err)
    assert err <= EXACT_BAR, err
    back = _rows(case, slice(None, None, -1))
    rev = ctx.solve_gates(*back)
    assert _same([x[::-1] for x in rev], got)
    plain_rev = ctx.solve_states(*back[:4])
    assert np.array_equal(rev[1], plain_rev[1]) and np.array_equal(rev[2], plain_rev[2])
    assert np.array_equal(rev[0][ungated[::-1]], plain_rev[0][ungated[::-1]])


# ---- B. shared times ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_shared_times_with_gates(ctx7, ctx9, order):
    """A 1-D t gives the bits of the same row repeated per drone, on the host entry and on the device entry with
    shared_times = 1.  Measured on an MI355X against 60 digits: 3.9e-13 at order 7, 1.1e-12 at order 9."""
    ctx = _ctx(order, ctx7, ctx9)
    case = wp, t, start, end, fix, via = GC.shared(order)
    assert t.ndim == 1
    got = ctx.solve_gates(*case)
    assert (got[2] == 0).all(), got[2]
    tiled = (wp, np.tile(t, (wp.shape[0], 1)), start, end, fix, via)
    assert _same(got, ctx.solve_gates(*tiled))
    assert np.array_equal(got[1], np.tile(t[1:] - t[:-1], (wp.shape[0], 1)))
    err = norm_rel(got[0], GC.exact(("shared", order), case))
    print(f"order {order}: shared times vs 60 digits", err)
    assert err <= EXACT_BAR, err
    assert _same(got, _on_device(order, case, True))
    assert _same(got, _on_device(order, tiled, False))


# ---- C. rest ends ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_rest_ends_with_gates(ctx7, ctx9, order):
    """start and / or end NULL with fix given: the 60-digit minimiser from and to rest, and the bits of an explicit
    block of zeros (tests/test_states_gpu.py, test_zero_states_are_the_rest_to_rest_solve, has the same identity without
    gates).  Measured on an MI355X against 60 digits, (rest, rest) / (given, rest) / (rest, given): 7.3e-14, 2.1e-13,
    1.3e-13 at order 7; 9.0e-13, 9.7e-13, 7.9e-13 at order 9."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    errs = []
    for combo in GC.REST_COMBOS:
        case = wp, t, start, end, fix, via = GC.rest(order, combo)
        got = ctx.solve_gates(*case)
        assert (got[2] == 0).all(), (combo, got[2])
        zero = np.zeros((wp.shape[0], 4, K - 1))
        assert _same(got, ctx.solve_gates(wp, t, zero if start is None else start, zero if end is None else end, fix,
                                          via)), combo
        errs.append(norm_rel(got[0], GC.exact(("rest", order, combo), case)))
    print(f"order {order}: rest ends {GC.REST_COMBOS} vs 60 digits", errs)
    assert max(errs) <= EXACT_BAR, errs


# ---- D. prescribed zeros --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_prescribed_zeros_of_either_sign(ctx7, ctx9, order):
    """A stop at a waypoint, a hold of zero acceleration (the examples of include/msnap.h): every used value 0.0, then
    -0.0.  The leaving segment holds the zero exactly -- z[c] = g[c], row c of G is zero and the products that meet
    them are zeros -- and the arriving segment meets it as in test_the_gate_is_honoured_on_both_sides: the worst jump
    across the gated knots, exact on the float64 coefficients in units of the Horner sum's scale, is at most twice the
    worst jump across the interior knots of msnap_solve_states on the same inputs.  Measured on an MI355X: against 60
    digits 1.3e-13 / 1.2e-12 (order 7 / 9, either sign); the jump in units of 2^-52 of the scale, gated against
    ungated, 81 against 1005 at order 7 and 1224 against 14 967 at order 9."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    ungated = None
    for zero in (0.0, -0.0):
        case = wp, t, start, end, fix, via = GC.zeros(order, zero)
        coef, dur, status = ctx.solve_gates(*case)
        assert (status == 0).all(), status
        used = GC.used_bits(fix, K)
        for q in range(1, K):
            assert (coef[:, 1:, :, q][used[:, :, q - 1]] == 0.0).all(), (zero, q)
        err = norm_rel(coef, GC.exact(("zeros", order), case))
        gated = _worst_jump(coef, dur, K, used | used.any(axis=2, keepdims=True))
        if ungated is None:
            plain = ctx.solve_states(wp, t, start, end)
            ungated = _worst_jump(plain[0], plain[1], K, np.ones_like(used))
        print(f"order {order}: prescribed {zero!r} vs 60 digits {err}; worst jump across gated knots "
              f"{gated / 2.0 ** -52:.2f} ulp of scale, across the interior knots of solve_states {ungated / 2.0 ** -52:.2f}")
        assert err <= EXACT_BAR, err
        assert gated <= 2.0 * ungated, (gated, ungated)


# ---- E. every knot fully gated --------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M", GC.FULL_SEGMENTS)
def test_every_knot_fully_gated_is_hermite_interpolation(ctx7, ctx9, order, M):
    """Every S is the identity and every G zero: status 0, not singular.  Each segment is the interpolant of its two
    knots' states, a closed form that owes nothing to the elimination: the lower coefficients are the given states
    within 4 * 2^-52 relative, the whole is the 60-digit interpolant (one 2K x 2K solve per segment) at EXACT_BAR and
    M one-segment msnap_solve_states calls at FORM_BAR (those refine every segment's end, this solve its last one's).
    Measured on an MI355X, against the interpolant / against the one-segment solves: 2.9e-14 / 3.3e-14
    (order 7, M 2), 2.0e-14 / 3.4e-14 (7, 5), 3.4e-13 / 3.1e-13 (9, 2), 2.9e-13 / 4.5e-13 (9, 5); the lower coefficients
    within 0.66 ulp."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    case = wp, t, start, end, fix, via = GC.full(order, M)
    coef, dur, status = ctx.solve_gates(*case)
    assert (status == 0).all(), status
    assert np.array_equal(dur, t[:, 1:] - t[:, :-1])
    states = GC.knot_states(start, end, via)
    worst = 0.0
    for q in range(1, K):
        want = states[:, :-1, :, q - 1]
        worst = max(worst, (np.abs(coef[:, :, :, q] * float(factorial(q)) - want) / np.abs(want)).max())
    assert np.array_equal(coef[..., 0], wp[:, :-1])
    err = norm_rel(coef, GC.hermite_batch(wp, t, states, K))
    pieces = []
    for i in range(M):
        t1 = np.stack([np.zeros(wp.shape[0]), dur[:, i]], axis=1)
        c1, d1, s1 = ctx.solve_states(np.ascontiguousarray(wp[:, i:i + 2]), t1, np.ascontiguousarray(states[:, i]),
                                      np.ascontiguousarray(states[:, i + 1]))
        assert (s1 == 0).all() and np.array_equal(d1[:, 0], dur[:, i])
        pieces.append(c1)
    form = norm_rel(coef, np.concatenate(pieces, axis=1))
    print(f"order {order} M {M}: fully gated -- lower coefficients within {worst / 2.0 ** -52:.2f} ulp, vs the 60-digit "
          f"interpolant {err}, vs {M} one-segment solve_states {form}")
    assert worst <= ULP4, worst / 2.0 ** -52
    assert err <= EXACT_BAR, err
    assert form <= FORM_BAR[order], form


# ---- F. a non-finite value or a bad mask at every knot --------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M", GC.FAULT_SEGMENTS)
def test_a_bad_value_or_mask_at_every_knot_fails_its_drone(ctx7, ctx9, order, M):
    """Knot 1's mask and values are fetched ahead of the set-up, the last knot's twice, and with two segments the one
    knot is both: drone d carries one NaN, +Inf, -Inf, mask 2^(K-1) or mask -1 at knot 1 + d mod (M-1), on axis d mod 4
    and derivative d mod (K-1).  Every such drone reports MSNAP_ST_NONFINITE with NaN coefficients, dur is written for
    all, and a clean neighbour keeps its bits.  A bad time beside the fault still reports MSNAP_ST_NONFINITE; a bad time
    alone MSNAP_ST_TIMES."""
    ctx = _ctx(order, ctx7, ctx9)
    clean, fix, via, faulted = GC.faults(order, M, "all")
    wp, t, start, end = clean[:4]
    want = ctx.solve_gates(*clean)
    assert (want[2] == 0).all() and np.isfinite(want[0]).all()
    coef, dur, status = ctx.solve_gates(wp, t, start, end, fix, via)
    assert (status == GC.ST_NONFINITE).all(), status
    assert np.isnan(coef).all() and np.array_equal(dur, want[1])
    # faults on the odd drones only: the even ones are the clean solve
    _, fix, via, odd = GC.faults(order, M, "odd")
    coef, dur, status = ctx.solve_gates(wp, t, start, end, fix, via)
    assert (status[odd] == GC.ST_NONFINITE).all() and (status[~odd] == 0).all(), status
    assert np.isnan(coef[odd]).all() and np.array_equal(coef[~odd], want[0][~odd]) and np.array_equal(dur, want[1])
    # precedence: drone 1 has its fault and a time that does not increase, drone 2 the time alone
    t2 = t.copy()
    j = M // 2 + 1
    t2[1, j] = t2[1, j - 1]
    t2[2, j] = t2[2, j - 1]
    coef, dur, status = ctx.solve_gates(wp, t2, start, end, fix, via)
    expect = np.where(odd, GC.ST_NONFINITE, 0)
    expect[2] = GC.ST_TIMES
    assert np.array_equal(status, expect), status
    failed = expect != 0
    assert np.isnan(coef[failed]).all() and np.array_equal(coef[~failed], want[0][~failed])
    assert np.array_equal(dur, t2[:, 1:] - t2[:, :-1]) and dur[1, j - 1] == 0.0 and dur[2, j - 1] == 0.0


# ---- G. stiff durations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_stiff_duration_ratios(ctx7, ctx9, order):
    """Durations alternating 1.5 s and 1.5 / R s, R = 30 at order 7 and 10 at order 9 (the float64 restatement leaves
    2e-10 at order 9 with R = 30: tests/test_gates_edges_cpu.py has its figures on these inputs).  Measured on an
    MI355X against 60 digits: 5.3e-13 at order 7, 4.1e-11 at order 9 (the restatement: 7.2e-13, 1.5e-11)."""
    ctx = _ctx(order, ctx7, ctx9)
    case = wp, t, start, end, fix, via = GC.stiff(order)
    coef, dur, status = ctx.solve_gates(*case)
    assert (status == 0).all(), status
    assert np.array_equal(dur, t[:, 1:] - t[:, :-1])
    err = norm_rel(coef, GC.exact(("stiff", order), case))
    print(f"order {order}: durations 1.5 s and 1.5 / {GC.STIFF_RATIO[order]:g} s vs 60 digits", err)
    assert err <= EXACT_BAR, err


# ---- H. translation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("gated", [True, False])
def test_translation_by_an_exact_offset(ctx7, ctx9, order, gated):
    """Waypoints on a 2^-20 m grid, then 2^22 m away on every axis: every difference of two waypoints is the same
    number.  The elimination and recover_segment see differences only, so coef[..., 0] is the translated waypoint and
    coefficients 1 .. are the untranslated solve's bit for bit -- on every segment but the last.  There refine_end
    evaluates the *position* at the end and takes its residual out of the upper coefficients K .. 2K-1; the residual
    is rounded at the size of the position, so those four / five coefficients move, within FORM_BAR (norm_rel over
    coefficients 1 .. of the last segment: c[0] would drown it), and coefficients 1 .. K-1 do not.  The end state still
    comes back through msnap_eval_state within the bound include/msnap.h states for msnap_solve_states.  gated False is
    msnap_solve_states itself (fix = NULL).  Measured on an MI355X, last segment's upper coefficients / end state in
    ulp of its scale: 3.5e-12 / 1.00 ulp at order 7, 1.7e-10 / 0.84 ulp
    at order 9, the same gated and not (the worst drone carries no gate)."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    near, far = GC.translated(order, gated)
    a, b = ctx.solve_gates(*near), ctx.solve_gates(*far)
    assert (a[2] == 0).all() and (b[2] == 0).all() and np.array_equal(a[1], b[1])
    if not gated:
        assert _same(b, ctx.solve_states(*far[:4]))
    assert np.array_equal(b[0][..., 0], far[0][:, :-1])
    assert np.array_equal(b[0][:, :-1, :, 1:], a[0][:, :-1, :, 1:])
    assert np.array_equal(b[0][:, -1, :, 1:K], a[0][:, -1, :, 1:K])
    err = norm_rel(b[0][:, -1:, :, 1:], a[0][:, -1:, :, 1:])
    # the end state, as tests/test_states_gpu.py test_the_given_end_is_honoured holds it
    coef, dur = b[0], b[1]
    end = far[3]
    _, d1 = ctx.eval_state(coef, dur, _knot_times(dur)[:, -1])
    assert np.isfinite(d1).all()
    T, last = dur[:, -1], np.abs(coef[:, -1])
    worst = 0.0
    for q in range(1, K):
        scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
        r = np.abs(d1[:, :, q - 1] - end[:, :, q - 1]) / np.maximum(np.abs(end[:, :, q - 1]), scale)
        worst = max(worst, r.max())
    print(f"order {order} gated {gated}: 2^22 m away -- last segment's coefficients 1 .. vs the untranslated solve {err}, "
          f"end state within {worst / 2.0 ** -52:.2f} ulp of its scale")
    assert err <= FORM_BAR[order], err
    assert worst <= ULP4, worst / 2.0 ** -52


# ---- I. symmetries with gates ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_scaling_by_four_is_exact_with_gates(ctx7, ctx9, order):
    """tests/test_states_gpu.py test_scaling_by_four_is_exact with fix and via carried along, in value and in time.
    Four times every length -- waypoints, end states, gate values -- is four times every coefficient.  Four times
    every time, with the q-th derivative of every given state and gate value times 4^-q, is coefficient j times 4^-j
    and four times every duration: every operand of the sweep scales by a power of two, the masked rows' 1.0 on the
    diagonal of S multiplies nothing but its own right-hand side, and refine_end's local time scales with the rest.
    Both bit for bit."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    case = GC.dyadic(order)
    coef, dur, status = ctx.solve_gates(*case)
    assert (status == 0).all(), status
    c4, d4, s4 = ctx.solve_gates(*GC.scaled_in_value(case))
    assert np.array_equal(c4, 4.0 * coef) and np.array_equal(d4, dur) and np.array_equal(s4, status)
    ct, dt, st = ctx.solve_gates(*GC.scaled_in_time(case, order))
    assert np.array_equal(dt, 4.0 * dur) and np.array_equal(st, status)
    assert np.array_equal(ct, coef * 4.0 ** -np.arange(2.0 * K))


@pytest.mark.parametrize("order", ORDERS)
def test_time_reversal_with_gates(ctx7, ctx9, order):
    """tests/test_states_gpu.py test_time_reversal with gates: the mask rows and the value rows reverse, the end states
    swap, the odd derivatives change sign; durations dyadic, so both running sums are exact.  The reversed problem's
    solution, expanded as p(T - s) per segment at 60 digits, against the forward one at FORM_BAR; both against 60
    digits at EXACT_BAR.  Measured on an MI355X, reversal / forward / reversed: 5.4e-13 / 2.6e-13 / 4.0e-13 at order 7,
    2.5e-11 / 9.8e-12 / 1.8e-11 at order 9."""
    ctx = _ctx(order, ctx7, ctx9)
    case = GC.dyadic(order)
    rev = GC.reversed_in_time(case, order)
    fwd, dur_f, st = ctx.solve_gates(*case)
    assert (st == 0).all() and np.array_equal(dur_f, np.diff(case[1], axis=1))
    bwd, dur_b, st = ctx.solve_gates(*rev)
    assert (st == 0).all() and np.array_equal(dur_b, dur_f[:, ::-1])
    err = norm_rel(_reversed_in_time(bwd, dur_b), fwd)
    e_f = norm_rel(fwd, GC.exact(("dyadic", order), case))
    e_b = norm_rel(bwd, GC.exact(("dyadic reversed", order), rev))
    print(f"order {order}: a gated path against the reversal of the reversed problem {err}; vs 60 digits forward {e_f}, "
          f"reversed {e_b}")
    assert err <= FORM_BAR[order], err
    assert max(e_f, e_b) <= EXACT_BAR, (e_f, e_b)
