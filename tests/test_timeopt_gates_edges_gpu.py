"""Time allocation through gates at the caps and edges (include/msnap.h, msnap_optimize_times_gates;
csrc/msnap_timeopt_kernel.h, timeopt_kernel<K, kTimeoptGates>; DESIGN.md §5 K22, "tests at the caps and edges"), on
the inputs of tests/timeopt_gates_cases.py and the fixture of tests/golden/make_timeopt_gates_edges_golden.py:

  A. 79 / 57 segments, where msnap_solve_gates no longer reaches and a full 8-drone tile fills the LDS: structure, the
     coefficients against the 60-digit solve at the kernel's own t_out, the gates on both sides of knot 64, tile
     membership, the prefix of the iteration, the optimum; the same drones through msnap_optimize_times_states;
  B. the floor beyond segment 64 (the second word of the free-set bitmask);
  C. the edge families of tests/gates_cases.py through the allocation, bit for bit msnap_solve_gates at t_out;
  D. exact invariances: value times 4, translation by 2^22 m, time times 4;
  E. a zero weight, stream capture, the host entry without its optional outputs, the argument errors.

The tests print what they measure before they assert (run with -s)."""
import ctypes
import os
import sys
from math import factorial

import numpy as np
import pytest

from conftest import GOLDEN_DIR, norm_rel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gates_cases as GC  # noqa: E402
import gates_exact as GE  # noqa: E402
import states_exact as SE  # noqa: E402
import timeopt_entry_cases as E  # noqa: E402
import timeopt_gates_cases as TC  # noqa: E402
import timeopt_ref as R  # noqa: E402
from test_gates_gpu import EXACT_BAR, FORM_BAR  # noqa: E402
from test_timeopt_gates_gpu import ULP4, _allocate, _mixed_gates, _same, _solve_gates, _worst_jump  # noqa: E402

pytestmark = pytest.mark.gpu

W1 = TC.W1
MARGIN_MIN = 1e-3                    # prefix runs below it are left out
ALONE = (0, 7, 8, 10)                # the first and last drone of the full tile and of the tail
ORDERS = [7, 9]
_Z = {}
_RUN = {}


def _ctx(order, ctx7, ctx9):
    return ctx7 if order == 7 else ctx9


def _fixture():
    if not _Z:
        z = np.load(os.path.join(GOLDEN_DIR, "timeopt_gates_edges_golden.npz"))
        _Z["z"], _Z["ref"] = z, TC.unpack(z)
        _Z["in"] = {g[0]: g for g in TC.groups(z)}
    return _Z["z"], _Z["ref"], _Z["in"]


def _run(ctx, name, max_iter, entry="gates"):
    """The fixture's group `name` at the GPU tests' settings (tol 1e-4), computed once per max_iter and entry"""
    key = (name, max_iter, entry)
    if key not in _RUN:
        _, order, mf, _, (wp, t, start, end, fix, via) = _fixture()[2][name]
        _RUN[key] = _allocate(ctx, entry, wp, t, start, end, (fix, via) if entry == "gates" else (), W1, mf, max_iter, 1e-4)
    return _RUN[key]


def _rows(case, sel):
    return tuple(x if x is None or x.ndim == 1 else np.ascontiguousarray(x[sel]) for x in case)


def _structure(out, t, mf, tag):
    """A.1: status, both end knots, dur = diff(t_out) bit for bit, the floor, the cost not raised"""
    t_out, coef, dur, status, info = out
    N, M = dur.shape
    tt = np.tile(t, (N, 1)) if t.ndim == 1 else t
    assert (status == 0).all(), (tag, status)
    assert (t_out[:, 0] == 0.0).all() and np.array_equal(t_out[:, M], tt[:, M]), tag
    assert np.array_equal(dur, t_out[:, 1:] - t_out[:, :-1]), tag
    Tmin = mf * tt[:, M] / M
    assert (dur >= Tmin[:, None] * (1 - 1e-12)).all(), (tag, float((dur / Tmin[:, None]).min()))
    assert (info["cost"][:, 1] <= info["cost"][:, 0]).all(), tag


def _exact_error(out, case, K, drones):
    """A.2: norm_rel of the coefficients against the 60-digit solve at the kernel's own t_out, taken as data"""
    wp, t, start, end, fix, via = case
    t_out, coef = out[0], out[1]
    errs = []
    for d in drones:
        ref = GE.exact_solve(t_out[d], wp[d], start[d], end[d], fix[d], via[d], K)
        errs.append(norm_rel(coef[d], ref))
    return errs


def _gate_error(coef, fix, via, K):
    """A.3: the largest relative distance of a gated derivative on the leaving segment from its value, and the largest
    gated knot"""
    used = GC.used_bits(fix, K)
    worst = 0.0
    for q in range(1, K):
        sel = used[:, :, q - 1]
        got = coef[:, 1:, :, q][sel] * float(factorial(q))
        want = via[:, :, :, q - 1][sel]
        assert np.isfinite(want).all() and (want != 0).all()
        if want.size:
            worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
    return worst


def _delta(z):
    """The optimality margin by the rule of tests/test_timeopt_gates_gpu.py: 100 x the restatement's largest gap over
    the drones on which it converged, and not below 1e-9"""
    return max(100.0 * float(z["gap4"][z["conv4"]].max()), 1e-9)


def _optimum(out, ref, z, tag):
    """A.6 -> (worst gap to J_ref over the converged drones, worst against a 500-step stop)"""
    delta = _delta(z)
    c_0, c_1 = out[4]["cost"][:, 0], out[4]["cost"][:, 1]
    worst_gap, worst_held = -1.0, -1.0
    lines, fails = [], []
    for d, c in enumerate(ref):
        gap = c_1[d] / c["J_ref"] - 1.0
        lines.append(f"{tag} drone {d}: J/J0 {c_1[d] / c_0[d]:.4g} gap {gap:.3e} pg {out[4]['pg'][d]:.2e} iters "
                     f"{int(out[4]['iters'][d])} (restatement {c['iters4']}, converged {c['conv4']})")
        if not abs(c_0[d] - c["J0"]) <= 1e-9 * c["J0"]:
            fails.append((d, "J0", c_0[d], c["J0"]))
        if c["conv4"]:
            worst_gap = max(worst_gap, gap)
            if not c_1[d] <= c["J_ref"] * (1 + delta):
                fails.append((d, "J_ref", gap, delta))
        else:
            held = c_1[d] / c["J4"] - 1.0
            worst_held = max(worst_held, held)
            if not c_1[d] <= c["J4"] * (1 + 1e-6):
                fails.append((d, "J4", held))
    print("\n".join(lines))
    print(f"{tag}: delta {delta:.3e}, worst gap to J_ref {worst_gap:.3e}, worst against a 500-step stop {worst_held:.3e}")
    assert not fails, fails
    return worst_gap, worst_held


def _prefix(ctx, name, ref, total, entry="gates"):
    """A.5 -> (runs kept, worst |dt| / t[M] in units of prefix_sens)"""
    worst, kept, fails = 0.0, 0, []
    for j, mi in enumerate((1, 3)):
        out = _run(ctx, name, mi, entry)
        assert (out[3] == 0).all()
        for d, c in enumerate(ref):
            if c["p_margin"][j] < MARGIN_MIN:
                continue
            kept += 1
            ratio = float(np.abs(out[0][d] - c["p_t"][j]).max() / total[d]) / float(c["prefix_sens"][j])
            worst = max(worst, ratio)
            if int(out[4]["iters"][d]) != int(c["p_iters"][j]) or not ratio <= 10.0:
                fails.append((d, mi, int(out[4]["iters"][d]), int(c["p_iters"][j]), ratio))
    print(f"{name} ({entry}): {kept} prefix runs, worst |dt| / t[M] = {worst:.2e} x prefix_sens")
    assert kept > 0 and not fails, fails
    return kept, worst


# ---- A. the caps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_cap_structure_and_coefficients_to_60_digits(ctx7, ctx9, order):
    """A.1 and A.2.  Above 47 / 32 segments msnap_solve_gates does not run, so the coefficients are held to
    gates_exact.exact_solve at the kernel's own t_out: all 11 drones at max_iter 0, drones 0, 3, 7 and 10 at max_iter
    500.  The bar is K21's, 1e-10; the NumPy restatement stands 2.9e-13 / 1.2e-11 from 60 digits on these inputs.  One
    drone is held to another bar: at its allocated times drone 0 of order 9 has durations of 11 : 1 (17 : 1 without
    gates), where the float64 restatement itself stands 1.94e-10 (1.51e-8) from 60 digits; the kernel measures 1.83e-10
    (1.60e-8) there and is held to 10 x the restatement's figure (TC.exact_bar; tests/test_timeopt_gates_edges_cpu.py
    measures the figure again).  Measured on an MI355X: DESIGN.md §5 K22."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    name = f"cap{order}"
    assert ctx.optimize_times_gates_max_segments() == TC.CAP[order] and TC.EXACT_BAR == EXACT_BAR
    _, _, mf, _, case = _fixture()[2][name]
    moved = 0
    for mi, drones in ((0, range(TC.N_CAP)), (500, (0, 3, 7, 10))):
        out = _run(ctx, name, mi)
        _structure(out, case[1], mf, (name, mi))
        if mi == 0:
            assert (out[4]["iters"] == 0).all() and np.array_equal(out[0], case[1])
        moved += int(out[4]["iters"].sum())
        errs = _exact_error(out, case, K, drones)
        print(f"order {order}, {TC.CAP[order]} segments, max_iter {mi}: coefficients vs 60 digits at t_out, drones "
              f"{list(drones)}: worst {max(errs):.3e}", ["%.1e" % e for e in errs])
        bars = [TC.exact_bar(name, d, mi) for d in drones]
        assert all(e <= b for e, b in zip(errs, bars)), (mi, errs, bars)
    assert moved > 0


@pytest.mark.parametrize("order", ORDERS)
def test_cap_gates_are_honoured_on_both_sides_of_knot_64(ctx7, ctx9, order):
    """A.3: after the times moved, every gated derivative on the leaving segment within 4 ulp of its value, knots 64
    and up included; the exact jump of the gated derivatives across their knots on drones 0 and 10, at most twice the
    worst jump of the end-state mode across the interior knots of the same two drones."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    name = f"cap{order}"
    _, _, mf, _, (wp, t, start, end, fix, via) = _fixture()[2][name]
    out = _run(ctx, name, 500)
    assert (out[3] == 0).all() and (out[4]["iters"] > 0).all()
    worst = _gate_error(out[1], fix, via, K)
    top = int(np.flatnonzero(fix.any(axis=0)).max()) + 1
    assert top == TC.CAP[order] - 1
    if order == 7:      # (column j of fix is knot j + 1, whose leaving segment is j + 1)
        assert fix[:, TC.WORD - 1:].any(axis=1).sum() == 9
        high = _gate_error(out[1][:, TC.WORD - 1:], fix[:, TC.WORD - 1:], via[:, TC.WORD - 1:], K)
        print(f"order 7: knots 64 and up within {high / 2.0 ** -52:.2f} ulp")
        assert high <= ULP4, high / 2.0 ** -52
    two = [0, 10]
    used = GC.used_bits(fix, K)[two]
    gated = _worst_jump(out[1][two], out[2][two], K, used)
    plain = _allocate(ctx, "states", wp, t, start, end, (), W1, mf, 500, 1e-4)
    assert (plain[3] == 0).all()
    ungated = _worst_jump(plain[1][two], plain[2][two], K, np.ones_like(used))
    print(f"order {order}: leaving segments within {worst / 2.0 ** -52:.2f} ulp of the prescribed values up to knot {top}; "
          f"worst jump of a gated derivative on drones {two} {gated / 2.0 ** -52:.2f} ulp of scale, across the interior "
          f"knots of the end-state mode {ungated / 2.0 ** -52:.2f}")
    assert worst <= ULP4, worst / 2.0 ** -52
    assert 0.0 < gated <= 2.0 * ungated, (gated, ungated)


@pytest.mark.parametrize("order", ORDERS)
def test_cap_tile_membership(ctx7, ctx9, order):
    """A.4: drones 0, 7, 8 and 10 alone give the bits they give in the call; the drones without a gate (3 and 7) give
    the rows of msnap_optimize_times_states on the same 11 drones."""
    ctx = _ctx(order, ctx7, ctx9)
    name = f"cap{order}"
    _, _, mf, _, case = _fixture()[2][name]
    wp, t, start, end, fix, via = case
    for mi in (3, 500):
        whole = _run(ctx, name, mi)
        assert (whole[3] == 0).all() and (whole[4]["iters"] > 0).all()
        for d in ALONE:
            r = _rows(case, slice(d, d + 1))
            one = _allocate(ctx, "gates", *r[:4], r[4:], W1, mf, mi, 1e-4)
            assert _same(whole, one, slice(d, d + 1)), (order, mi, d)
        plain = _allocate(ctx, "states", wp, t, start, end, (), W1, mf, mi, 1e-4)
        ungated = np.flatnonzero(~fix.any(axis=1))
        assert ungated.tolist() == [3, 7]
        assert _same(whole, plain, ungated, ungated), (order, mi)
        assert not np.array_equal(whole[0][0], plain[0][0])          # (a gated drone is another problem)


@pytest.mark.parametrize("order", ORDERS)
def test_cap_prefix_and_optimum(ctx7, ctx9, order):
    """A.5 and A.6 against the fixture.  Measured on an MI355X: DESIGN.md §5 K22."""
    ctx = _ctx(order, ctx7, ctx9)
    name = f"cap{order}"
    z, ref, inputs = _fixture()
    total = inputs[name][4][1][:, -1]
    _prefix(ctx, name, ref[name], total)
    _optimum(_run(ctx, name, 500), ref[name], z, name)


@pytest.mark.parametrize("order", ORDERS)
def test_cap_of_the_end_state_mode_with_a_full_tile(ctx7, ctx9, order):
    """A.7: the cap drones without gates through msnap_optimize_times_states -- a full 8-drone tile whose last drones
    carry non-zero end states, the last words of the LDS layout.  Structure; the coefficients of drones 0, 3, 7 and 10
    against 60 digits at t_out; prefix and optimum against the fixture's ungated group; the end states of drones 7 and
    10 through msnap_eval_state by the rule of tests/test_timeopt_states_gpu.py; the gated entry with fix = NULL and
    with empty masks gives the same bits."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    name = f"cap{order}_plain"
    z, ref, inputs = _fixture()
    _, _, mf, _, case = inputs[name]
    wp, t, start, end, fix, via = case
    assert ctx.optimize_times_states_max_segments() == TC.CAP[order] and not fix.any()
    assert (end[7] != 0).all() and (end[10] != 0).all()
    for mi in (0, 500):
        out = _run(ctx, name, mi, "states")
        _structure(out, t, mf, (name, mi))
        errs = _exact_error(out, case, K, (0, 3, 7, 10))
        print(f"order {order}, end-state mode at {TC.CAP[order]} segments, max_iter {mi}: coefficients of drones 0, 3, 7, 10 "
              f"vs 60 digits at t_out", ["%.1e" % e for e in errs])
        bars = [TC.exact_bar(name, d, mi) for d in (0, 3, 7, 10)]
        assert all(e <= b for e, b in zip(errs, bars)), (mi, errs, bars)
        assert _same(_allocate(ctx, "gates", wp, t, start, end, (None, None), W1, mf, mi, 1e-4), out), (mi, "NULL")
        assert _same(_run(ctx, name, mi, "gates"), out), (mi, "empty masks")
    _prefix(ctx, name, ref[name], t[:, -1], "states")
    out = _run(ctx, name, 500, "states")
    _optimum(out, ref[name], z, name)
    # the end states of the last drone of the full tile and of the call
    t_out, coef, dur = out[0], out[1], out[2]
    N, M = dur.shape
    assert np.array_equal(coef[:, 0, :, 0], wp[:, 0, :])
    p0, d0 = ctx.eval_state(coef, dur, np.zeros(N))
    assert np.array_equal(p0, wp[:, 0, :])
    rel0 = (np.abs(d0 - start) / np.where(start == 0, 1.0, np.abs(start))).max()
    total = np.zeros(N)
    for i in range(M):
        total = total + dur[:, i]
    p1, d1 = ctx.eval_state(coef, dur, total)
    assert np.isfinite(d1).all()
    T, last = dur[:, -1], np.abs(coef[:, -1])
    worst1 = 0.0
    for q in range(0, K):
        want = wp[:, M, :] if q == 0 else end[:, :, q - 1]
        got = p1 if q == 0 else d1[:, :, q - 1]
        scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
        r = np.abs(got - want) / np.maximum(np.abs(want), scale)
        worst1 = max(worst1, float(r[[7, 10]].max()))
        assert (r <= ULP4).all(), (q, (r / 2.0 ** -52).max(axis=1))
    print(f"order {order}: start states within {rel0 / 2.0 ** -52:.2f} ulp; end states of drones 7 and 10 within "
          f"{worst1 / 2.0 ** -52:.2f} ulp of their scale")
    assert rel0 <= ULP4


# ---- B. the floor beyond segment 64 ---------------------------------------------------------------------------------------
def test_floor_beyond_segment_64(ctx7):
    """Order 7, 79 segments, min_fraction 0.5, the input below the floor on segments 60, 64, 68, 72, 76: the raised
    start within the bar of tests/test_timeopt_wide_gpu.py::test_raised_start_on_inputs_below_the_floor, structure,
    gates, prefix and optimum while segments of the second bitmask word sit at their floor."""
    name = "floor7"
    z, ref, inputs = _fixture()
    _, _, mf, _, case = inputs[name]
    wp, t, start, end, fix, via = case
    N, M = t.shape[0], t.shape[1] - 1
    assert mf == 0.5 and M == 79
    out0 = _run(ctx7, name, 0)
    _structure(out0, t, mf, (name, 0))
    bound = 4.0 * M * 2.0 ** -52 * t[:, M]
    Tmin = mf * t[:, M] / M
    err = np.array([np.abs(out0[0][d] - R.start_times(t[d], Tmin[d])).max() for d in range(N)])
    print("floor7, max_iter 0: |t_out - start_times| / bound", np.round(err / bound, 3).tolist())
    assert (err <= bound).all() and (out0[4]["iters"] == 0).all()
    assert np.array_equal(out0[4]["cost"][:, 0], out0[4]["cost"][:, 1])
    out = _run(ctx7, name, 500)
    _structure(out, t, mf, (name, 500))
    assert (out[4]["iters"] > 0).all()
    at_floor = out[2] - Tmin[:, None] <= 1e-6 * Tmin[:, None]
    high = [np.flatnonzero(at_floor[d, TC.WORD:]).tolist() for d in range(N)]
    print("floor7: segments at the floor at 64 and up (index - 64) per drone", high, "; the reference's",
          [(c["active"][c["active"] >= TC.WORD] - TC.WORD).tolist() for c in ref[name]])
    assert sum(1 for h in high if h) >= 4
    worst = _gate_error(out[1], fix, via, 4)
    print(f"floor7: leaving segments within {worst / 2.0 ** -52:.2f} ulp of the prescribed values")
    assert worst <= ULP4
    _prefix(ctx7, name, ref[name], t[:, -1])
    _optimum(out, ref[name], z, name)


# ---- C. K21's families through the allocation ---------------------------------------------------------------------------
def _families(order):
    yield "sparse", GC.sparse(order)
    yield "shared", GC.shared(order)
    for combo in GC.REST_COMBOS:
        yield f"rest {combo}", GC.rest(order, combo)
    for zero in (0.0, -0.0):
        yield f"zeros {zero!r}", GC.zeros(order, zero)
    for M in GC.FULL_SEGMENTS:
        yield f"full {M}", GC.full(order, M)
    yield "stiff", _fixture()[2][f"stiff{order}"][4]      # (GC.stiff but for the drones the fixture drew again)


@pytest.mark.parametrize("order", ORDERS)
def test_edge_families_are_the_gated_solve_at_t_out(ctx7, ctx9, order):
    """Every family of tests/gates_cases.py at max_iter 0 and 500: structure, and coef and dur are msnap_solve_gates' at
    t_out bit for bit -- tests/test_gates_edges_gpu.py pins that solve to 60 digits on these families, so the bits
    carry the exactness over."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    z, ref, _ = _fixture()
    for fam, case in _families(order):
        wp, t, start, end, fix, via = case
        moved = 0
        for mi in (0, 500):
            out = _allocate(ctx, "gates", wp, t, start, end, (fix, via), W1, 0.1, mi, 1e-4)
            _structure(out, t, 0.1, (order, fam, mi))
            cs, ds, ss = _solve_gates(ctx, wp, out[0], start, end, fix, via)
            assert (ss == 0).all(), (fam, ss)
            assert np.array_equal(out[2], ds) and np.array_equal(out[1], cs), (order, fam, mi, norm_rel(out[1], cs))
            moved += int(out[4]["iters"].sum())
            if mi == 0:
                assert (out[4]["iters"] == 0).all()
        print(f"order {order} {fam}: {wp.shape[0]} drones, {moved} accepted steps, coefficients msnap_solve_gates' bits")
        assert moved > 0, fam
        if fam == "sparse":
            plain = _allocate(ctx, "states", wp, t, start, end, (), W1, 0.1, 500, 1e-4)
            free = ~fix.any(axis=1)
            assert free.sum() == 28 and _same(out, plain, free, free)
            for sel in (slice(16, 32), slice(32, 33)):          # tile 1: no gate at all; drone 32: alone in its tile
                r = _rows(case, sel)
                assert _same(out, _allocate(ctx, "gates", *r[:4], r[4:], W1, 0.1, 500, 1e-4), sel), sel
        if fam == "stiff":
            _optimum(out, ref[f"stiff{order}"], z, f"stiff{order}")
        if fam.startswith("zeros"):
            used = GC.used_bits(fix, K)
            for q in range(1, K):
                assert (out[1][:, 1:, :, q][used[:, :, q - 1]] == 0.0).all(), (fam, q)


# ---- D. exact invariances -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_value_times_four_is_exact(ctx7, ctx9, order):
    """Four times every length: t_out, dur, iters and pg keep their bits, coef is 4 times, cost 16 times, bit for bit
    (what tests/test_timeopt_gpu.py holds the plain mode to)."""
    ctx = _ctx(order, ctx7, ctx9)
    for tag, case in (("dyadic", GC.dyadic(order)), ("translated", GC.translated(order, True)[0])):
        wp, t, start, end, fix, via = case
        w4 = GC.scaled_in_value(case)
        for mi in (3, 200):
            a = _allocate(ctx, "gates", wp, t, start, end, (fix, via), W1, 0.1, mi, 1e-4)
            b = _allocate(ctx, "gates", *w4[:4], w4[4:], W1, 0.1, mi, 1e-4)
            assert (a[3] == 0).all() and (b[3] == 0).all() and (a[4]["iters"] > 0).any()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), (tag, mi)
            assert np.array_equal(a[4]["iters"], b[4]["iters"]) and np.array_equal(a[4]["pg"], b[4]["pg"]), (tag, mi)
            assert np.array_equal(b[1], 4.0 * a[1]) and np.array_equal(b[4]["cost"], 16.0 * a[4]["cost"]), (tag, mi)


@pytest.mark.parametrize("order", ORDERS)
def test_translation_by_an_exact_offset(ctx7, ctx9, order):
    """2^22 m away on every axis, every difference of two waypoints the same number: the trials' cost and gradient are
    the unrefined ones and the elimination sees differences only, so t_out, dur, cost, pg and iters keep their bits;
    coef[..., 1:] keeps its bits on every segment but the last, coef[..., 0] is the translated waypoint, and the last
    segment's upper coefficients (refine_end rounds its residual at the size of the position) hold within FORM_BAR as
    in tests/test_gates_edges_gpu.py."""
    ctx = _ctx(order, ctx7, ctx9)
    K = GC.half(order)
    for tag, near in (("translated", GC.translated(order, True)[0]), ("dyadic", GC.dyadic(order))):
        near = (np.round(near[0] / GC.GRID) * GC.GRID,) + near[1:]
        far = (near[0] + GC.FAR,) + near[1:]
        assert np.array_equal(far[0] - GC.FAR, near[0])
        for mi in (3, 200):
            a = _allocate(ctx, "gates", *near[:4], near[4:], W1, 0.1, mi, 1e-4)
            b = _allocate(ctx, "gates", *far[:4], far[4:], W1, 0.1, mi, 1e-4)
            assert (a[3] == 0).all() and (b[3] == 0).all() and (a[4]["iters"] > 0).any()
            same_t = np.array_equal(a[0], b[0])
            err = norm_rel(b[1][:, -1:, :, 1:], a[1][:, -1:, :, 1:])
            print(f"order {order} {tag} max_iter {mi}: t_out bit-identical {same_t}, last segment's coefficients 1 .. "
                  f"vs the untranslated run {err:.3e}")
            assert same_t and np.array_equal(a[2], b[2]), (tag, mi, float(np.abs(a[0] - b[0]).max()))
            for k in ("cost", "pg", "iters"):
                assert np.array_equal(a[4][k], b[4][k]), (tag, mi, k)
            assert np.array_equal(b[1][..., 0], far[0][:, :-1])
            assert np.array_equal(b[1][:, :-1, :, 1:], a[1][:, :-1, :, 1:]), (tag, mi)
            assert np.array_equal(b[1][:, -1, :, 1:K], a[1][:, -1, :, 1:K]), (tag, mi)
            assert err <= FORM_BAR[order], (tag, mi, err)


@pytest.mark.parametrize("order", ORDERS)
def test_time_times_four(ctx7, ctx9, order):
    """t -> 4 t with the q-th derivative of every given state and gate value times 4^-q: the same accepted steps, and
    t_out / 4 within 10 x prefix_sens of the unscaled run at max_iter 1 and 3 (prefix_sens: the largest the fixture
    holds for the order; bit identity is not demanded, the NumPy restatement does not have it either)."""
    ctx = _ctx(order, ctx7, ctx9)
    z, ref, _ = _fixture()
    per_drone = z["order"][z["group"]] == order
    sens = z["prefix_sens"][per_drone][z["p_margin"][per_drone] >= MARGIN_MIN]
    bar = 10.0 * float(sens.max())
    for tag, case in (("dyadic", GC.dyadic(order)), ("translated", GC.translated(order, True)[0])):
        wp, t, start, end, fix, via = case
        s4 = GC.scaled_in_time(case, order)
        for mi in (1, 3):
            a = _allocate(ctx, "gates", wp, t, start, end, (fix, via), W1, 0.1, mi, 1e-4)
            b = _allocate(ctx, "gates", *s4[:4], s4[4:], W1, 0.1, mi, 1e-4)
            assert (a[3] == 0).all() and (b[3] == 0).all() and (a[4]["iters"] > 0).any()
            diff = float((np.abs(b[0] / 4.0 - a[0]).max(axis=1) / t[:, -1]).max())
            print(f"order {order} {tag} max_iter {mi}: |t_out(4t) / 4 - t_out| / t[M] {diff:.3e} (bar {bar:.3e}), "
                  f"bit-identical on {int((b[0] / 4.0 == a[0]).all(axis=1).sum())} of {t.shape[0]} drones")
            assert np.array_equal(a[4]["iters"], b[4]["iters"]), (tag, mi)
            assert diff <= bar, (tag, mi, diff, bar)


# ---- E. what the other modes' tests have ---------------------------------------------------------------------------------
def _entry_batch():
    wp, t, start, end = SE.case(7, 10, N=17)
    fix, via = _mixed_gates(7, 17, 10)
    return wp, t, start, end, fix, via


def test_zero_weight_ignores_the_axis(ctx7):
    wp, t, start, end, fix, via = _entry_batch()
    w = (1.0, 1.0, 1.0, 0.0)
    a = _allocate(ctx7, "gates", wp, t, start, end, (fix, via), w)
    rng = np.random.default_rng(2)
    wp2, s2, e2, v2 = wp.copy(), start.copy(), end.copy(), via.copy()
    wp2[:, :, 3] = rng.normal(size=wp[:, :, 3].shape) * 3.0
    s2[:, 3, :] = rng.normal(size=s2[:, 3, :].shape)
    e2[:, 3, :] = rng.normal(size=e2[:, 3, :].shape)
    v2[:, :, 3, :] = np.where(np.isnan(via[:, :, 3, :]), np.nan, rng.normal(size=via[:, :, 3, :].shape))
    assert not np.array_equal(v2, via, equal_nan=True)
    b = _allocate(ctx7, "gates", wp2, t, s2, e2, (fix, v2), w)
    assert (a[3] == 0).all() and (b[3] == 0).all() and (a[4]["iters"] > 0).any()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[4]["cost"], b[4]["cost"])
    assert np.array_equal(a[1][:, :, :3], b[1][:, :, :3])
    ones = _allocate(ctx7, "gates", wp, t, start, end, (fix, via), W1)
    assert not np.array_equal(ones[0], a[0]) and not np.array_equal(ones[4]["cost"], a[4]["cost"])


def test_entries_and_capture(ctx7):
    """The device entry, eager and inside a captured graph on a context of its own, and the host entry without its
    optional outputs, against the host entry (the shape of tests/test_timeopt_states_gpu.py)."""
    import torch
    from drone_path_planning_python_amd import Context
    wp, t, start, end, fix, via = _entry_batch()
    n, m = 17, 10
    host = ctx7.optimize_times_gates(wp, t, start, end, fix, via)
    assert (host[3] == 0).all() and (host[4]["iters"] > 0).any()
    for states in ((start, end, fix, via), (None, end, fix, via), (start, None, None, None)):
        E.assert_host_entry_without_optionals_is_the_device_entry(ctx7, "_gates", wp, t, states)
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (wp, t, start, end, fix, via)]
    f64 = dict(dtype=torch.float64, device=dev)
    o_t, o_c, o_d = torch.empty((n, m + 1), **f64), torch.empty((n, m, 4, 8), **f64), torch.empty((n, m), **f64)
    o_s = torch.empty((n,), dtype=torch.int32, device=dev)
    o_j, o_p = torch.empty((n, 2), **f64), torch.empty((n,), **f64)
    o_i = torch.empty((n,), dtype=torch.int32, device=dev)
    outs = (o_t, o_c, o_d, o_s, o_j, o_p, o_i)

    def result():
        return tuple(x.cpu().numpy() for x in (o_t, o_c, o_d, o_s)) + \
            ({"cost": o_j.cpu().numpy(), "pg": o_p.cpu().numpy(), "iters": o_i.cpu().numpy()},)

    def call(ctx):
        ctx.optimize_times_gates_device(n, m, ins[0], ins[1], 0, *ins[2:], W1, 0.1, 200, 1e-4, *outs)

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


def test_argument_errors(ctx7, ctx9):
    from drone_path_planning_python_amd._lib import MsnapError
    for ctx in (ctx7, ctx9):
        K = GC.half(ctx.order)
        wp, t, start, end, fix, via = GC.full(ctx.order, 5, 2)
        for kw in ({"weights": (1, -1, 1, 1)}, {"weights": (1, np.nan, 1, 1)}, {"min_fraction": 0.0},
                   {"min_fraction": 1.5}, {"max_iter": -1}, {"tol": -1.0}):
            with pytest.raises(MsnapError) as e:
                ctx.optimize_times_gates(wp, t, start, end, fix, via, **kw)
            assert e.value.code == -1, kw                  # MSNAP_EINVAL
        # one segment above the cap: MSNAP_ESEGMENTS from both entries, nothing written
        top = ctx.optimize_times_gates_max_segments()
        assert top == TC.CAP[ctx.order]
        M = top + 1
        wpb, tb = np.cumsum(np.ones((2, M + 1, 4)), axis=1), np.tile(np.arange(M + 1.0), (2, 1))
        fb, vb = np.ones((2, M - 1), dtype=np.int32), np.ones((2, M - 1, 4, K - 1))
        t_out, coef, dur = np.full((2, M + 1), 7.0), np.full((2, M, 4, 2 * K), 7.0), np.full((2, M), 7.0)
        st = np.full((2,), 7, dtype=np.int32)
        w = (ctypes.c_double * 4)(1, 1, 1, 1)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        for entry in (ctx._lib.msnap_optimize_times_gates, ctx._lib.msnap_optimize_times_gates_device):
            rc = entry(ctx._h, 2, M, vp(wpb), vp(tb), 0, None, None, vp(fb), vp(vb), w, 0.1, 3, 1e-4, vp(t_out), vp(coef),
                       vp(dur), vp(st), None, None, None)
            assert rc == -4, rc                            # MSNAP_ESEGMENTS
        assert (t_out == 7.0).all() and (coef == 7.0).all() and (dur == 7.0).all() and (st == 7).all()
        with pytest.raises(MsnapError) as e:
            ctx.optimize_times_gates(wpb, tb, None, None, fb, vb)
        assert e.value.code == -4
        # no drones: a no-op with the right shapes
        empty = ctx.optimize_times_gates(np.zeros((0, 4, 4)), np.arange(4.0), np.zeros((0, 4, K - 1)), None,
                                         np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2, 4, K - 1)))
        assert empty[0].shape == (0, 4) and empty[1].shape == (0, 3, 4, ctx.ncoef) and empty[2].shape == (0, 3)
        assert empty[3].shape == (0,) and empty[4]["cost"].shape == (0, 2) and empty[4]["iters"].shape == (0,)
