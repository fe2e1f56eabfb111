"""The caps and edges of msnap_optimize_times_gates on the CPU (include/msnap.h, msnap_optimize_times_gates; DESIGN.md
§5 K22): the builders of tests/timeopt_gates_cases.py have the structure tests/test_timeopt_gates_edges_gpu.py relies
on, the fixture of tests/golden/make_timeopt_gates_edges_golden.py meets the conditions it was built for and belongs to
these builders, and the NumPy restatement of the masked sweep (tests/gates_ref.py) reaches the 60-digit solve at the
caps at the bar the kernel is then held to.  Every test prints what it measures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gates_cases as GC  # noqa: E402
import gates_exact as GE  # noqa: E402
import gates_ref as GR  # noqa: E402
import states_exact as SE  # noqa: E402
import timeopt_gates_cases as TC  # noqa: E402
import timeopt_gates_ref as G  # noqa: E402
import timeopt_ref as R  # noqa: E402
from conftest import GOLDEN_DIR, norm_rel  # noqa: E402

EXACT_BAR = 1e-10                   # the bar tests/test_gates_edges_cpu.py holds the restatement to
SAME_MINIMUM = 1e-6
MARGIN_MIN = 1e-3
PATH = os.path.join(GOLDEN_DIR, "timeopt_gates_edges_golden.npz")
_Z = {}


def _fixture():
    if not _Z:
        _Z["z"] = np.load(PATH)
        _Z["groups"] = TC.unpack(_Z["z"])
    return _Z["z"], _Z["groups"]


# ---- the builders -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_cap_builders(order):
    K = GC.half(order)
    M = TC.CAP[order]
    wp, t, start, end, fix, via = TC.cap(order)
    assert M == {7: 79, 9: 57}[order] and wp.shape == (11, M + 1, 4) and t.shape == (11, M + 1)
    assert fix.shape == (11, M - 1) and fix.dtype == np.int32 and via.shape == (11, M - 1, 4, K - 1)
    # the combinations cycle; every given state is non-zero, every other row zero; drones 7 and 10 carry an end block
    assert {TC.combo_of(d) for d in range(4)} == {"start", "end", "both", "neither"}
    for d in range(11):
        c = TC.combo_of(d)
        assert (start[d] != 0).all() == (c in ("start", "both")) and (start[d] == 0).all() == (c not in ("start", "both"))
        assert (end[d] != 0).all() == (c in ("end", "both")) and (end[d] == 0).all() == (c not in ("end", "both"))
        one = TC.drone_of((wp, t, start, end, fix, via), c, d)
        assert (one[2] is None) == (c not in ("start", "both")) and (one[3] is None) == (c not in ("end", "both"))
    assert (end[7] != 0).all() and (end[10] != 0).all() and (end[7, 3] != 0).all() and (end[10, 3] != 0).all()
    assert (np.abs(start) <= np.array(SE.STATE_SCALE[:K - 1])).all() and (np.abs(end) <= np.array(SE.STATE_SCALE[:K - 1])).all()
    # the masks
    gated = fix.any(axis=1)
    assert gated.tolist() == [d % 4 != 3 for d in range(11)] and not fix[3].any() and not fix[7].any()
    assert set(fix[fix != 0].tolist()) == set(range(1, 2 ** (K - 1)))             # every non-empty mask value
    for i in TC.always_gated(order):
        assert (fix[gated, i - 1] != 0).all(), i
    assert set(TC.always_gated(order)) >= {1, 2, M - 2, M - 1}
    between = np.delete(fix[gated], [i - 1 for i in TC.always_gated(order)], axis=1)
    share = (between != 0).mean()
    print(f"order {order}: {int((fix != 0).sum())} gated knots, {share:.3f} of the knots between carry a gate")
    assert 0.4 <= share <= 0.6
    if order == 7:
        assert {63, 64, 65} <= set(TC.always_gated(7))
        assert (fix[gated][:, :TC.WORD - 1] != 0).any(axis=1).all() and (fix[gated][:, TC.WORD:] != 0).any(axis=1).all()
    used = np.broadcast_to(GC.used_bits(fix, K)[:, :, None, :], via.shape)
    assert np.isfinite(via[used]).all() and np.isnan(via[~used]).all()
    assert (np.nan_to_num(np.abs(via)) <= np.array(SE.STATE_SCALE[:K - 1])).all()
    # the plain group: the same drones, nothing gated
    plain = TC.cap(order, gated=False)
    for x, y in zip(plain[:4], (wp, t, start, end)):
        assert np.array_equal(x, y)
    assert not plain[4].any() and np.isnan(plain[5]).all()


def test_floor_builder():
    wp, t, start, end, fix, via = TC.floor()
    ref = TC.cap(7)
    for x, y in zip((wp, start, end, fix), (ref[0],) + ref[2:5]):
        assert np.array_equal(x, y)
    used = np.broadcast_to(GC.used_bits(fix, 4)[:, :, None, :], via.shape)             # values of the group's own
    assert np.isfinite(via[used]).all() and np.isnan(via[~used]).all() and not np.array_equal(via[used], ref[5][used])
    assert (np.abs(via[used]) > 0).all() and (np.nan_to_num(np.abs(via)) <= np.array(SE.STATE_SCALE[:3])).all()
    dur, dur0 = np.diff(t, axis=1), np.diff(ref[1], axis=1)
    sq = list(TC.SQUEEZED)
    assert sq == [60, 64, 68, 72, 76] and (t[:, 0] == 0).all() and (dur > 0).all()
    assert np.allclose(dur[:, sq], 0.15 * dur0[:, sq], rtol=1e-12)
    assert np.allclose(np.delete(dur, sq, axis=1), np.delete(dur0, sq, axis=1), rtol=1e-12)
    Tmin = TC.FLOOR_FRACTION * t[:, -1] / 79
    below = dur < Tmin[:, None]
    assert below[:, sq].all() and (below.sum(axis=1) >= 3).all()                 # the input lies below the floor
    assert (below[:, :TC.WORD].any(axis=1) & below[:, TC.WORD:].any(axis=1)).all()


def test_groups_are_the_families():
    names = [g[0] for g in TC.groups()]
    assert names == ["cap7", "cap9", "cap7_plain", "cap9_plain", "floor7", "stiff7", "stiff9"]
    for name, order, mf, combos, batch in TC.groups():
        assert len(combos) == batch[0].shape[0] and mf == (0.5 if name == "floor7" else 0.1)
        if name.startswith("stiff"):
            for x, y in zip(batch, GC.stiff(order)):
                assert np.array_equal(x, y, equal_nan=True)


# ---- the fixture --------------------------------------------------------------------------------------------------------
def test_fixture_conditions():
    assert os.path.getsize(PATH) < 200 * 1024
    z, groups = _fixture()
    built = TC.groups()
    assert [str(x) for x in z["gname"]] == [g[0] for g in built] and int(z["n"]) == sum(len(g[3]) for g in built)
    seg = np.diff(z["off"]) - 1
    for gi, (name, order, mf, combos, batch) in enumerate(built):
        ks = np.flatnonzero(z["group"] == gi)
        assert len(ks) == len(combos) and (seg[ks] == batch[0].shape[1] - 1).all(), name
        assert int(z["order"][gi]) == order and float(z["min_fraction"][gi]) == mf
    assert (z["J_ref"] < z["J0"]).all()
    assert (z["gap4"] >= -1e-12).all() and (z["gap4"][z["conv4"]] <= SAME_MINIMUM).all()
    assert np.array_equal(z["J_ref"], np.minimum(z["J_slsqp"], z["J_descent"]))
    left_out = z["p_margin"] < MARGIN_MIN
    print(f"{int(z['n'])} drones; {int((~z['conv4']).sum())} stopped on max_iter at tol 1e-4; max converged gap4 "
          f"{z['gap4'][z['conv4']].max():.3e}; {int(left_out.sum())} of {left_out.size} prefix runs below the margin, "
          f"smallest margin {z['p_margin'].min():.3g}; prefix_sens max {z['prefix_sens'][~left_out].max():.3e}")
    assert left_out.sum() <= 0.25 * left_out.size
    assert np.isfinite(z["prefix_sens"][~left_out]).all() and (z["prefix_sens"][~left_out] > 0).all()
    assert (z["p_iters"] <= np.array([1, 3])).all() and (z["p_iters"] >= 0).all()
    for name, drones in groups.items():
        for c in drones:
            assert c["p_t"][0][0] == 0.0 and c["p_t"][1][0] == 0.0
            assert (np.diff(c["active"]) > 0).all() and (c["active"] >= 0).all()
    # the floor group
    fl = groups["floor7"]
    fix = TC.floor()[4]
    assert all(c["n_below"] >= 3 for c in fl)
    high = np.array([(c["active"] >= TC.WORD).any() for c in fl])
    both = np.array([(c["active"] >= TC.WORD).any() and (c["active"] < TC.WORD).any() for c in fl])
    print("floor7: active segments at 64 and up per drone",
          [c["active"][c["active"] >= TC.WORD].tolist() for c in fl])
    assert high.sum() >= 4 and (high & fix.any(axis=1)).sum() >= 2 and both.any()
    assert all(c["active"].max(initial=-1) < 79 for c in fl)


def test_the_fixture_belongs_to_the_builders():
    """The file holds no input: J0 of every drone is the restatement's cost at the raised start of the builders'
    drone (2e-9 leaves room for another LAPACK's rounding, as tests/test_timeopt_gates_cpu.py does), n_below is the
    builders', and the prefix runs end at the builders' total duration."""
    z, groups = _fixture()
    worst = 0.0
    seeds = {g[0]: g[4] for g in TC.groups()}
    assert z["r_k"].tolist() == [0, 10, 13, 48, 72, 74] and (z["r_attempt"] == 1).all()     # the drones drawn again
    for name, order, mf, combos, batch in TC.groups(z):
        nd = GC.half(order) - 1
        drawn = [c["k"] in z["r_k"] for c in groups[name]]
        for d, was_drawn in enumerate(drawn):     # a drawn drone has other waypoints and its masks, the others the seeds'
            same = [np.array_equal(x[d], y[d], equal_nan=True) for x, y in zip(batch, seeds[name])]
            assert same[4] and (not same[0] if was_drawn else all(same)), (name, d)
        if name.startswith("stiff"):
            assert np.array_equal(batch[1], seeds[name][1])                                # and a stiff one in its times
        assert (np.abs(batch[2]) <= np.array(SE.STATE_SCALE[:nd])).all() and (np.abs(batch[3]) <= np.array(SE.STATE_SCALE[:nd])).all()
        used = np.broadcast_to(GC.used_bits(batch[4], nd + 1)[:, :, None, :], batch[5].shape)
        assert np.isfinite(batch[5][used]).all() and np.isnan(batch[5][~used]).all() and (batch[5][used] != 0).all()
        for d, (combo, c) in enumerate(zip(combos, groups[name])):
            assert (batch[2][d] != 0).all() == (combo in ("start", "both")) and (batch[3][d] != 0).all() == (combo in ("end", "both"))
            assert (batch[2][d] == 0).all() == (combo not in ("start", "both"))
            assert (batch[3][d] == 0).all() == (combo not in ("end", "both"))
            wp, t, start, end, fix, via = TC.drone_of(batch, combo, d)
            Tmin = R.floor_of(t, mf)
            ts = R.start_times(t, Tmin)
            J0 = G.cost(G.solve(wp, ts, start, end, fix, via, (order + 1) // 2), np.diff(ts), TC.W1)
            worst = max(worst, abs(J0 - c["J0"]) / J0)
            assert abs(J0 - c["J0"]) <= 2e-9 * J0, (name, d, J0, c["J0"])
            assert c["n_below"] == int((np.diff(t) < Tmin).sum()), (name, d)
            for p in c["p_t"]:
                assert p.shape == t.shape and p[-1] == t[-1] and (np.diff(p) >= Tmin * (1 - 1e-12)).all(), (name, d)
    print(f"J0 of the fixture against the builders' drones: within {worst:.2e}")


# ---- the restatement at the caps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_the_restatement_reaches_60_digits_at_the_caps(order):
    """The masked sweep of tests/gates_ref.py at 79 / 57 segments against gates_exact.exact_solve on the cap group, the
    inputs' own times: 2.9e-13 at order 7, 1.2e-11 at order 9, both on a drone without a gate (the gated ones stay below
    1.8e-13: the gates shorten the chain the error travels along) -- the bar of 1e-10 the kernel is held to at t_out
    is reachable in float64."""
    K = GC.half(order)
    wp, t, start, end, fix, via = TC.cap(order)
    got = GR.solve_batch(wp, t, start, end, fix, via, K)
    ref = np.stack([GE.exact_solve(t[d], wp[d], start[d], end[d], fix[d], via[d], K) for d in range(wp.shape[0])])
    errs = [norm_rel(got[d], ref[d]) for d in range(wp.shape[0])]
    print(f"order {order}, {TC.CAP[order]} segments: restatement vs 60 digits, worst {max(errs):.3e}, per drone",
          ["%.1e" % e for e in errs])
    assert max(errs) <= EXACT_BAR, errs


@pytest.mark.parametrize("name", ["cap9", "cap9_plain"])
def test_where_float64_misses_the_bar_at_the_allocated_times(name):
    """Drone 0 of the order-9 cap groups at the times the allocation gives it (tol 1e-4, 500 steps; J falls to 8.5e-4
    of J0 with gates and 5.5e-2 without, and the durations spread to 11 : 1 and 17 : 1): the float64 restatement of the sweep stands
    1.94e-10 (gated) and 1.51e-8 (not) from 60 digits there, above the 1e-10 it meets at the input's times.  The GPU
    test holds the kernel's coefficients of this drone to 10 x the figure (TC.exact_bar); every other drone keeps 1e-10."""
    z, _ = _fixture()
    _, order, mf, combos, batch = {g[0]: g for g in TC.groups(z)}[name]
    K = GC.half(order)
    wp, t, start, end, fix, via = TC.drone_of(batch, combos[0], 0)
    r = G.optimize(wp, t, start, end, fix, via, TC.W1, mf, 500, 1e-4, order + 1)
    dur = np.diff(r["t_out"])
    s0 = np.zeros((4, K - 1)) if start is None else start
    err = norm_rel(GR.solve(wp, r["t_out"], s0, end, fix, via, K), GE.exact_solve(r["t_out"], wp, s0, end, fix, via, K))
    figure = TC.RESTATED_AT_T_OUT[name, 0]
    print(f"{name} drone 0: {r['iters']} steps, J / J0 {r['cost'] / r['cost0']:.2e}, longest / shortest duration "
          f"{dur.max() / dur.min():.1f}, restatement vs 60 digits at its t_out {err:.3e} (recorded {figure:.3e})")
    assert EXACT_BAR < err <= 1.5 * figure, (err, figure)         # (1.5: another LAPACK's rounding)
    assert TC.exact_bar(name, 0, 500) == 10.0 * figure and TC.exact_bar(name, 0, 0) == TC.exact_bar(name, 3, 500) == EXACT_BAR
    assert set(TC.RESTATED_AT_T_OUT) == {("cap9", 0), ("cap9_plain", 0)} and TC.EXACT_BAR == EXACT_BAR
