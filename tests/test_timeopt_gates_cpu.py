"""Time allocation through gates, what needs no GPU (include/msnap.h, msnap_optimize_times_gates):
the three symbols through every layer, the closed-form gradient of the restatement tests/timeopt_gates_ref.py against
central differences of its own solved cost, the fixture of tests/golden/make_timeopt_gates_golden.py and the
restatement on it, the exec check on the new object, swarm.replan_gated's refusals."""
import ctypes
import inspect
import os
import re
import subprocess
import sys
from math import factorial

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import states_exact as SE  # noqa: E402
import timeopt_gates_ref as G  # noqa: E402
import timeopt_ref as R  # noqa: E402
from conftest import GOLDEN_DIR, ROOT  # noqa: E402

COMBOS = ("start", "end", "both", "neither")
FIRST_TD8 = {7: 40, 9: 29}
NAMES = ("msnap_optimize_times_gates", "msnap_optimize_times_gates_device", "msnap_optimize_times_gates_max_segments")
_Z = {}


def _fixture():
    if not _Z:
        z = np.load(os.path.join(GOLDEN_DIR, "timeopt_gates_golden.npz"))
        _Z["z"], _Z["cases"] = z, G.unpack_cases(z)
    return _Z["z"], _Z["cases"]


# ---- 1. the symbols --------------------------------------------------------------------------------------------------
def test_the_three_symbols_through_every_layer():
    from drone_path_planning_python_amd import Context, _lib, swarm
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        m = re.search(rf"\bint {name}\s*\(([^)]*)\)", text)
        assert m and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in NAMES[:2]:      # a null context: MSNAP_EINVAL
        assert getattr(lib, name)(None, 1, 2, p, p, 0, None, None, None, None, p, 0.1, 1, 1e-4, p, p, p, p, None, None,
                                  None) == -1
    assert [lib.msnap_optimize_times_gates_max_segments(o) for o in (7, 9, 8)] == [79, 57, -3]
    assert [lib.msnap_optimize_times_gates_max_segments(o) for o in (7, 9)] == \
        [lib.msnap_optimize_times_states_max_segments(o) for o in (7, 9)]
    for name in ("optimize_times_gates", "optimize_times_gates_device", "optimize_times_gates_max_segments"):
        assert hasattr(Context, name), name
    want = ["wp", "t", "start", "end", "fix", "via", "weights", "min_fraction", "max_iter", "tol"]
    assert list(inspect.signature(swarm.DeviceCompute.optimize_times_gates).parameters)[1:] == want
    assert list(inspect.signature(Context.optimize_times_gates).parameters)[1:] == want
    assert list(inspect.signature(swarm.replan_gated).parameters) == ["compute", "coef", "dur", "t_r", "wp_new", "t_new",
                                                                      "gates", "end", "optimize"]


# ---- 2. the gradient ----------------------------------------------------------------------------------------------------
def _gradient_gap(c):
    """worst |fd - g_i| / max |g| of one fixture drone at its input times, central differences at h = 1e-5 T_i"""
    nc, w = c["order"] + 1, (2.0, 0.5, 1.0, 3.0)
    args = (w, nc, c["start"], c["end"], c["fix"], c["via"])
    J, g, _ = G.evaluate(c["wp"], c["t"], *args)
    T = np.diff(c["t"])
    worst = 0.0
    for i in range(len(T)):
        h = 1e-5 * T[i]
        Jpm = []
        for sgn in (+1, -1):
            T2 = T.copy()
            T2[i] += sgn * h
            Jpm.append(G.evaluate(c["wp"], np.concatenate([[0.0], np.cumsum(T2)]), *args)[0])
        worst = max(worst, abs((Jpm[0] - Jpm[1]) / (2 * h) - g[i]) / np.abs(g).max())
    return worst


@pytest.mark.parametrize("order", [7, 9])
def test_closed_form_gradient_against_central_differences(order):
    """dJ*/dT_i = -sum_a w_a E_i,a with prescribed derivatives at interior knots: a gated component is data, which the
    envelope argument does not look at.  On the fixture's 2-, 3- and 10-segment drones, gated and not, weights
    (2, 0.5, 1, 3); the bar is the states mode's, 1e-6 of the largest component."""
    _, cases = _fixture()
    worst, n, gated = 0.0, 0, 0
    for c in cases:
        if c["order"] != order or len(c["t"]) - 1 not in (2, 3, 10):
            continue
        gap = _gradient_gap(c)
        worst, n, gated = max(worst, gap), n + 1, gated + int((c["fix"] != 0).any())
        assert gap <= 1e-6, (c["k"], gap)
    print(f"order {order}: {n} drones ({gated} gated), worst |fd - g| / max |g| = {worst:.2e}")
    assert n >= 12 and gated >= 9


# ---- 3. the fixture and the restatement on it ---------------------------------------------------------------------------
def test_fixture_invariants():
    path = os.path.join(GOLDEN_DIR, "timeopt_gates_golden.npz")
    assert os.path.getsize(path) < 200 * 1024
    z, cases = _fixture()
    seg = np.diff(z["off"]) - 1
    order = z["order"][z["group"]]
    assert 40 <= int(z["n"]) <= 64 and (seg > 1).all()
    for o in (7, 9):
        have = set(seg[order == o].tolist())
        assert {2, 3, 10, FIRST_TD8[o]} <= have, (o, have)
        assert max(np.bincount(z["group"][(order == o) & (seg == FIRST_TD8[o])])) == 11
        nm = 2 ** ((o + 1) // 2 - 1)
        assert {int(v) for c in cases if c["order"] == o for v in c["fix"]} == set(range(nm))      # every mask value
    groups = {}
    for c in cases:
        groups.setdefault(c["group"], []).append(c)
        t, nd = c["t"], (c["order"] + 1) // 2 - 1
        M = len(t) - 1
        assert t[0] == 0.0 and (np.diff(t) >= 0.5).all() and (np.diff(t) <= 2.0).all() and c["wp"].shape == (M + 1, 4)
        for blk in (c["start"], c["end"]):
            assert blk is None or (blk.shape == (4, nd) and (np.abs(blk) <= np.array(SE.STATE_SCALE[:nd])).all())
        fix, via = c["fix"], c["via"]
        assert fix.shape == (M - 1,) and via.shape == (M - 1, 4, nd) and (fix >= 0).all() and (fix < 2 ** nd).all()
        used = np.broadcast_to((((fix[:, None] >> np.arange(nd)) & 1).astype(bool))[:, None, :], via.shape)
        assert np.isfinite(via[used]).all() and np.isnan(via[~used]).all()
        assert (np.abs(via[used].reshape(-1)) <= np.broadcast_to(np.array(SE.STATE_SCALE[:nd]), via.shape)[used]).all()
        if fix.any():      # gates at knot 1, at knot M-1 and at adjacent knots
            assert fix[0] != 0 and fix[-1] != 0 and (M < 3 or fix[1] != 0), c["k"]
    for g, drones in groups.items():
        gated = [bool(c["fix"].any()) for c in drones]
        assert any(gated) and not all(gated), g                 # some drones in every group carry no gate
        nm = 2 ** ((drones[0]["order"] + 1) // 2 - 1)
        vals = [int(v) for c in drones for v in c["fix"] if v]
        assert len(vals) < nm - 1 or set(vals) == set(range(1, nm)), g      # the masks cycle through every value
    assert set(z["combo"].tolist()) == set(COMBOS)
    assert (z["gap4"] >= -1e-12).all() and z["gap4"][z["conv4"]].max() < 1e-6
    assert np.array_equal(z["J_ref"], np.minimum(z["J_slsqp"], z["J_descent"]))
    assert (z["J_ref"] < z["J0"]).all()
    assert z["shared"].sum() == 1 and (np.asarray(z["weights"]) != 1.0).any(axis=1).sum() == 1
    assert [tuple(w) for w in np.asarray(z["weights"]) if (w != 1.0).any()] == [(2.0, 0.5, 1.0, 3.0)]
    floor = z["min_fraction"][z["group"]] == 0.5
    assert floor.sum() == 4 and (z["n_below"][floor] > 0).all()
    # the prefix runs: at most a quarter left out, every (order, combination) keeps one
    left_out = z["p_margin"] < 1e-3
    assert left_out.sum() <= 0.25 * left_out.size
    kept = ~left_out
    assert np.isfinite(z["prefix_sens"][kept]).all() and (z["prefix_sens"][kept] > 0).all()
    for o in (7, 9):
        for c in COMBOS:
            assert kept[(order == o) & (z["combo"] == c)].any(), (o, c)


def test_the_restatement_holds_every_gate_exactly_at_the_gpu_tests_settings():
    """On every fixture drone: the restatement at tol 1e-4, 500 steps, lowers the cost, keeps the floor and both end
    knots, and its coefficients at t_out carry every gated derivative on the leaving segment exactly -- tests/gates_ref.py
    writes u / q!, and u is the value itself.  The cost at t_out is held to the fixture's reference as the GPU test
    holds the kernel (the bounds leave room for another LAPACK's rounding, nothing else)."""
    z, cases = _fixture()
    delta = max(100.0 * float(z["gap4"][z["conv4"]].max()), 1e-9)
    checked = 0
    for c in cases:
        k, nc, w, mf = c["k"], c["order"] + 1, c["weights"], c["min_fraction"]
        r4 = G.optimize(c["wp"], c["t"], c["start"], c["end"], c["fix"], c["via"], w, mf, 500, 1e-4, nc)
        t4 = r4["t_out"]
        coef = G.solve(c["wp"], t4, c["start"], c["end"], c["fix"], c["via"], nc // 2)
        J4 = G.cost(coef, np.diff(t4), w)
        assert abs(r4["cost0"] - float(z["J0"][k])) <= 2e-9 * r4["cost0"], k
        assert J4 <= r4["cost0"] and (np.diff(t4) >= R.floor_of(c["t"], mf) * (1 - 1e-12)).all(), k
        assert t4[0] == 0.0 and t4[-1] == c["t"][-1] and r4["iters"] > 0, k
        if bool(z["conv4"][k]):
            assert J4 <= float(z["J_ref"][k]) * (1 + delta), (k, J4, float(z["J_ref"][k]))
        else:
            assert J4 <= float(z["J4"][k]) * (1 + 1e-6), (k, J4, float(z["J4"][k]))
        for i, q, got, want in G.gated_values(coef, c["fix"], c["via"]):
            assert np.array_equal(coef[i, :, q], want / factorial(q)), (k, i, q)
            assert (np.abs(got - want) <= 2.0 ** -52 * np.abs(want)).all(), (k, i, q)
            checked += 1
    assert checked > 400


# ---- 4. the exec check -----------------------------------------------------------------------------------------------
def test_the_exec_check_names_the_new_object_and_passes_on_it():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    csrc = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc")
    obj = os.path.join(csrc, "msnap_timeopt_gates.o")
    assert chk.K22_OBJS == [obj] and chk.K21_OBJS == [os.path.join(csrc, "msnap_gates.o")]
    with open(os.path.join(csrc, "Makefile")) as f:
        assert "msnap_timeopt_gates.hip" in f.read()
    if os.path.exists(obj) and os.path.exists(f"{chk.LLVM}/llvm-objdump"):      # (a machine that built the library)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), obj], capture_output=True,
                           text=True)
        assert r.returncode == 0 and "2 kernels" in r.stdout and "none under a reduced exec mask" in r.stdout, \
            r.stdout + r.stderr
        assert chk.lane_latches(obj) == {}
        # a run without arguments covers it
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py")], capture_output=True, text=True)
        assert r.returncode == 0 and "msnap_timeopt_gates.o" in r.stdout, r.stdout + r.stderr


# ---- 5. swarm.replan_gated ------------------------------------------------------------------------------------------------
def test_replan_gated_refuses_a_free_total_and_replan_still_refuses_gates_with_optimize():
    from drone_path_planning_python_amd import swarm
    with pytest.raises(ValueError, match="time_weight"):
        swarm.replan_gated(None, None, None, 0.0, None, None, (None, None), optimize={"time_weight": 1.0})
    with pytest.raises(ValueError, match="steps"):
        swarm.replan_gated(None, None, None, 0.0, None, None, (None, None), optimize={"steps": 3})
    with pytest.raises(ValueError, match="gates") as e:
        swarm.replan(None, None, None, 0.0, None, None, optimize={}, gates=(None, None))
    assert "replan_gated" in str(e.value)


def test_the_wrappers_check_fix_and_via_as_solve_gates_does():
    from drone_path_planning_python_amd import Context
    ctx = Context.__new__(Context)      # (the shape checks need no library)
    ctx.ncoef, ctx.order = 8, 7
    wp, t, _, _ = SE.case(7, 3, N=2)
    fix = np.zeros((2, 2), dtype=np.int32)
    for bad in ({"fix": fix}, {"fix": fix[:, :1], "via": np.zeros((2, 2, 4, 3))}, {"fix": fix, "via": np.zeros((2, 2, 4, 4))}):
        for call in (ctx.optimize_times_gates, ctx.solve_gates):
            with pytest.raises(ValueError):
                call(wp, t, **bad)
