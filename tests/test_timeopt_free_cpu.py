"""Time allocation with a free total duration without a GPU: the closed-form gradient k_T - sum_a w_a E_i,a against
central differences of the solved objective with every duration -- and so the total -- free, Euler's identity on the
restatement, the fixture's own conditions and that it reproduces from the restatement, the wiring of the entry
points, and the exec check on the object that holds the new kernels."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import states_exact as SE  # noqa: E402
import timeopt_free_ref as FR  # noqa: E402
import timeopt_states_ref as S  # noqa: E402
from conftest import GOLDEN_DIR, ROOT  # noqa: E402

NEW = ["msnap_optimize_times_free", "msnap_optimize_times_free_device", "msnap_optimize_times_free_max_segments"]
COMBOS = ("start", "end", "both", "neither")
FIRST_TD8 = {7: 40, 9: 29}
MAX_SEG = {7: 79, 9: 57}
KINDS = {"walk", "tile8", "cap", "shared", "weights", "below", "span"}
W_MIXED = (2.0, 0.5, 1.0, 3.0)


def _knots(T):
    return np.concatenate([[0.0], np.cumsum(T)])


@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 10])
def test_closed_form_gradient_against_central_differences(order, M):
    """dF/dT_i = k_T - sum_a w_a E_i,a with nothing held: each T_i is moved alone, so the total moves with it.  Nonzero
    states at both ends, weights (2, 0.5, 1, 3); the difference step is 1e-5 of the duration and the bound 1e-6 of the
    largest component, as tests/test_timeopt_periodic_cpu.py takes both.  Measured on these cases: within 2.2e-9
    (order 7) and 4.4e-8 (order 9)."""
    wp, t, start, end = SE.case(order, M, N=1)
    wp, t, s, e = wp[0], t[0], start[0], end[0]
    assert np.abs(s).min() > 0 and np.abs(e).min() > 0
    kT = 3.7
    F, g, J, _ = FR.evaluate(wp, t, W_MIXED, kT, order + 1, s, e)
    assert F == J + kT * t[-1]
    T = np.diff(t)
    worst = 0.0
    for i in range(M):
        h = 1e-5 * T[i]
        Fpm = []
        for sgn in (+1, -1):
            T2 = T.copy()
            T2[i] += sgn * h
            Fpm.append(FR.evaluate(wp, _knots(T2), W_MIXED, kT, order + 1, s, e)[0])
        fd = (Fpm[0] - Fpm[1]) / (2 * h)
        worst = max(worst, abs(fd - g[i]) / np.abs(g).max())
        assert abs(fd - g[i]) <= 1e-6 * np.abs(g).max(), (i, fd, g[i])
    print(f"order {order} M {M}: central differences within {worst:.2e} of the largest component")


@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("M", [1, 3, 10])
def test_euler_identity_with_zero_states(order, M):
    """Rest to rest J is homogeneous of degree -(2k - 1) in the durations, so sum_i T_i g_i = k_T T - (2k - 1) J at
    every point (the dense solve's rounding: 1e-8 of the larger term), and at a converged return with no segment at
    the floor |(2k - 1) J - k_T T| <= tol sqrt(M) F -- derived from the stopping measure, |sum T_i g_i| <= |g|_2 T."""
    wp, t, _, _ = SE.case(order, M, N=1)
    wp, t = wp[0], t[0]
    J_in = S.cost(S.solve(wp, t, None, None, (order + 1) // 2), np.diff(t), W_MIXED)
    kT = 0.3 * order * J_in / t[-1]
    F, g, J, _ = FR.evaluate(wp, t, W_MIXED, kT, order + 1)
    lhs, rhs = float(np.dot(np.diff(t), g)), kT * t[-1] - order * J
    print(f"order {order} M {M}: sum T g = {lhs:.9g}, k_T T - (2k-1) J = {rhs:.9g}")
    assert abs(lhs - rhs) <= 1e-8 * max(kT * t[-1], order * J)
    tol = 1e-5
    r = FR.optimize(wp, t, None, None, W_MIXED, kT, 0.01, 2000, tol, order + 1)
    Tmin = FR.floor_of(t, 0.01)
    assert r["pg"] <= tol and (np.diff(r["t_out"]) > Tmin * (1 + 1e-6)).all()
    miss = abs(order * r["J"] - kT * r["t_out"][-1])
    print(f"    at return: |(2k-1) J - k_T T| = {miss:.3e}, bound {tol * np.sqrt(M) * r['cost']:.3e}")
    assert miss <= tol * np.sqrt(M) * r["cost"]


def _fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "timeopt_free_golden.npz"))
    return z, FR.unpack_cases(z)


def test_fixture_invariants_and_the_objective_falls_on_every_drone():
    path = os.path.join(GOLDEN_DIR, "timeopt_free_golden.npz")
    assert os.path.getsize(path) < 200 * 1024
    z, cases = _fixture()
    n = int(z["n"])
    assert 60 <= n <= 80 and 14 <= len(z["order"]) <= 20
    seg = np.diff(z["off"]) - 1
    order = z["order"][z["group"]]
    kind = z["kind"][z["group"]]
    assert set(kind.tolist()) == KINDS
    for o in (7, 9):
        have = set(seg[order == o].tolist())
        assert {1, 2, 3, 10, 20, FIRST_TD8[o], MAX_SEG[o]} <= have, (o, have)
        assert max(np.bincount(z["group"][(order == o) & (seg == FIRST_TD8[o])])) == 11      # a full tile and a tail of 3
    for c in cases:
        t, nd = c["t"], (c["order"] + 1) // 2 - 1
        assert t[0] == 0.0 and (np.diff(t) > 0).all() and c["wp"].shape == (len(t), 4) and c["time_weight"] > 0
        for blk in (c["start"], c["end"]):
            assert blk is None or (blk.shape == (4, nd) and (np.abs(blk) <= np.array(SE.STATE_SCALE[:nd])).all())
    assert set(z["combo"].tolist()) == set(COMBOS)
    # the objective falls on every drone, at the reference and at the GPU test's settings, one segment included
    assert (z["F_ref"] < z["F0"]).all() and (z["F4"] < z["F0"]).all()
    assert (z["gap4"] >= 0).all() and z["gap4"][z["conv4"]].max() < 1e-6
    assert float(z["delta"]) == max(100.0 * float(z["gap4"][z["conv4"]].max()), 1e-9)
    assert (~z["conv4"]).sum() <= 0.05 * n
    assert z["shared"].sum() == 1 and (np.asarray(z["weights"]) != 1.0).any(axis=1).sum() == 1
    # the floor: raised starts whose total grows, a heavy weight that ends at it, a light one whose total grows
    below = kind == "below"
    assert below.sum() == 4 and (z["n_below"][below] > 0).all() and (z["T_start"][below] > z["T_in"][below]).all()
    span = np.flatnonzero(kind == "span")
    tw = z["time_weight"][span]
    assert len(span) == 4 and tw.max() / tw.min() >= 1e3
    heavy, light = span[0], span[-1]
    assert 3 <= z["active"][heavy] < seg[heavy] and z["first_active"][heavy] and z["last_active"][heavy]
    assert z["T_ref"][light] > z["T_in"][light] and z["T4"][light] > z["T_in"][light]
    assert (z["T4"] <= z["F0"] / z["time_weight"]).all()
    left_out = z["p_margin"] < 1e-3
    assert left_out.sum() <= 0.25 * 2 * n
    assert np.isfinite(z["prefix_sens"][~left_out]).all() and (z["prefix_sens"][~left_out] > 0).all()
    for o in (7, 9):
        for cb in COMBOS:
            assert (~left_out)[(order == o) & (z["combo"] == cb)].any(), (o, cb)
    print(f"fixture: {n} drones in {len(z['order'])} calls, {int((~z['conv4']).sum())} unconverged at tol 1e-4, "
          f"{int(left_out.sum())} prefix runs left out, delta {float(z['delta']):.3e}, accepted steps at tol 1e-4 mean "
          f"{z['iters4'].mean():.1f} max {int(z['iters4'].max())}, at the reference max {int(z['iters_ref'].max())}")


def test_fixture_reproduces_from_the_restatement():
    """On every drone of up to 10 segments: the start objective, the run at the GPU test's settings and both prefixes,
    with the bounds of tests/test_timeopt_states_cpu.py: a cost to 2e-9 (another LAPACK's rounding on coefficients good
    to 1e-9), a kept prefix run the same decisions and knots within prefix_sens, the full run held to the fixture's
    reference as the GPU test is, and lower than where it started."""
    z, cases = _fixture()
    delta = float(z["delta"])
    done = 0
    for c in cases:
        M = len(c["t"]) - 1
        if M > 10:
            continue
        k, nc, w, mf, kT = c["k"], c["order"] + 1, c["weights"], c["min_fraction"], c["time_weight"]
        Tmin = FR.floor_of(c["t"], mf)
        ts = FR.start_times(c["t"], Tmin)
        F0 = FR.evaluate(c["wp"], ts, w, kT, nc, c["start"], c["end"])[0]
        assert abs(F0 - float(z["F0"][k])) <= 2e-9 * F0, k
        r4 = FR.optimize(c["wp"], c["t"], c["start"], c["end"], w, kT, mf, 500, 1e-4, nc)
        assert r4["cost"] < F0 and (np.diff(r4["t_out"]) >= Tmin * (1 - 1e-12)).all() and r4["t_out"][0] == 0.0
        assert r4["t_out"][-1] <= F0 / kT
        if bool(z["conv4"][k]):
            assert r4["cost"] <= float(z["F_ref"][k]) * (1 + delta), (k, r4["cost"], float(z["F_ref"][k]))
        else:
            assert r4["cost"] <= float(z["F4"][k]) * (1 + 1e-6), (k, r4["cost"], float(z["F4"][k]))
        for j, mi in enumerate((1, 3)):
            if z["p_margin"][k, j] < 1e-3:
                continue
            r = FR.optimize(c["wp"], c["t"], c["start"], c["end"], w, kT, mf, mi, 1e-4, nc)
            assert r["iters"] == int(z["p_iters"][k, j]), (k, mi)
            assert np.abs(r["t_out"] - c["p_t"][j]).max() / c["t"][-1] <= float(z["prefix_sens"][k, j]), (k, mi)
        done += 1
    assert done >= 35


def test_the_raise_and_max_iter_zero():
    """Durations below the floor are raised to it, every other one is the input's bit for bit and the sum grows; an
    input with nothing below the floor comes back bit for bit; max_iter = 0 returns exactly that."""
    z, cases = _fixture()
    c = next(c for c in cases if c["kind"] == "below")
    Tmin = FR.floor_of(c["t"], c["min_fraction"])
    T = np.diff(c["t"])
    ts = FR.start_times(c["t"], Tmin)
    assert (T < Tmin).any() and ts[-1] > c["t"][-1]
    want = np.where(T < Tmin, Tmin, T)
    assert np.abs(np.diff(ts) - want).max() <= 4 * 2.0 ** -52 * ts[-1]       # (knots are running sums)
    r = FR.optimize(c["wp"], c["t"], c["start"], c["end"], c["weights"], c["time_weight"], c["min_fraction"], 0, 1e-4,
                    c["order"] + 1)
    assert np.array_equal(r["t_out"], ts) and r["iters"] == 0 and r["cost"] == r["cost0"]
    c = next(c for c in cases if c["kind"] == "walk")
    assert FR.start_times(c["t"], FR.floor_of(c["t"], 0.1)) is not c["t"]
    assert np.array_equal(FR.start_times(c["t"], FR.floor_of(c["t"], 0.1)), c["t"])


def test_the_entry_points_and_their_segment_range():
    from drone_path_planning_python_amd import Context, _lib, swarm
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in NEW[:2]:                                              # a null context: MSNAP_EINVAL
        assert getattr(lib, name)(None, 1, 3, p, p, 0, None, None, p, p, 0.1, 1, 1e-4, p, p, p, p, None, None,
                                  None) == -1
    for order in (7, 9):
        assert lib.msnap_optimize_times_free_max_segments(order) == MAX_SEG[order]
        assert lib.msnap_optimize_times_free_max_segments(order) == lib.msnap_optimize_times_states_max_segments(order)
    assert lib.msnap_optimize_times_free_max_segments(8) == -3        # MSNAP_EORDER
    for name in ("optimize_times_free", "optimize_times_free_device", "optimize_times_free_max_segments"):
        assert hasattr(Context, name), name
    assert hasattr(swarm.DeviceCompute, "optimize_times_free") and hasattr(swarm, "replan_within_limits")


@pytest.mark.parametrize("order", [7, 9])
def test_wrong_shapes_raise_before_the_library_is_asked(order):
    from drone_path_planning_python_amd import Context
    ctx = Context.__new__(Context)
    ctx.order, ctx.ncoef = order, order + 1
    nd = (order + 1) // 2 - 1
    wp, t = np.zeros((3, 5, 4)), np.arange(5.0)
    for kw in ({"start": np.zeros((3, 4, nd + 1))}, {"end": np.zeros((2, 4, nd))}):
        with pytest.raises(ValueError, match="must be"):
            ctx.optimize_times_free(wp, t, **kw)
    for kw in ({"time_weight": np.ones(2)}, {"time_weight": np.ones((3, 1))}, {"weights": (1, 1, 1)}):
        with pytest.raises(ValueError):
            ctx.optimize_times_free(wp, t, **kw)
    with pytest.raises(ValueError):
        ctx.optimize_times_free(wp, np.arange(4.0))


def test_the_exec_check_passes_on_the_object_with_the_new_kernels():
    """tools/check_exec_isa.py on msnap_timeopt_free.o: two kernels, no register-pressure copy at all (the order-9
    instance takes 235 VGPRs, no accumulation registers, no scratch), no loop the lanes leave one by one."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    obj = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_timeopt_free.o")
    assert chk.K17_OBJS == [obj]
    with open(os.path.join(ROOT, "tools", "check_exec_isa.py")) as f:
        assert len(re.findall(r"\+ K16_OBJS \+ K17_OBJS\b", f.read())) == 2      # checked and censused by default
    with open(os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "Makefile")) as f:
        assert "msnap_timeopt_free.hip" in f.read()
    if os.path.exists(obj) and os.path.exists(f"{chk.LLVM}/llvm-objdump"):      # (a machine that built the library)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), obj], capture_output=True,
                           text=True)
        assert r.returncode == 0 and "2 kernels, 0 register-pressure copies" in r.stdout, r.stdout + r.stderr
        assert chk.lane_latches(obj) == {}
