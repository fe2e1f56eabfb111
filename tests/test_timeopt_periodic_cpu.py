"""Time allocation on closed loops without a GPU: the closed-form gradient on the ring against central differences of
the solved cost, the fixture's own conditions and that the cost falls on every one of its drones, rotation of the cut,
the fixture's reproduction from the restatement, the wiring of the entry points, and the exec check on the object
that holds the new kernels."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_exact as PE  # noqa: E402
import timeopt_periodic_ref as PR  # noqa: E402
import timeopt_ref as R  # noqa: E402
from conftest import GOLDEN_DIR, ROOT  # noqa: E402

NEW = ["msnap_optimize_times_periodic", "msnap_optimize_times_periodic_device",
       "msnap_optimize_times_periodic_max_segments"]
FIRST_TD8 = {7: 25, 9: 18}          # the first segment count that runs as 8-drone tiles
MAX_SEG = {7: 48, 9: 33}
KINDS = {"walk", "tile8", "cap", "shared", "floor", "weights", "curve", "polygon"}


@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("M", [2, 3, 5, 10])
def test_closed_form_gradient_against_central_differences(order, M):
    """dJ*/dT_i = -sum_a w_a E_i,a with the period free, on every segment of the ring: the seam state is a stationary
    unknown like every interior knot.  Random loops with a nonzero lap offset on every axis; the difference step is 1e-5
    of the duration.  Measured on these cases: within 3.0e-9 (order 7) and 1.5e-7 (order 9) of the largest component."""
    wp, t = PE.case(order, M, N=1)
    wp, t = wp[0], t[0]
    assert (wp[M] != wp[0]).all()
    w = (2.0, 0.5, 1.0, 3.0)
    J, g, _ = PR.evaluate(wp, t, w, order + 1)
    T = np.diff(t)
    worst = 0.0
    for i in range(M):
        h = 1e-5 * T[i]
        Jpm = []
        for sgn in (+1, -1):
            T2 = T.copy()
            T2[i] += sgn * h
            Jpm.append(PR.evaluate(wp, np.concatenate([[0.0], np.cumsum(T2)]), w, order + 1)[0])
        fd = (Jpm[0] - Jpm[1]) / (2 * h)
        worst = max(worst, abs(fd - g[i]) / np.abs(g).max())
        assert abs(fd - g[i]) <= 1e-6 * np.abs(g).max(), (i, fd, g[i])
    print(f"order {order} M {M}: central differences within {worst:.2e} of the largest component")


def _fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "timeopt_periodic_golden.npz"))
    return z, PR.unpack_cases(z)


def _delta(z):
    return max(100.0 * float(z["gap4"][z["conv4"]].max()), 1e-9)


def test_fixture_invariants_and_the_cost_falls_on_every_drone():
    path = os.path.join(GOLDEN_DIR, "timeopt_periodic_golden.npz")
    assert os.path.getsize(path) < 200 * 1024
    z, cases = _fixture()
    n = int(z["n"])
    assert 55 <= n <= 70
    seg = np.diff(z["off"]) - 1
    order = z["order"][z["group"]]
    kind = z["kind"][z["group"]]
    assert set(kind.tolist()) == KINDS
    for o in (7, 9):
        have = set(seg[order == o].tolist())
        assert {2, 3, 10, FIRST_TD8[o], PE.MAX_SEG[o]} <= have, (o, have)
        assert max(np.bincount(z["group"][(order == o) & (seg == FIRST_TD8[o])])) == 11      # a full tile and a tail of 3
    for c in cases:
        t = c["t"]
        assert t[0] == 0.0 and (np.diff(t) > 0).all() and c["wp"].shape == (len(t), 4)
        lap = c["wp"][-1] - c["wp"][0]
        if c["kind"] in ("curve", "polygon"):
            assert (lap[:3] == 0).all() and abs(lap[3] - 2.0 * np.pi) < 1e-6, (c["k"], lap)
        else:
            assert (lap != 0).all(), (c["k"], lap)
    # the cost falls on every drone, at the reference and at the GPU test's settings
    assert (z["J_ref"] < z["J0"]).all() and (z["J4"] < z["J0"]).all()
    assert (z["gap4"] >= -1e-12).all() and z["gap4"][z["conv4"]].max() < 1e-6
    assert np.array_equal(z["J_ref"], np.minimum(z["J_slsqp"], z["J_descent"]))
    assert (np.abs(z["J_slsqp"] - z["J_descent"]) <= 1e-6 * z["J_ref"]).sum() >= 0.8 * n
    assert z["shared"].sum() == 1 and (np.asarray(z["weights"]) != 1.0).any(axis=1).sum() == 1
    floor = kind == "floor"
    assert floor.sum() == 3 and (z["min_fraction"][z["group"]][floor] == 0.5).all()
    assert (z["active"][floor] > 0).any() and (z["n_below"][floor] > 0).all()
    # what the generator drew its inputs for
    assert (~z["conv4"]).sum() <= 0.1 * n
    left_out = z["p_margin"] < 1e-3
    assert left_out.sum() <= 0.1 * 2 * n
    assert np.isfinite(z["prefix_sens"][~left_out]).all() and (z["prefix_sens"][~left_out] > 0).all()
    poly = kind == "polygon"
    assert poly.sum() == 8 and z["conv4"][poly].all() and set(seg[poly].tolist()) == {3, 6}
    assert (np.abs(z["J4"][poly] / z["J_even"][poly] - 1.0) <= 1e-9).all()
    print(f"fixture: {n} drones, {int((~z['conv4']).sum())} unconverged at tol 1e-4, {int(left_out.sum())} prefix runs "
          f"left out, delta {_delta(z):.3e}, polygons within {np.abs(z['J4'][poly] / z['J_even'][poly] - 1).max():.2e} of "
          f"J(even) and {z['t_even_err'][poly].max():.2e} s of the even grid")


def test_fixture_reproduces_from_the_restatement():
    """On the drones of up to 6 segments: the start cost, the run at the GPU test's settings and both prefixes, with
    the bounds of tests/test_timeopt_states_cpu.py: a cost to 2e-9 (another LAPACK's rounding on coefficients good to
    1e-9), a kept prefix run the same decisions and knots within prefix_sens, the full run held to the fixture's
    reference as the GPU test is."""
    z, cases = _fixture()
    delta = _delta(z)
    done = 0
    for c in cases:
        M = len(c["t"]) - 1
        if M > 6:
            continue
        k, nc, w, mf = c["k"], c["order"] + 1, c["weights"], c["min_fraction"]
        ts = R.start_times(c["t"], R.floor_of(c["t"], mf))
        J0 = PR.cost(PR.solve(c["wp"], ts, nc // 2), np.diff(ts), w)
        assert abs(J0 - float(z["J0"][k])) <= 2e-9 * J0, k
        r4 = PR.optimize(c["wp"], c["t"], w, mf, 500, 1e-4, nc)
        J4 = PR.cost(PR.solve(c["wp"], r4["t_out"], nc // 2), np.diff(r4["t_out"]), w)
        assert bool(z["conv4"][k]) and J4 <= float(z["J_ref"][k]) * (1 + delta), (k, J4, float(z["J_ref"][k]))
        assert J4 <= J0 and (np.diff(r4["t_out"]) >= R.floor_of(c["t"], mf) * (1 - 1e-12)).all()
        assert r4["t_out"][0] == 0.0 and r4["t_out"][-1] == c["t"][-1]
        for j, mi in enumerate((1, 3)):
            if z["p_margin"][k, j] < 1e-3:
                continue
            r = PR.optimize(c["wp"], c["t"], w, mf, mi, 1e-4, nc)
            assert r["iters"] == int(z["p_iters"][k, j]), (k, mi)
            assert np.abs(r["t_out"] - c["p_t"][j]).max() / c["t"][-1] <= float(z["prefix_sens"][k, j]), (k, mi)
        done += 1
    assert done >= 20


@pytest.mark.parametrize("order", [7, 9])
def test_where_the_loop_is_cut_does_not_matter(order):
    """The iteration on the same loop started at knots 0, 1 and M-1 ends at the same cost within the fixture's delta
    (measured: 3e-12 relative)."""
    z, cases = _fixture()
    delta = _delta(z)
    c = min((c for c in cases if c["order"] == order and c["kind"] == "walk" and len(c["t"]) == 4),
            key=lambda c: int(z["iters4"][c["k"]]))
    M = len(c["t"]) - 1
    costs = []
    for j in (0, 1, M - 1):
        wp, t = PE.rotate(c["wp"], c["t"], j)
        r = PR.optimize(wp, t, c["weights"], c["min_fraction"], 500, 1e-4, order + 1)
        costs.append(PR.cost(PR.solve(wp, r["t_out"], (order + 1) // 2), np.diff(r["t_out"]), c["weights"]))
    spread = (max(costs) - min(costs)) / min(costs)
    print(f"order {order}: three cuts of a {M}-segment loop agree within {spread:.2e} (delta {delta:.2e})")
    assert spread <= delta


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
        assert getattr(lib, name)(None, 1, 3, p, p, 0, p, 0.1, 1, 1e-4, p, p, p, p, None, None, None) == -1
    for order in (7, 9):
        assert lib.msnap_optimize_times_periodic_max_segments(order) == MAX_SEG[order]
        assert MAX_SEG[order] >= lib.msnap_solve_periodic_max_segments(order)
    assert lib.msnap_optimize_times_periodic_max_segments(5) == -3    # MSNAP_EORDER
    for name in ("optimize_times_periodic", "optimize_times_periodic_device", "optimize_times_periodic_max_segments"):
        assert hasattr(Context, name), name
    assert hasattr(swarm.DeviceCompute, "optimize_times_periodic")


def test_wrong_shapes_raise_before_the_library_is_asked():
    from drone_path_planning_python_amd import Context
    ctx = Context.__new__(Context)
    ctx.order, ctx.ncoef = 7, 8
    wp, t = np.zeros((3, 5, 4)), np.arange(5.0)
    with pytest.raises(ValueError):
        ctx.optimize_times_periodic(wp, np.arange(4.0))
    with pytest.raises(ValueError):
        ctx.optimize_times_periodic(wp[:, :, :3], t)
    with pytest.raises(ValueError):
        ctx.optimize_times_periodic(wp, t, weights=(1, 1, 1))


def test_the_exec_check_passes_on_the_object_with_the_new_kernels():
    """tools/check_exec_isa.py on msnap_timeopt_periodic.o: the two ring instances keep values in accumulation
    registers (the order-9 one fills the 256 VGPRs), so the check has something to look at: no such copy under a reduced
    exec mask, and no loop the lanes leave one by one."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    obj = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_timeopt_periodic.o")
    assert chk.K16_OBJS == [obj]
    with open(os.path.join(ROOT, "tools", "check_exec_isa.py")) as f:
        assert len(re.findall(r"\+ K15_OBJS \+ K16_OBJS\b", f.read())) == 2      # checked and censused by default
    if os.path.exists(obj) and os.path.exists(f"{chk.LLVM}/llvm-objdump"):      # (a machine that built the library)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), obj], capture_output=True,
                           text=True)
        assert r.returncode == 0 and re.search(r"2 kernels, \d+ register-pressure copies, none under", r.stdout), \
            r.stdout + r.stderr
        assert chk.lane_latches(obj) == {}
