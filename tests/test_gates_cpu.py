"""Prescribed derivatives at interior waypoints on the CPU (include/msnap.h, "gates"): the exact
reference of tests/gates_exact.py against a dense QP, the NumPy restatement of the masked sweep against the exact
reference at the bar the GPU test holds the kernel to, and the wiring of the entry points."""
import ctypes
import inspect
import os
import re
import sys
from math import factorial

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gates_exact as GE  # noqa: E402
import gates_ref as GR  # noqa: E402
from conftest import ROOT, norm_rel  # noqa: E402

EXACT_BAR = 1e-10                   # the bar tests/test_states_gpu.py holds msnap_solve_states to


def _dense_qp(t, wp, start, end, fix, via):
    """Order 7: minimise sum_s int (p_s'''')^2 over monomial coefficients subject to interpolation, C1..C3 continuity
    at the interior knots, the end states and the gate rows -- one dense KKT solve for the four axes."""
    K, NC = 4, 8
    T = np.diff(t)
    M = len(T)
    n = NC * M

    def drow(j, x):
        r = np.zeros(NC)
        for k in range(j, NC):
            r[k] = factorial(k) / factorial(k - j) * x ** (k - j)
        return r

    H = np.zeros((n, n))
    for s in range(M):
        for j in range(K, NC):
            for k in range(K, NC):
                cj, ck = factorial(j) / factorial(j - K), factorial(k) / factorial(k - K)
                H[NC * s + j, NC * s + k] = 2 * cj * ck * T[s] ** (j + k - 2 * K + 1) / (j + k - 2 * K + 1)
    A, b = [], []

    def add(s, row, val, s2=None, row2=None):
        r = np.zeros(n)
        r[NC * s:NC * (s + 1)] = row
        if s2 is not None:
            r[NC * s2:NC * (s2 + 1)] = row2
        A.append(r)
        b.append(val)

    for s in range(M):
        add(s, drow(0, 0.0), wp[s])
        add(s, drow(0, T[s]), wp[s + 1])
    for q in range(1, K):
        add(0, drow(q, 0.0), start[:, q - 1])
        add(M - 1, drow(q, T[M - 1]), end[:, q - 1])
    for i in range(1, M):
        for q in range(1, K):
            add(i - 1, drow(q, T[i - 1]), np.zeros(4), i, -drow(q, 0.0))
            if (int(fix[i - 1]) >> (q - 1)) & 1:
                add(i, drow(q, 0.0), via[i - 1, :, q - 1])
    A, b = np.array(A), np.array(b)
    m = A.shape[0]
    kkt = np.block([[H, A.T], [A, np.zeros((m, m))]])
    sol = np.linalg.solve(kkt, np.vstack([np.zeros((n, 4)), b]))
    return np.ascontiguousarray(sol[:n].T.reshape(4, M, NC).transpose(1, 0, 2))


@pytest.mark.parametrize("M", [3, 4])
def test_the_exact_solve_agrees_with_a_dense_qp(M):
    """Catches a wrong pairing of a prescribed derivative with the continuity row it replaces, which is off by O(1)."""
    wp, t, start, end, fix, via = GE.case(7, M)
    worst = 0.0
    for d in range(8):               # knot 1 of drones 0..7 carries every mask value of order 7
        exact = GE.exact_solve(t[d], wp[d], start[d], end[d], fix[d], via[d], 4)
        dense = _dense_qp(t[d], wp[d], start[d], end[d], fix[d], via[d])
        worst = max(worst, norm_rel(dense[None], exact[None]))
    print(f"order 7 M {M}: dense KKT vs 60 digits", worst)
    assert worst <= 1e-6, worst


def test_the_cases_hold_what_the_tests_rely_on():
    for order in (7, 9):
        K = (order + 1) // 2
        for M in GE.GPU_SEGMENTS[order]:
            wp, t, start, end, fix, via = GE.case(order, M)
            tile = fix[:16]
            assert set(tile[:, 0].tolist()) == set(range(2 ** (K - 1)))            # every mask value, at knot 1
            assert (tile[:, -1] != 0).any()                                        # gates at knot M-1
            if M >= 3:
                assert ((tile[:, 0] != 0) & (tile[:, 1] != 0)).any()               # and at two adjacent knots
            assert len({(fix[d].tobytes(), via[d].tobytes()) for d in range(16)}) == 16
            used = ((fix[:, :, None] >> np.arange(K - 1)) & 1).astype(bool)
            assert np.isfinite(via[np.broadcast_to(used[:, :, None, :], via.shape)]).all()
            assert np.isnan(via[~np.broadcast_to(used[:, :, None, :], via.shape)]).all()
            assert (np.nan_to_num(np.abs(via)) <= np.array(GE.SE.STATE_SCALE[:K - 1])).all()


@pytest.mark.parametrize("order", [7, 9])
def test_the_restatement_reaches_the_bar_of_the_gpu_test(order):
    """Every (order, M) of tests/test_gates_gpu.py: the float64 masked sweep against the 60-digit reference at
    EXACT_BAR -- the bar is reachable in float64 before the kernel is held to it."""
    K = (order + 1) // 2
    errs = {}
    for M in GE.GPU_SEGMENTS[order]:
        wp, t, start, end, fix, via = GE.case(order, M)
        errs[M] = norm_rel(GR.solve_batch(wp, t, start, end, fix, via, K), GE.reference(order, M))
    print(f"order {order}: restatement vs 60 digits", errs)
    assert max(errs.values()) <= EXACT_BAR, errs


def test_an_empty_mask_and_a_full_mask():
    """No gates: states_exact's solution.  Every derivative prescribed at a knot: the two halves decouple."""
    from states_exact import exact_solve as states_exact_solve
    wp, t, start, end, fix, via = GE.case(7, 4)
    d = 3
    none = GR.solve(wp[d], t[d], start[d], end[d], np.zeros(3, dtype=int), np.full((3, 4, 3), np.nan), 4)
    want = states_exact_solve(t[d], wp[d], [(start[d], end[d])], 4)[0]
    assert norm_rel(none[None], want[None]) <= EXACT_BAR
    g = 2
    f = np.array([0, 7, 0])
    v = np.full((3, 4, 3), np.nan)
    v[g - 1] = 0.25 * np.arange(12).reshape(4, 3) - 1.0
    left = states_exact_solve(t[d, :g + 1], wp[d, :g + 1], [(start[d], v[g - 1])], 4)[0]
    tr = np.concatenate([[0.0], t[d, g + 1:] - t[d, g]])
    right = states_exact_solve(tr, wp[d, g:], [(v[g - 1], end[d])], 4)[0]
    halves = np.concatenate([left, right])[None]
    # (the right half's times are rounded differences: the bar is the rounding of a time, not the solve's)
    assert norm_rel(GE.exact_solve(t[d], wp[d], start[d], end[d], f, v, 4)[None], halves) <= 1e-13
    assert norm_rel(GR.solve(wp[d], t[d], start[d], end[d], f, v, 4)[None], halves) <= EXACT_BAR


def test_the_entry_points_refuse_a_null_context_and_report_their_segment_range():
    from drone_path_planning_python_amd import Context, _lib, swarm
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("msnap_solve_gates", "msnap_solve_gates_device"):
        assert getattr(lib, name)(None, 1, 1, p, p, 0, None, None, None, None, p, p, p) == -1      # MSNAP_EINVAL
    for order in (7, 9):
        cap = lib.msnap_solve_gates_max_segments(order)
        assert cap >= 20 and cap == GE.MAX_SEG[order]
    assert lib.msnap_solve_gates_max_segments(8) == -3                                   # MSNAP_EORDER
    for name in ("solve_gates", "solve_gates_device", "solve_gates_max_segments"):
        assert hasattr(Context, name), name
    assert hasattr(swarm.DeviceCompute, "solve_gates")
    assert list(inspect.signature(swarm.DeviceCompute.solve_gates).parameters)[1:] == ["wp", "t", "start", "end", "fix",
                                                                                      "via"]
    assert inspect.signature(swarm.replan).parameters["gates"].default is None
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("msnap_solve_gates", "msnap_solve_gates_device", "msnap_solve_gates_max_segments"):
        m = re.search(rf"\bint {name}\s*\(([^)]*)\)", text)
        assert m and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_replan_refuses_gates_together_with_optimize():
    from drone_path_planning_python_amd import swarm
    with pytest.raises(ValueError, match="gates"):
        swarm.replan(None, None, None, 0.0, None, None, optimize={}, gates=(None, None))


def test_the_exec_check_covers_the_new_object_and_its_loops_are_wave_uniform():
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    obj = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_gates.o")
    assert chk.K21_OBJS == [obj]
    if os.path.exists(obj) and os.path.exists(f"{chk.LLVM}/llvm-objdump"):      # (a machine that built the library)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), obj], capture_output=True,
                           text=True)
        assert r.returncode == 0 and "2 kernels, 0 register-pressure copies" in r.stdout, r.stdout + r.stderr
        assert chk.lane_latches(obj) == {}
