"""Replanning in flight on the CPU (include/msnap.h, "replanning in flight"): the exact reference of
tests/states_exact.py against the committed solutions and a closed form, the NumPy restatement of msnap_eval_state
against mpmath, and the wiring of the entry points."""
import ctypes
import os
import re
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import states_exact as SE  # noqa: E402
from conftest import GOLDEN_DIR, ROOT, norm_rel  # noqa: E402


@pytest.mark.parametrize("order,name", [(7, "m2"), (7, "m3"), (7, "cfg2"), (7, "m20"), (9, "m2"), (9, "m3"), (9, "m10"),
                                        (9, "m20")])
def test_zero_states_reproduce_the_committed_solutions(order, name):
    g = np.load(os.path.join(GOLDEN_DIR, "ref_golden.npz" if order == 7 else "order9_golden.npz"))
    wp, t, ref = g[name + "_wp"], g[name + "_t"], g[name + "_coef"]
    K = (order + 1) // 2
    if wp.ndim == 2:                  # a single trajectory
        wp, ref = wp[None], ref[None]
    for d in range(min(2, wp.shape[0])):
        tt = t if t.ndim == 1 else t[d]
        assert tt[0] == 0.0
        zeros = np.zeros((4, K - 1))
        rest, explicit = SE.exact_solve(tt, wp[d], [(None, None), (zeros, zeros)], K)
        assert np.array_equal(rest, explicit)
        err = norm_rel(rest, ref[d])
        print(order, name, d, err)
        assert err <= 1e-11, err


@pytest.mark.parametrize("order", [7, 9])
def test_one_segment_is_the_two_point_hermite_polynomial(order):
    K = (order + 1) // 2
    wp, t, start, end = SE.case(order, 1)
    for d in range(4):
        got = SE.exact_solve(t[d], wp[d], [(start[d], end[d])], K)[0]
        for a in range(4):
            want = SE.hermite_two_point(t[d, 1], wp[d, 0, a], wp[d, 1, a], start[d, a], end[d, a], K)
            want = np.array([float(v) for v in want])
            assert np.abs(got[0, a] - want).max() <= 1e-15 * np.abs(want).max(), (d, a)
            # and the closed form has the given end data
            for q in range(1, K):
                assert abs(SE.falling(q, q) * want[q] - start[d, a, q - 1]) <= 1e-15 * max(1.0, abs(start[d, a, q - 1]))


@pytest.mark.parametrize("order", [7, 9])
def test_the_eval_restatement_agrees_with_mpmath(order):
    """4 ulp of sum_j |d_j| t^j, d the coefficients of the derivative being evaluated"""
    K = (order + 1) // 2
    rng = np.random.default_rng(77 + order)
    N, M = 6, 4
    coef = rng.uniform(-3.0, 3.0, (N, M, 4, 2 * K))
    dur = rng.uniform(0.5, 2.0, (N, M))
    ends = np.zeros((N, M + 1))
    for i in range(M):
        ends[:, i + 1] = ends[:, i] + dur[:, i]           # the running sums of the lookup
    tq = np.array([0.0, ends[1, 2], ends[2, M], 0.37 * ends[3, M], 0.81 * ends[4, M], ends[5, 1] * (1 + 2.0 ** -40)])
    pos, deriv = SE.eval_state_np(coef, dur, tq)
    for d in range(N):
        seg = next(i for i in range(M) if tq[d] <= ends[d, i] + dur[d, i])
        if d == 1:
            assert seg == 1              # a knot belongs to the earlier segment
        tl = tq[d] - ends[d, seg]
        for a in range(4):
            for q in range(K):
                got = pos[d, a] if q == 0 else deriv[d, a, q - 1]
                want = SE.eval_state_mp(coef[d, seg, a], tl, q)
                scale = sum(SE.falling(j, q) * abs(coef[d, seg, a, j]) * tl ** (j - q) for j in range(q, 2 * K))
                assert abs(mp.mpf(float(got)) - want) <= 4 * 2.0 ** -52 * scale, (d, a, q)
    out = SE.eval_state_np(coef, dur, np.array([-1e-9, ends[1, M] * (1 + 1e-15), np.nan, 0.0, 0.0, 0.0]))
    assert np.isnan(out[0][:3]).all() and np.isnan(out[1][:3]).all() and np.isfinite(out[0][3:]).all()


def test_the_entry_points_refuse_a_null_context_and_report_their_segment_range():
    from drone_path_planning_python_amd import Context, _lib, swarm
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("msnap_solve_states", "msnap_solve_states_device"):
        assert getattr(lib, name)(None, 1, 1, p, p, 0, None, None, p, p, p) == -1      # MSNAP_EINVAL
    for name in ("msnap_eval_state", "msnap_eval_state_device"):
        assert getattr(lib, name)(None, 1, 1, p, p, p, p, p) == -1
    for order in (7, 9):
        cap = lib.msnap_solve_states_max_segments(order)
        assert cap >= 20 and cap == SE.MAX_SEG[order]
    assert lib.msnap_solve_states_max_segments(8) == -3                                  # MSNAP_EORDER
    for name in ("solve_states", "solve_states_device", "eval_state", "eval_state_device"):
        assert hasattr(Context, name), name
    assert hasattr(swarm.DeviceCompute, "solve_states") and hasattr(swarm.DeviceCompute, "eval_state")
    assert hasattr(swarm, "replan")
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("msnap_solve_states", "msnap_solve_states_device", "msnap_solve_states_max_segments",
                 "msnap_eval_state", "msnap_eval_state_device"):
        assert re.search(rf"\bint {name}\s*\(", text) and name in _lib.SIGNATURES, name


def test_the_exec_check_covers_the_new_object_and_its_loops_are_wave_uniform():
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    obj = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_states.o")
    assert obj in chk.K13_OBJS
    if os.path.exists(obj) and os.path.exists(f"{chk.LLVM}/llvm-objdump"):      # (a machine that built the library)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), obj], capture_output=True,
                           text=True)
        assert r.returncode == 0 and "4 kernels, 0 register-pressure copies" in r.stdout, r.stdout + r.stderr
        assert chk.lane_latches(obj) == {}
