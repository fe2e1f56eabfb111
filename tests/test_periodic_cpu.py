"""Closed-loop paths on the CPU (include/msnap.h, "closed-loop paths"): the 60-digit reference of
tests/periodic_exact.py against a dense periodic collocation and against its own rotation, the NumPy model of the
kernel's recurrence (tests/periodic_ref.py) against the reference on every case the GPU tests solve, and the wiring of
the entry points."""
import ctypes
import os
import re
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_exact as PE  # noqa: E402
import periodic_ref as PR  # noqa: E402
from conftest import ROOT, norm_rel  # noqa: E402

MODEL_BAR = {7: 1e-11, 9: 1e-10}


def test_the_entry_points_are_declared_exported_and_bound():
    from drone_path_planning_python_amd import Context, _lib, swarm
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("msnap_solve_periodic", "msnap_solve_periodic_device", "msnap_solve_periodic_max_segments"):
        m = re.search(rf"\bint {name}\s*\(([^;]*)\)\s*;", text)
        assert m and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    for name in ("solve_periodic", "solve_periodic_device", "solve_periodic_max_segments"):
        assert hasattr(Context, name), name
    assert hasattr(swarm.DeviceCompute, "solve_periodic") and hasattr(swarm, "join_loop")


def test_the_segment_range_and_a_null_context():
    from drone_path_planning_python_amd import _lib
    lib = _lib.load()
    assert lib.msnap_solve_periodic_max_segments(7) == PE.MAX_SEG[7] >= 24
    assert lib.msnap_solve_periodic_max_segments(9) == PE.MAX_SEG[9] >= 16
    assert lib.msnap_solve_periodic_max_segments(8) == -3                                # MSNAP_EORDER
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("msnap_solve_periodic", "msnap_solve_periodic_device"):
        assert getattr(lib, name)(None, 1, 2, p, p, 0, p, p, p) == -1                    # MSNAP_EINVAL


def test_the_exec_check_covers_the_new_object_and_its_loops_are_wave_uniform():
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    obj = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_periodic.o")
    assert chk.K15_OBJS == [obj]
    with open(os.path.join(ROOT, "tools", "check_exec_isa.py")) as f:      # ... and a run without arguments checks it
        assert len(re.findall(r"\+ K13_OBJS \+ K15_OBJS\b", f.read())) == 2
    with open(os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\bmsnap_periodic\.hip\b", f.read(), flags=re.M)
    if os.path.exists(obj) and os.path.exists(f"{chk.LLVM}/llvm-objdump"):      # (a machine that built the library)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), obj], capture_output=True,
                           text=True)
        # (the order-9 kernel keeps values in accumulation registers: the copies are counted, none may sit under a
        # reduced exec mask)
        assert r.returncode == 0 and re.search(r"msnap_periodic\.o: 2 kernels, \d+ register-pressure copies, none under",
                                               r.stdout), r.stdout + r.stderr
        assert chk.lane_latches(obj) == {}


@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("M", [2, 3])
def test_the_superposition_is_the_dense_periodic_collocation(order, M):
    """the seam rows written like an interior knot's: 1e-40 relative, coefficient by coefficient"""
    K = (order + 1) // 2
    for kind in ("offset", "closed"):
        wp, t = PE.case(order, M, N=2, kind=kind)
        for d in range(2):
            X, _ = PE._solve_mp([mp.mpf(float(v)) for v in t[d]], wp[d], K)
            Y = PE.dense_periodic(t[d], wp[d], K)
            for a in range(4):
                scale = max(abs(v) for v in Y[a])
                assert max(abs(x - y) for x, y in zip(X[a], Y[a])) <= mp.mpf(10) ** -40 * scale, (kind, d, a)


@pytest.mark.parametrize("order", [7, 9])
def test_the_reference_started_one_knot_later_is_the_rotated_reference(order):
    K = (order + 1) // 2
    NC = 2 * K
    for M in (2, 3, 10):
        wp, t = PE.case(order, M, N=2)
        wp = np.round(wp * 2.0 ** 20) / 2.0 ** 20          # dyadic: the lap offset and the shifted waypoints are exact
        for d in range(2):
            X, _ = PE._solve_mp([mp.mpf(float(v)) for v in t[d]], wp[d], K)
            wp2, t2 = PE.rotate(wp[d], t[d], 1)
            # (the rotated knot times are sums of the same durations; both sides take the durations from their own
            # float64 times, so build the rotated times in mpf from the original ones)
            tm = [mp.mpf(float(v)) for v in t[d]]
            T = [tm[i + 1] - tm[i] for i in range(M)]
            T2 = T[1:] + T[:1]
            tm2 = [mp.mpf(0)]
            for v in T2:
                tm2.append(tm2[-1] + v)
            assert np.allclose([float(v) for v in tm2], t2, rtol=1e-15, atol=0)
            Y, _ = PE._solve_mp(tm2, wp2, K)
            lap = wp[d, M] - wp[d, 0]
            for a in range(4):
                scale = max(abs(v) for v in X[a])
                for s in range(M):
                    src = (s + 1) % M                      # segment s of the rotated loop is segment s+1 of the original
                    for q in range(NC):
                        want = X[a][NC * src + q] + (mp.mpf(float(lap[a])) if (q == 0 and s == M - 1) else 0)
                        assert abs(Y[a][NC * s + q] - want) <= mp.mpf(10) ** -40 * scale, (M, d, a, s, q)


@pytest.mark.parametrize("order", [7, 9])
def test_the_recurrence_model_agrees_with_the_reference_on_every_gpu_case(order):
    """If this fails the recurrence is wrong or ill-conditioned: to be resolved before any GPU run."""
    K = (order + 1) // 2
    worst = {}
    for M, kind in PE.gpu_cases(order):
        wp, t = PE.case(order, M, kind=kind)
        ref, seam = PE.reference(order, M, kind)
        got, u0 = PR.solve_batch(wp, t, K)
        worst[(M, kind)] = norm_rel(got, ref)
        assert np.abs(u0 - seam).max() <= 1e-8 * max(1.0, np.abs(seam).max()), (M, kind)
    print(f"order {order}: NumPy model vs 60 digits", worst)
    assert max(worst.values()) <= MODEL_BAR[order], worst


@pytest.mark.parametrize("order", [7, 9])
def test_the_periodic_optimum_is_the_boundary_state_solve_at_its_own_seam_state(order):
    """what the GPU tests use as their yardstick: states_exact.exact_solve given the optimum's seam state at both ends"""
    import states_exact as SE
    K = (order + 1) // 2
    wp, t = PE.case(order, 3, N=2)
    ref, seam = PE.exact_batch(wp, t, K)
    for d in range(2):
        got = SE.exact_solve(t[d], wp[d], [(seam[d], seam[d])], K)[0]
        assert norm_rel(got, ref[d]) <= 1e-13
