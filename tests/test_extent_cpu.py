"""Path extent on the CPU (include/msnap.h, "path extent"): the NumPy restatement of the kernel's walk
(tests/extent_exact.fp64_extent) against the exact reference on every family of tests/extent_cases.py, the hand-built
paths' known suprema, the motivating overshoot through the oracle, and the wiring of the entry points."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extent_cases as EC  # noqa: E402
import extent_exact as EE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _eval_flat(coef, dur, ts):
    """the restated msnap_eval_flat positions: [N, len(ts), 3]"""
    ts = np.asarray(ts, dtype=np.float64)
    return np.stack([EE._positions(coef, dur, np.full(len(ts), d), ts) for d in range(coef.shape[0])])


@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("name", sorted(EC.SWARMS))
def test_the_restatement_meets_the_contract_and_every_walk_closes(name, order):
    coef, dur, dirs = EC.swarm_case(name, order)
    st = {}
    EE.fp64_extent(coef, dur, dirs, stats=st)
    print(name, order, "nodes per lane: mean", st["nodes"].mean(), "max", st["nodes"].max())
    assert not st["capped"].any()
    EE.check_contract(EE.restated, _eval_flat, coef, dur, dirs, pick=EC.PICK.get(name))


@pytest.mark.parametrize("order", [7, 9])
def test_hand_built_paths(order):
    for T in (1.0, 3.0):
        coef, dur = EC.parabola(order, T)
        ext, t_ext, upper, _ = EE.check_contract(EE.restated, _eval_flat, coef, dur, EC.AXES[:2])
        if T == 1.0:
            assert ext[0, 0] == 0.25 and t_ext[0, 0] == 0.5
        assert abs(ext[0, 0] - 0.25) <= 1e-15 and abs(t_ext[0, 0] - T / 2) <= 1e-7 * T
        assert ext[0, 1] == 0.0 and t_ext[0, 1] == 0.0            # 0 at both ends: the earlier one
    for name in EC.HAND:
        coef, dur, dirs, S, t = EC.hand_case(name, order)
        ext, t_ext, upper, _ = EE.check_contract(EE.restated, _eval_flat, coef, dur, dirs)
        assert ext[0, 0] == S and t_ext[0, 0] == t, (name, ext, t_ext)
    coef, dur, dirs = EC.constant_path(order)
    ext, t_ext, upper, _ = EE.restated(coef, dur, dirs)
    want = EE.unfused_dot(dirs, coef[0, 0, :3, 0][None, :])
    assert np.array_equal(ext[0], want) and np.array_equal(upper[0], want) and (t_ext == 0.0).all()


@pytest.mark.parametrize("order", [7, 9])
def test_the_fit_through_waypoints_inside_the_workspace_leaves_it(order):
    wp, t = EC.overshoot_waypoints()
    assert ((wp[0, :, :3] >= EC.BOX_LO) & (wp[0, :, :3] <= EC.BOX_HI)).all()
    coef, dur = EC.solve(wp, t, order + 1)
    S, ts = EE.exact_extent(coef[0], dur[0], EC.AXES[0])
    # the dense scan's figures to their four decimals, and the two references against each other to 1e-9
    assert abs(float(S) - EC.OVERSHOOT_MAX_X[order]) < 5e-5 and abs(float(ts) - 3.0) < 1e-6
    ext, t_ext, upper = EE.fp64_extent(coef, dur, EC.AXES)
    assert abs(ext[0, 0] - float(S)) <= 1e-9 and abs(t_ext[0, 0] - 3.0) < 1e-6
    assert ext[0, 0] > EC.BOX_HI[0] + 1.0                     # more than a metre through the wall at x = 2.2
    dense = np.linspace(0.0, 6.0, 60001)
    scan = _eval_flat(coef, dur, dense)[0, :, 0]
    assert abs(scan.max() - float(S)) <= 1e-9


def test_zero_and_scaled_directions():
    coef, dur, dirs = EC.swarm_case("near_n5_m3_k7", 7)
    both = np.concatenate([dirs[6:7], 3.0 * dirs[6:7], np.zeros((1, 3))])
    ext, t_ext, upper = EE.fp64_extent(coef, dur, both)
    assert np.allclose(ext[:, 1], 3.0 * ext[:, 0], rtol=1e-12) and np.allclose(t_ext[:, 1], t_ext[:, 0], atol=1e-6)
    assert (ext[:, 2] == 0.0).all() and (upper[:, 2] == 0.0).all() and (t_ext[:, 2] == 0.0).all()


def test_the_entry_points_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    from drone_path_planning_python_amd import Context, _lib, swarm
    lib = _lib.load()
    for name in ("msnap_path_extent", "msnap_path_extent_device"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(Context, "path_extent") and hasattr(Context, "path_extent_device")
    assert hasattr(swarm.DeviceCompute, "path_extent") and hasattr(swarm, "certify_geofence")
    assert lib.msnap_version() == 500
    # the header's constant is the tests'
    m = re.search(r"C_ROUND_EXTENT = (\d+)", raw)
    assert m and float(m.group(1)) == EE.C_ROUND_EXTENT


def test_the_exec_check_covers_the_new_object_and_its_loops_are_wave_uniform():
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    obj = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_extent.o")
    assert obj in chk.K12_OBJS
    if os.path.exists(obj) and os.path.exists(f"{chk.LLVM}/llvm-objdump"):      # (a machine that built the library)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), obj], capture_output=True, text=True)
        assert r.returncode == 0 and "6 kernels, 0 register-pressure copies" in r.stdout, r.stdout + r.stderr
        assert chk.lane_latches(obj) == {}
