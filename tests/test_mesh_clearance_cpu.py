"""Mesh clearance without a GPU: the NumPy restatement of the kernel's method against the exact reference
(tests/mesh_clearance_exact.py; D of the contract cases from tests/golden/mesh_clearance_golden.npz), the allowance's
coordinate term, and the entry point's presence in the header, the library and the bindings."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clearance_cases as MC  # noqa: E402
import mesh_clearance_exact as ME  # noqa: E402


def _restated(coef, dur, tris):
    md, tm, tri, lower = ME.fp64_mesh_clearance(coef, dur, tris)
    return md, tm, tri, lower, np.zeros(len(md), dtype=np.int32)


@pytest.mark.parametrize("name", sorted(MC.CONTRACT))
def test_restatement_against_the_exact_reference(name):
    coef, dur, tris = MC.contract_case(name)
    ME.check_contract(_restated, coef, dur, tris, exact=MC.golden()[name])


def test_the_recorded_reference_is_what_the_exact_reference_gives():
    coef, dur, tris = MC.contract_case("o7_m1_one")
    _, tm, _, _ = ME.fp64_mesh_clearance(coef, dur, tris)
    for d in range(2):
        D, _ = ME.exact_mesh_clearance(coef[d], dur[d], tris, hint_t=[float(tm[d])])
        assert float(D) == MC.golden()["o7_m1_one"][d]


def test_the_tunnelling_drone_on_the_restatement():
    coef, dur = MC.tunnelling()
    wall = np.array([[[0.0, -2.0, -2.0], [0.0, 3.0, -2.0], [0.0, 0.0, 3.0]]])
    st = {}
    md, tm, tri, lower = ME.fp64_mesh_clearance(coef, dur, wall, stats=st)
    assert md[0] <= 1e-9 and lower[0] <= md[0] and abs(tm[0] - 0.55) < 1e-6 and not st["capped"].any()
    D, _ = ME.exact_mesh_clearance(coef[0], dur[0], wall, hint_t=[float(tm[0])])
    assert float(D) < 1e-30


def test_the_allowance_without_its_coordinate_term_fails_far_from_the_origin():
    off = 1e5
    coef, dur, wall = MC.contract_case("o7_m2_one")
    coef = coef[:1].copy()
    coef[:, :, :3, 0] += off
    dur, wall = dur[:1], wall + off
    md, tm, tri, lower = ME.fp64_mesh_clearance(coef, dur, wall)
    D, _ = ME.exact_mesh_clearance(coef[0], dur[0], wall, hint_t=[float(tm[0])])
    R = ME.mesh_R(coef[0], dur[0], wall)
    att = ME.exact_distance_at(coef[0], dur[0], wall, float(tm[0]))
    print("md", md[0], "lower", lower[0], "D", float(D), "R", R, "ratio", ME.round_ratio(md[0], lower[0], D, R, att))
    assert not ME.contract_violations(md[0], lower[0], D, R=R)
    # an ulp of 1e5 m is 1.5e-11 m: the position at t_min carries it, the terms that scale with the distance do not
    assert abs(md[0] - float(att)) > ME.REL_ROUND * float(att) + ME.ABS_ROUND
    assert ME.round_ratio(md[0], lower[0], D, R, att) < ME.C_ROUND_MESH


def test_the_entry_point_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    from drone_path_planning_python_amd import Context, _lib
    lib = _lib.load()
    for name in ("msnap_mesh_clearance", "msnap_mesh_clearance_device"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(Context, "mesh_clearance") and hasattr(Context, "mesh_clearance_device")
    from drone_path_planning_python_amd import swarm
    assert hasattr(swarm.DeviceCompute, "mesh_clearance") and hasattr(swarm, "certify_mesh_clearance")


def test_the_exec_check_covers_the_new_object_and_its_loops_are_wave_uniform():
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    obj = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_mesh_clearance.o")
    assert obj in chk.K11_OBJS
    if not os.path.exists(obj) or not os.path.exists(f"{chk.LLVM}/llvm-objdump"):
        pytest.skip("no object file / ROCm LLVM tools here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), obj], capture_output=True, text=True)
    assert r.returncode == 0 and "none under a reduced exec mask" in r.stdout, r.stdout + r.stderr
    assert chk.lane_latches(obj) == {}
