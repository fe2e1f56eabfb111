"""Mesh conflict windows without a GPU (include/msnap.h, "mesh conflict windows"): the proof that every
fixture of the closing checks is transversal, the NumPy restatement of the lane and fold rules against the exact
reference (tests/mesh_conflict_exact.py) on the cases of tests/mesh_conflict_cases.py, swarm.mesh_conflict_windows /
latest_replan_time with a stand-in compute object, the declarations and bindings of the new entries, the argument checks
of the C entries that need no GPU, and the build checks on the kernels' object."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clearance_cases as MC  # noqa: E402
import mesh_clearance_exact as ME  # noqa: E402
import mesh_conflict_cases as KC  # noqa: E402
import mesh_conflict_exact as MX  # noqa: E402

OBJ = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_mesh_conflict.o")
LLVM = "/opt/rocm/lib/llvm/bin"
ENTRIES = ("msnap_mesh_conflict_window", "msnap_mesh_conflict_window_device")


def test_the_entries_are_declared_exported_and_bound():
    from drone_path_planning_python_amd import Context, _lib, swarm
    header = open(os.path.join(ROOT, "include", "msnap.h")).read()
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(msnap_ctx \*ctx,", header, re.M), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 18
        assert hasattr(_lib.load(), name)
    assert callable(Context.mesh_conflict_window) and callable(Context.mesh_conflict_window_device)
    assert callable(swarm.DeviceCompute.mesh_conflict_window) and callable(swarm.mesh_conflict_windows)
    assert "first_conflict" in swarm.MeshConflictWindowResult.__dataclass_fields__
    assert _lib.load().msnap_version() == 500


@pytest.mark.parametrize("name", sorted(KC.CLOSING))
def test_every_fixture_of_the_closing_checks_is_transversal(name):
    """Every entry and exit at >= 1e-3 m/s, no touch, no exact infimum within 1e-6 m of the threshold: no flight of
    these fixtures is a graze, and none is excluded from the closing checks."""
    groups, exact = KC.fixture(name)
    assert len(groups) == len(exact) and groups
    for g, exs in zip(groups, exact):
        assert len(exs) == len(g[1])
        for ex in exs:
            ex.assert_transversal()


def test_the_exact_entry_of_the_wall_flight_is_the_root_of_the_step_polynomial():
    ex = KC.fixture("wall_o7")[1][0][0]
    (t_in, t_out), = ex.ranges
    assert abs(float(t_in) - 0.534448773) < 1e-9                         # s(x) = 0.575
    assert abs(float(MX.step(8, t_in)) - 0.575) < 1e-15 and abs(float(MX.step(8, t_out)) - 0.675) < 1e-15


@pytest.mark.parametrize("nc", [8, 10])
def test_restatement_wall(nc):
    KC.check_wall(MX.RestatedContext(nc - 1), nc)


def test_restatement_real_scene():
    KC.check_hole(MX.RestatedContext(7))


@pytest.mark.parametrize("name", KC.FEATURE_LINES)
def test_restatement_closest_features(name):
    KC.check_features(MX.RestatedContext(int(name[1])), name)


def test_restatement_conflict_across_a_knot():
    KC.check_knot(MX.RestatedContext(7))


def test_restatement_in_conflict_at_both_ends():
    KC.check_both_ends(MX.RestatedContext(7))


def test_restatement_two_conflicts():
    KC.check_two_conflicts(MX.RestatedContext(7))


def test_restatement_far_from_the_origin():
    KC.check_far(MX.RestatedContext(7))


def test_restatement_nan_duplicate_and_degenerate_triangles():
    KC.check_odd_mesh(MX.RestatedContext(7))


def test_restatement_closing_gap_follows_t_res():
    KC.check_t_res(MX.RestatedContext(7))


def test_restatement_verdict_cases():
    ctx = MX.RestatedContext(7)
    KC.check_never_close(ctx)
    KC.check_tangent(ctx)
    KC.check_threshold_zero(ctx)
    KC.check_no_triangles(ctx)


@pytest.mark.parametrize("name", sorted(KC.CURVED))
def test_restatement_curved_paths(name):
    KC.check_curved(MX.RestatedContext(KC.curved(name)[0].shape[3] - 1), name)


def test_restatement_identities():
    KC.check_identities(MX.RestatedContext(7))


def test_node_counts_of_the_issues_trial():
    """The restatement's forward walk on the wall flight: 29 nodes at order 7, 41 at t_res 1e-9, 32 at order 9; the
    real scene's flight closes in 31."""
    for nc, t_res, want in ((8, 1e-6, 29), (8, 1e-9, 41), (10, 1e-6, 32)):
        g = KC.wall(nc)[0]
        coef, dur = KC.paths(g)
        stats = {}
        MX.fp64_mesh_conflict_window(coef, dur, g[3], g[4], t_res, stats)
        assert stats["nodes"][0, 0] == want
    g = KC.hole_scene()[0]
    coef, dur = KC.paths(g)
    stats = {}
    MX.fp64_mesh_conflict_window(coef, dur, g[3], g[4], 1e-6, stats)
    assert stats["nodes"][:, 0].tolist() == [31, 1, 1]


class _Compute:
    """DeviceCompute's mesh conflict-window method on CPU tensors through the restatement."""

    def mesh_conflict_window(self, coef, dur, tris, threshold, t_res=1e-6):
        import torch
        out = MX.fp64_mesh_conflict_window(coef.numpy(), dur.numpy(), tris.numpy(), threshold, t_res)
        return tuple(torch.from_numpy(x) for x in out + (np.zeros(len(out[0]), dtype=np.int32),))


class _Failing(_Compute):
    def mesh_conflict_window(self, *a, **k):
        out = list(super().mesh_conflict_window(*a, **k))
        out[8][0] = 2
        return tuple(out)


def test_swarm_mesh_conflict_windows_and_latest_replan_time_with_a_stand_in():
    """certify_case: the drones whose certified lower bound is below the radius go through the entry; the tunnelling
    ones get the window, every other drone the certified-clear values and first_conflict = +inf."""
    import torch
    from drone_path_planning_python_amd.swarm import (MeshClearanceResult, latest_replan_time, mesh_conflict_windows)
    coef, dur, tris = MC.certify_case()
    md, tm, tri, lower = ME.fp64_mesh_clearance(coef, dur, tris)
    tt = torch.from_numpy
    z = torch.zeros(12, dtype=torch.float64)
    hit = tt(md < MC.CERTIFY_RADIUS)
    mres = MeshClearanceResult(tt(md), tt(tm), tt(tri), tt(lower), hit, ~hit & tt(lower < MC.CERTIFY_RADIUS), ~hit, z, hit,
                               0.05, 12)
    res = mesh_conflict_windows(_Compute(), mres, tt(coef), tt(dur), tt(tris), MC.CERTIFY_RADIUS)
    assert set(KC.TUNNELLING) <= set(res.idx.tolist()) and 0 not in res.idx.tolist()
    t_r = latest_replan_time(res, 0.3)
    KC.check_swarm_windows(res, t_r, coef, dur, 0.3)
    for d in set(range(12)) - set(res.idx.tolist()):
        got = tuple(x[d].item() for x in (res.t_clear_until, res.t_first, res.d_first, res.tri_first, res.t_last,
                                          res.d_last, res.tri_last, res.t_clear_from))
        assert got == MX.CLEAR and res.first_conflict[d].item() == np.inf
    assert (latest_replan_time(res, 10.0)[list(KC.TUNNELLING)] == 0.0).all()            # clamped at 0
    with pytest.raises(ValueError):
        mesh_conflict_windows(_Compute(), mres, tt(coef), tt(dur), tt(tris), -1.0)
    with pytest.raises(ValueError):
        mesh_conflict_windows(_Failing(), mres, tt(coef), tt(dur), tt(tris), MC.CERTIFY_RADIUS)


def test_argument_checks_without_gpu():
    from drone_path_planning_python_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    outs = (p,) * 9
    for fn in (lib.msnap_mesh_conflict_window, lib.msnap_mesh_conflict_window_device):
        assert fn(None, 1, 1, p, p, 1, p, 0.25, 1e-6, *outs) == -1                       # MSNAP_EINVAL: no context
        assert fn(None, 0, 1, p, p, 1, p, 0.25, 1e-6, *outs) == -1                       # before the no-op
    h = ctypes.c_void_p()
    if lib.msnap_create(ctypes.byref(h), 0, 7, 4) == 0:       # a GPU is present: the checks that need a context
        try:
            for f in (lib.msnap_mesh_conflict_window, lib.msnap_mesh_conflict_window_device):
                assert f(h, 1, 5, p, p, 1, p, 0.25, 1e-6, *outs) == -4                    # MSNAP_ESEGMENTS
                for thr, res in ((-0.1, 1e-6), (np.nan, 1e-6), (np.inf, 1e-6), (0.25, 0.0), (0.25, -1.0), (0.25, np.inf),
                                 (0.25, np.nan)):
                    assert f(h, 1, 1, p, p, 1, p, thr, res, *outs) == -1
                    assert f(h, 0, 1, p, p, 1, p, thr, res, *outs) == -1                  # before the no-op
                assert f(h, 1, 1, p, p, 1, p, 0.25, 1e-6, None, *outs[1:]) == -1          # a null array
                assert f(h, 1, 1, p, p, 1, None, 0.25, 1e-6, *outs) == -1                 # tris == NULL with n_tris > 0
                assert f(h, 0, 1, None, None, 0, None, 0.0, 1e-6, *(None,) * 9) == 0      # no-op
        finally:
            lib.msnap_destroy(h)


def test_the_new_object_is_in_the_build_checks_uses_no_scratch_and_has_no_lane_retiring_loop():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    assert OBJ in chk.K19_OBJS
    if not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.skip("no object file / ROCm LLVM tools here")
    assert chk.lane_latches(OBJ) == {}
    n_kernels, n_spill, bad = chk.check(OBJ)
    assert n_kernels == 6 and not bad and n_spill == 0      # per order a flags, a lane and a fold kernel
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", OBJ, os.path.join(tmp, "copy.o")], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fat}", f"--output={co}"], check=True)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    vgpr = [int(x) for x in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    assert len(scratch) == 6 == len(vgpr) and scratch == [0] * 6 and max(vgpr) <= 256, list(zip(vgpr, scratch))
