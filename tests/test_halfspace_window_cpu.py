"""Half-space windows without a GPU (include/msnap.h, "half-space windows"): the NumPy restatement of
the lane and fold rules against the exact reference (tests/halfspace_exact.py) on the cases of tests/halfspace_cases.py,
the proof that every solved fixture of the closing checks has only transversal crossings, the restatement's own
identities, swarm.geofence_windows / certify_corridor with a stand-in compute object built on the restatement, the
argument checks of the C entries that need no GPU, and the build checks on the kernels' object."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extent_cases as EC  # noqa: E402
import extent_exact as XE  # noqa: E402
import halfspace_cases as HC  # noqa: E402
import halfspace_exact as HE  # noqa: E402
# the restatement restates kernels of this tree: without the entry and the functions around it nothing here applies
from drone_path_planning_python_amd import _lib  # noqa: E402
from drone_path_planning_python_amd.swarm import (CORRIDOR_FAILED, CORRIDOR_INSIDE, CORRIDOR_OUTSIDE,  # noqa: E402
                                                  CORRIDOR_UNDECIDED, certify_corridor, certify_geofence,
                                                  geofence_windows, latest_replan_time)

assert {"msnap_halfspace_window", "msnap_halfspace_window_device"} <= set(_lib.SIGNATURES)

CSRC = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc")
OBJ = os.path.join(CSRC, "msnap_halfspace.o")
LLVM = "/opt/rocm/lib/llvm/bin"
# msnap_conflict.o's kernels before and after first_crossing moved into msnap_walk.h (code-object metadata, sorted)
CONFLICT_VGPRS = sorted([8, 154, 94, 154, 126, 8, 192, 109, 192, 94])
SWARM_CASES = [(name, order) for name in sorted(HC.SWARMS) for order in (7, 9)]


@pytest.mark.parametrize("nc", [8, 10])
def test_restatement_parabola_is_outside_on_one_quarter_to_three_quarters(nc):
    HC.check_parabola(HE.RestatedContext(nc - 1), nc - 1)


def test_restatement_tangency_is_never_outside():
    HC.check_tangency(HE.RestatedContext(7))


@pytest.mark.parametrize("order", [7, 9])
def test_restatement_overshoot_window_contains_t_3(order):
    HC.check_overshoot(HE.RestatedContext(order), order)


def test_restatement_two_conflicts_in_one_query_give_the_first_and_the_last():
    HC.check_two_conflicts(HE.RestatedContext(7))


def test_restatement_outside_at_the_start_and_at_the_end_of_the_range():
    HC.check_ends(HE.RestatedContext(7))


def test_restatement_ranges_inside_a_violation_empty_and_one_instant():
    HC.check_ranges(HE.RestatedContext(7))


def test_restatement_partial_segments():
    HC.check_partial_segments(HE.RestatedContext(7))


def test_restatement_zero_nonfinite_and_nonunit_planes():
    HC.check_planes(HE.RestatedContext(7))


def test_restatement_closing_gap_follows_t_res():
    HC.check_t_res(HE.RestatedContext(7))


@pytest.mark.parametrize("name,order", SWARM_CASES)
def test_every_solved_fixture_has_only_transversal_crossings(name, order):
    HE.assert_transversal(HC.swarm_fixture(name, order)[4])


@pytest.mark.parametrize("name,order", SWARM_CASES)
def test_restatement_solved_swarms_near_far_and_long(name, order):
    HC.check_swarm(HE.RestatedContext(order), name, order)


def test_restatement_identities():
    HC.check_identities(HE.RestatedContext(7))


def test_measured_rounding_leaves_the_extent_constant_in_place():
    assert 0.0 < 10.0 * HE.WORST_MEASURED < XE.C_ROUND_EXTENT == HE.C_ROUND_HALFSPACE


_Compute, overshoot_swarm = HE.RestatedCompute, HC.overshoot_swarm


def test_swarm_geofence_windows_with_a_stand_in():
    import torch
    coef, dur = overshoot_swarm([1.0, 0.3])
    tt = torch.from_numpy
    comp = _Compute()
    geo = certify_geofence(comp, tt(coef), tt(dur), lo=EC.BOX_LO, hi=EC.BOX_HI)
    assert geo.outside.tolist() == [True, False] and geo.inside.tolist() == [False, True]
    res = geofence_windows(comp, geo, tt(coef), tt(dur))
    assert res.idx.tolist() == [0] and res.queries.shape == (6, 2)
    want = HE.fp64_halfspace_window(coef, dur, HC.X_LE(EC.BOX_HI[0]), HC.Q00)
    assert res.first_broken.tolist() == [0, -1]                        # +x is the first side that is broken
    assert res.first_conflict[0] == want[1][0] < 3.0 < res.last_conflict[0]
    assert res.inside_until[0] <= res.first_conflict[0] and res.inside_from[0] >= res.last_conflict[0]
    assert res.first_conflict[1] == np.inf and res.last_conflict[1] == -np.inf
    assert res.inside_until[1] == np.inf and res.inside_from[1] == -np.inf
    t_r = latest_replan_time(res, 0.3)
    assert t_r[0] == res.first_conflict[0] - 0.3 and t_r[1] == np.inf


def _corridor(chain, radius=0.0, coef_dur=None, status=None):
    import torch
    coef, dur = HC.chain_flights() if coef_dur is None else coef_dur
    planes, off = HC.boxes(*HC.CHAIN_BOXES)
    tt = torch.from_numpy
    return certify_corridor(_Compute(), tt(coef), tt(dur), tt(planes), off, chain, radius=radius, status=status)


def test_certify_corridor_chain_of_three_boxes_with_a_stand_in():
    res = _corridor([0, 1, 2])
    assert res.verdict.tolist() == [CORRIDOR_INSIDE, CORRIDOR_OUTSIDE, CORRIDOR_OUTSIDE, CORRIDOR_OUTSIDE]
    assert res.stage.tolist() == [-1, 1, 0, 2]
    assert res.plane.tolist() == [-1, 6 + 2, 1, 12 + 0]           # box 1's y <= 1; box 0's -x <= 0; box 2's x <= 10
    h = res.handover.numpy()
    assert h[0, 0] == 0.0 < h[0, 1] < h[0, 2] < 8.0 and res.proven_until[0] == 8.0
    assert np.isnan(h[1, 2]) and np.isnan(h[2, 1:]).all() and h[2, 0] == 0.0
    assert res.proven_until[2] == 0.0 and res.first_conflict[2] == 0.0 and res.value[2] == 1.0      # -x = 1 at the start
    assert res.first_conflict[0] == np.inf
    # the hand-over is the latest time proven inside the stage, t_res before the path leaves it
    coef, dur = HC.chain_flights()
    planes, _ = HC.boxes(*HC.CHAIN_BOXES)
    leave0 = HE.fp64_halfspace_window(coef, dur, planes, np.array([[0, 0]]))[0][0]      # x <= 4 of box 0
    assert h[0, 1] == leave0 - 1e-6
    # flight 1 leaves box 1 at y = 1, flight 3 the last box at x = 10: proven until then, and found within t_res of it
    for d in (1, 3):
        assert 0.0 < res.proven_until[d] <= res.first_conflict[d] <= res.proven_until[d] + 2e-6 < 8.0
    assert abs(res.value[1] - 1.0) < 1e-5 and abs(res.value[3] - 10.0) < 1e-5


def test_certify_corridor_chain_shapes_empty_polytope_radius_and_failed():
    import torch
    shared = _corridor([0, 1, 2])
    padded = _corridor(np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 2]]))
    for f in ("verdict", "proven_until", "stage", "plane", "first_conflict", "value", "handover"):
        assert np.array_equal(getattr(shared, f).numpy(), getattr(padded, f).numpy(), equal_nan=True), f
    # per-drone chains with padding: flight 0 through two stages only stops in box 1, which ends before the path does
    res = _corridor(np.array([[0, 1, -1], [0, 1, 2], [0, -1, -1], [0, 1, 2]]))
    assert res.verdict.tolist()[0] == CORRIDOR_OUTSIDE and res.stage.tolist() == [1, 1, 0, 2]
    assert res.plane[0] == 6 + 0                                      # box 1's x <= 7
    assert np.array_equal(res.handover.numpy()[1], shared.handover.numpy()[1], equal_nan=True)
    # an empty polytope is all of space: the chain 0 -> (empty) certifies every drone that starts inside box 0
    coef, dur = HC.chain_flights()
    planes, off = HC.boxes(*HC.CHAIN_BOXES)
    tt = torch.from_numpy
    off2 = np.concatenate([off, off[-1:]])                            # polytope 3: no planes
    res = certify_corridor(_Compute(), tt(coef), tt(dur), tt(planes), off2, [0, 3])
    # (flight 2 starts outside box 0, but no position is outside all of space: that stop is never definite)
    assert res.verdict.tolist() == [CORRIDOR_INSIDE, CORRIDOR_INSIDE, CORRIDOR_UNDECIDED, CORRIDOR_INSIDE]
    # the radius moves each limit by radius |n|: flight 1 meets y <= 1 - 0.25 earlier, and a doubled plane the same
    r0, r1 = _corridor([0, 1, 2]), _corridor([0, 1, 2], radius=0.25)
    assert r1.stage.tolist() == r0.stage.tolist() and r1.first_conflict[1] < r0.first_conflict[1]
    assert abs(r1.value[1] - 0.75) < 1e-5
    planes2 = planes.copy()
    planes2[8] *= 2.0
    r2 = certify_corridor(_Compute(), tt(coef), tt(dur), tt(planes2), off, [0, 1, 2], radius=0.25)
    assert r2.first_conflict[1] == r1.first_conflict[1] and r2.stage.tolist() == r1.stage.tolist()
    # a failed drone is refused
    res = _corridor([0, 1, 2], status=np.array([0, 0, 0, 3], dtype=np.int32))
    assert res.verdict.tolist()[3] == CORRIDOR_FAILED and bool(res.proven_until[3].isnan()) and res.stage[3] == -1
    for bad_chain in ([-1, 0, 1], [0, -1, 1], [0, 5, 1], np.zeros((3, 2), dtype=np.int64)):
        with pytest.raises(ValueError):
            _corridor(bad_chain)
    with pytest.raises(ValueError):
        _corridor([0, 1, 2], radius=-1.0)


def test_argument_checks_without_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    outs = (p,) * 7
    for fn in (lib.msnap_halfspace_window, lib.msnap_halfspace_window_device):
        assert fn(None, 1, 1, p, p, 1, p, 1, p, None, None, 1e-6, *outs) == -1          # MSNAP_EINVAL: no context
        assert fn(None, 1, 1, p, p, 1, p, 0, p, None, None, 1e-6, *outs) == -1          # before the no-op
    h = ctypes.c_void_p()
    if lib.msnap_create(ctypes.byref(h), 0, 7, 4) == 0:       # a GPU is present: the checks that need a context
        try:
            f = lib.msnap_halfspace_window
            assert f(h, 1, 5, p, p, 1, p, 1, p, None, None, 1e-6, *outs) == -4          # MSNAP_ESEGMENTS
            for res in (0.0, -1.0, np.inf, np.nan):
                assert f(h, 1, 1, p, p, 1, p, 1, p, None, None, res, *outs) == -1
                assert f(h, 1, 1, p, p, 1, p, 0, p, None, None, res, *outs) == -1       # before the no-op
            assert f(h, 1, 1, p, p, 1, None, 1, p, None, None, 1e-6, *outs) == -1       # planes == NULL, n_planes > 0
            assert f(h, 1, 1, p, p, -1, p, 1, p, None, None, 1e-6, *outs) == -1
            assert f(h, 1, 1, p, p, 1, p, 1, p, None, None, 1e-6, None, *outs[1:]) == -1    # a null array
            assert f(h, 1, 1, None, None, 0, None, 0, None, None, None, 1e-6, *(None,) * 7) == 0      # no-op
        finally:
            lib.msnap_destroy(h)


def _notes(obj, tmp):
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    return ([int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)],
            [int(x) for x in re.findall(r"\.vgpr_count:\s+(\d+)", notes)],
            [int(x) for x in re.findall(r"\.agpr_count:\s+(\d+)", notes)])


def test_the_new_object_is_in_the_build_checks_uses_no_scratch_and_the_conflict_object_keeps_its_registers():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    assert OBJ in chk.K20_OBJS
    if not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.skip("no object file / ROCm LLVM tools here")
    assert chk.lane_latches(OBJ) == {}
    n_kernels, n_spill, bad = chk.check(OBJ)
    assert n_kernels == 6 and not bad and n_spill == 0      # per order: the flags kernel, the lane kernel, the fold kernel
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        scratch, vgpr, agpr = _notes(OBJ, tmp)
    assert len(scratch) == 6 == len(vgpr) and scratch == [0] * 6 and agpr in ([], [0] * 6) and max(vgpr) <= 128, (vgpr, scratch)
    with tempfile.TemporaryDirectory() as tmp:
        scratch, vgpr, _ = _notes(os.path.join(CSRC, "msnap_conflict.o"), tmp)
    assert scratch == [0] * 10 and sorted(vgpr) == CONFLICT_VGPRS, vgpr
