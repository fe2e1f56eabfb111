"""Cross clearance without a GPU: the NumPy restatement of the new lanes against the exact reference on the cases of
tests/test_cross_clearance_gpu.py (through cross_clearance_exact.RestatedContext), the measured ratios below the two
constants, every walk closed, the restatement's own identities, the pair logic of swarm.certify_replan with a stand-in
compute object, the argument checks of the C entries that need no GPU, and the build checks on the kernels' object."""
import ctypes
import os
import sys

import numpy as np
import pytest

import c_oracle
from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_exact as CE  # noqa: E402
import cross_clearance_cases as XC  # noqa: E402
import cross_clearance_exact as XE  # noqa: E402

OBJ = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_clearance.o")


def solve(wp, t, nc):
    coef, dur, info, _ = c_oracle.solve_batch(wp, t, ncoef=nc)
    assert not info.any()
    return coef, dur


@pytest.mark.parametrize("nc, ma, mb", [(8, 3, 10), (8, 1, 1), (10, 2, 5)])
def test_restatement_against_the_exact_reference_unequal_segment_counts(nc, ma, mb):
    XC.check_near(XE.RestatedContext(nc - 1), solve, nc, ma, mb)


def test_restatement_far_from_the_origin_stays_below_c_round_cross():
    XC.check_far_origin(XE.RestatedContext(7), solve)


def test_restatement_on_a_far_clock_stays_below_c_clock():
    XC.check_far_clock(XE.RestatedContext(7), solve)


def test_restatement_finds_the_shifted_crossing():
    XC.check_crossing(XE.RestatedContext(7), solve)


def test_restatement_windows():
    XC.check_windows(XE.RestatedContext(7), solve)


def test_restatement_identities():
    XC.check_identities_in_one_entry(XE.RestatedContext(7), solve)


def test_one_set_against_itself_is_the_pairwise_restatement_bit_for_bit():
    for nc, m in ((8, 1), (8, 2), (8, 10), (10, 4)):
        coef, dur = solve(*XC.swarm(7000 + m, 6, m), nc)
        want = CE.fp64_clearance(coef, dur, XC.ALL15)
        for t0 in (None, np.zeros(6)):
            got = XE.fp64_cross_clearance(coef, dur, t0, coef, dur, t0, XC.ALL15)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_every_walk_of_these_inputs_closes():
    cases = [XC.unequal(solve, 8, 3, 10), XC.unequal(solve, 8, 1, 1), XC.unequal(solve, 10, 2, 5), XC.far_origin(solve),
             XC.far_clock(solve, offset=5000.0), XC.crossing(solve), XC.crossing(solve, 8, 3.7, 3.9), XC.windows(solve)]
    for (ca, da, ta), (cb, db, tb), pairs in cases:
        st = {}
        XE.fp64_cross_clearance(ca, da, ta, cb, db, tb, pairs, stats=st)
        assert st["lanes"] > 0 and not st["capped"].any() and st["nodes"].max() < XE.MAX_NODES


def test_a_continued_path_against_the_path_it_left():
    """A path that continues its old one from t_r (cross_clearance_cases.continued) starts ON it: t_min == t_r."""
    coef, dur = solve(*XC.swarm(8, 8, 6), 8)
    idx = [1, 4, 6]
    t_r = 0.4 * np.add.accumulate(dur, axis=1)[idx, -1]
    new_coef, new_dur = XC.continued(coef, dur, idx, t_r)
    A, B = (new_coef, new_dur, t_r), (coef[idx], dur[idx], None)
    md, tm, lower, _, _ = XE.check_contract(XE.RestatedContext(7), A, B, [(k, k) for k in range(3)], full=True)
    for k in range(3):
        args = (new_coef[k], new_dur[k], t_r[k], coef[idx[k]], dur[idx[k]], 0.0)
        r = XE.allowance(XE.pair_R(*args), XE.T_c(new_dur[k], t_r[k], dur[idx[k]], 0.0), XE.pair_Rprime(*args))
        assert tm[k] == t_r[k] and md[k] <= r and lower[k] <= r


class _Compute:
    """DeviceCompute's cross_clearance on CPU tensors through the restatement."""

    def cross_clearance(self, coef_a, dur_a, coef_b, dur_b, pairs, t0_a=None, t0_b=None):
        import torch
        n = lambda x: None if x is None else x.numpy()      # noqa: E731
        md, tm, lower = XE.fp64_cross_clearance(n(coef_a), n(dur_a), n(t0_a), n(coef_b), n(dur_b), n(t0_b), n(pairs))
        return tuple(torch.from_numpy(x) for x in (md, tm, lower, np.zeros(len(md), dtype=np.int32)))


def test_certify_replan_pairs_and_verdicts_with_a_stand_in():
    import torch
    from drone_path_planning_python_amd.swarm import certify_replan
    coef, dur, new_coef, new_dur = XC.replan_swarm(solve)
    tt = torch.from_numpy
    res = certify_replan(_Compute(), tt(coef), tt(dur), XC.REPLAN_IDX, tt(np.array(XC.REPLAN_T_R)), tt(new_coef),
                         tt(new_dur), XC.REPLAN_RADIUS)
    XC.check_replan(res, coef, dur, new_coef, new_dur)
    with pytest.raises(ValueError):
        certify_replan(_Compute(), tt(coef), tt(dur), [2, 2, 9], 0.4, tt(new_coef), tt(new_dur), 0.1)
    with pytest.raises(ValueError):
        certify_replan(_Compute(), tt(coef), tt(dur), XC.REPLAN_IDX, 0.4, tt(new_coef), tt(new_dur), 0.1,
                       new_status=torch.tensor([0, 2, 0]))


def test_argument_checks_without_gpu():
    from drone_path_planning_python_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.msnap_cross_clearance, lib.msnap_cross_clearance_device):
        assert fn(None, 1, 1, p, p, None, 1, 1, p, p, None, 1, p, p, p, p, p) == -1       # MSNAP_EINVAL: no context
        assert fn(None, 1, 1, p, p, None, 1, 1, p, p, None, 0, p, p, p, p, p) == -1       # before the no-op
    h = ctypes.c_void_p()
    if lib.msnap_create(ctypes.byref(h), 0, 7, 4) == 0:       # a GPU is present: the checks that need a context
        try:
            f = lib.msnap_cross_clearance
            assert f(h, 1, 5, p, p, None, 1, 1, p, p, None, 1, p, p, p, p, p) == -4       # MSNAP_ESEGMENTS, set A
            assert f(h, 1, 1, p, p, None, 1, 0, p, p, None, 1, p, p, p, p, p) == -4       # set B
            assert f(h, -1, 1, p, p, None, 1, 1, p, p, None, 1, p, p, p, p, p) == -1
            assert f(h, 1, 1, p, p, None, 1, 1, p, p, None, -1, p, p, p, p, p) == -1
            assert f(h, 1, 1, p, p, None, 1, 1, None, p, None, 1, p, p, p, p, p) == -1    # a null array
            assert f(h, 1, 1, None, None, None, 1, 1, None, None, None, 0, None, None, None, None, None) == 0   # no-op
        finally:
            lib.msnap_destroy(h)


def test_the_new_object_is_in_the_build_checks_and_has_no_lane_retiring_loop():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    assert OBJ in chk.DEFAULT_OBJS
    if not os.path.exists(OBJ) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no object file / ROCm LLVM tools here")
    assert chk.lane_latches(OBJ) == {}
    n_kernels, n_spill, bad = chk.check(OBJ)
    assert n_kernels == 10 and not bad      # 2 flags kernels, a lane and a fold kernel per (order, CROSS)
