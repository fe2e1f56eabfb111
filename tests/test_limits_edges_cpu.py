"""The dynamic-limit peaks where they are not comfortable, without a GPU: the inputs of tests/test_limits_edges_gpu.py
(tests/limits_cases.py) through limits_exact.fp64_walk_peaks, the NumPy restatement of the kernel, against the exact
reference.  What is asserted here about the restatement -- the contract with its coordinate term, the tie rule, the
closed ends, exact retiming by powers of two -- is what the GPU tests assert about the kernel; and the equioscillating
speeds leave the allowance WITHOUT the coordinate term, which is why the header has it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limits_cases as LC  # noqa: E402
import limits_exact as LE  # noqa: E402


def _total(dur_d):
    """the path's end as msnap_eval_flat accumulates it"""
    acc = 0.0
    for T in dur_d:
        acc = acc + float(T)
    return acc


def test_equioscillating_speeds_need_the_coordinate_term():
    broken = []
    for nc in (8, 10):
        coef, dur = LC.equioscillating(nc)
        res = LE.walk_peaks(coef, dur)
        peak, t_peak, nodes, capped = res[:4]
        assert not capped.any() and nodes.max() < LE.MAX_NODES
        LC.check_contract(coef, dur, peak, t_peak, with_R=True, label=f"order {nc - 1}")
        LC.check_attained(coef, dur, peak, t_peak, label=f"order {nc - 1}")
        worst = LC.horner_ratios(coef, dur, res).max()
        assert worst < LE.C_ROUND_PEAKS / 10 + 1e-3        # the constant is ten times the worst ratio measured
        for d in range(coef.shape[0]):
            S, _ = LE.exact_peaks(coef[d], dur[d])
            broken += [(nc, d, q) for q in range(4) if not LE.in_contract(peak[d, q], S[q])]
    print("outside the allowance without the coordinate term:", broken)
    assert broken


def test_the_value_at_t_peak_deep_into_a_path_needs_the_time_term():
    """1500 equioscillating segments, the acceleration and jerk peaks on the steep last point of the last one: the
    Horner's rounding stays within C_ROUND_PEAKS / 10 of 2^-52 R_q, the rounding of t_peak = acc + T u moves the exact
    value at t_peak by far more than r_q -- and by less than the header's proven term for it."""
    needed = []
    for nc in (8, 10):
        coef, dur = LC.deep_path(nc, 1500)
        res = LE.walk_peaks(coef, dur)
        assert not res.capped.any() and (res.seg[0, 1:3] == 1499).all()
        assert LC.horner_ratios(coef, dur, res).max() < LE.C_ROUND_PEAKS / 10 + 1e-3
        later = LC.later_pairs(res, dur)
        LC.check_attained(coef, dur, res.peak, res.t_peak, label=f"order {nc - 1}", later=later)
        err, R, tau = LC.attained_errors(coef, dur, res.peak, res.t_peak, later)
        needed += [(nc, q) for q in range(4) if err[0, q] > LE.round_term(R[0, q]) + 1e-15]
    print("beyond r_q at t_peak:", needed)
    assert needed


@pytest.mark.parametrize("nc", [8, 10])
def test_hand_built_polynomials_come_out_bit_for_bit(nc):
    for name, (coef, dur, want) in LC.hand_built(nc).items():
        peak, t_peak, nodes, capped = LE.fp64_walk_peaks(coef, dur)
        assert not capped.any()
        LC.check_contract(coef, dur, peak, t_peak, with_R=False, label=name)
        for q, (value, time) in want.items():
            if value is not None:
                assert peak[0, q] == value, (name, q, peak[0, q])
            assert t_peak[0, q] == time, (name, q, t_peak[0, q])
    one = LC.hand_built(nc)["one segment"]
    assert LE.fp64_walk_peaks(*one[:2])[2][0, 0, 0] == 3      # the speed's lane: the root's midpoint attains, two children


@pytest.mark.parametrize("nc", [8, 10])
def test_ties_across_segments_and_the_closed_ends(nc):
    coef, dur = LC.tie_segments(nc)
    peak, t_peak, _, _ = LE.fp64_walk_peaks(coef, dur)
    assert (t_peak[0] <= dur[0, 0]).all()
    LC.check_contract(coef, dur, peak, t_peak, with_R=False, label="tie")
    coef, dur = LC.tie_segments(nc, bump=True)
    peak, t_peak, _, _ = LE.fp64_walk_peaks(coef, dur)
    assert (t_peak[0] >= dur[0, 0] + dur[0, 1]).all()
    LC.check_contract(coef, dur, peak, t_peak, with_R=False, label="tie, third scaled up")
    coef, dur = LC.rising(nc)
    peak, t_peak, _, _ = LE.fp64_walk_peaks(coef, dur)
    assert (t_peak[0] == _total(dur[0])).all()
    _, tS = LE.exact_peaks(coef[0], dur[0])
    assert all(abs(float(t) - _total(dur[0])) < 1e-14 for t in tS)        # the builder does what it says
    LC.check_contract(coef, dur, peak, t_peak, label="rising")
    coef, dur = LC.rising(nc, mirror=True)
    peak, t_peak, _, _ = LE.fp64_walk_peaks(coef, dur)
    assert (t_peak[0] == 0.0).all()
    LC.check_contract(coef, dur, peak, t_peak, label="falling")
    for later in (False, True):
        coef, dur = LC.knot_jump(nc, later)
        peak, t_peak, _, _ = LE.fp64_walk_peaks(coef, dur)
        assert (t_peak[0] == dur[0, 0]).all()
        LC.check_contract(coef, dur, peak, t_peak, label=f"jump, later {later}")
        for q in range(4):          # the value is that of the segment that holds the peak
            here = float(LE.exact_value_at(coef[0], dur[0], q, float(t_peak[0, q]), later=later))
            there = float(LE.exact_value_at(coef[0], dur[0], q, float(t_peak[0, q]), later=not later))
            assert abs(peak[0, q] - here) <= LE.round_term(LE.peaks_R(coef[0], dur[0])[q]) + 1e-15 and there < 0.9 * here


@pytest.mark.parametrize("nc", [8, 10])
def test_retiming_by_powers_of_two_is_exact_in_the_restatement(nc):
    rng = np.random.default_rng(nc)
    coef = rng.standard_normal((5, 3, 4, nc)) / np.arange(1, nc + 1) ** 2
    dur = rng.uniform(0.3, 2.0, size=(5, 3))
    p0, t0, n0, _ = LE.fp64_walk_peaks(coef, dur)
    for k in (2.0, 0.5, 8.0):
        p, t, n, _ = LE.fp64_walk_peaks(coef * k ** -np.arange(nc), dur * k)
        assert np.array_equal(p, p0 * k ** -np.array([1.0, 2.0, 3.0, 1.0])) and np.array_equal(t, t0 * k)
        assert np.array_equal(n, n0)


def test_restatement_status_and_agreement_with_the_root_finder():
    rng = np.random.default_rng(5)
    coef = rng.standard_normal((6, 3, 4, 8)) / np.arange(1, 9) ** 2
    dur = rng.uniform(0.3, 2.0, size=(6, 3))
    peak, _, _, capped = LE.fp64_walk_peaks(coef, dur)
    assert not capped.any()
    np.testing.assert_allclose(peak, LE.fp64_peaks(coef, dur), rtol=1e-9, atol=1e-12)
    coef[1, 1, 3, 2] = np.nan          # yaw only
    dur[2, 0] = 0.0
    dur[3, 2] = np.inf
    coef[4, 0, 0, 1] = np.nan
    dur[4, 2] = -1.0
    peak, t_peak, nodes, _, status, _, _ = LE.walk_peaks(coef, dur)
    assert status.tolist() == [0, 3, 2, 3, 3, 0]
    assert np.isnan(peak[1:5]).all() and np.isnan(t_peak[1:5]).all() and np.isfinite(peak[[0, 5]]).all()
    assert (nodes[1, 1, 3] == 0) and (nodes[1, 1, :3] > 0).all()      # a lane tests only the axes it reads


def test_peaks_R_is_the_sum_of_magnitudes():
    coef, dur, _ = LC.hand_built(8)["constant speed after a slower segment"]
    # speed: segment 0 has |t| + |t^2| -> 2 on T = 1, segment 1 the constant 3; acceleration |1| + |-2| T;
    # jerk 2; yaw rate 3 T^2
    assert LE.peaks_R(coef[0], dur[0]).tolist() == [3.0, 3.0, 2.0, 3.0]
    assert LE.in_contract(1.0, 1.0) and not LE.in_contract(1.0 + 3e-12, 1.0)
    assert LE.in_contract(1.0 + 3e-12, 1.0, R=3e-12 / (LE.C_ROUND_PEAKS * LE.EPS))
