"""Pairwise clearance on the GPU where it is not comfortable (include/msnap.h, "pairwise clearance"): far from the
origin, extreme scales, long paths, knots that nearly coincide, degenerate differences, minima at the window's ends,
the input with the most nodes found, and the shape of the list.  Every case runs msnap_pair_clearance, checks the
header's inequalities (with the coordinate term c 2^-52 R) against the exact reference (tests/clearance_exact.py), that
msnap_eval_flat at t_min gives min_dist back, and that the kernel stays within 1e-9 of the NumPy restatement.  The
inputs and the test bodies are tests/clearance_cases.py's, solved here by the GPU solve.  Both orders: far offsets
(15 of the 21 pairs at order 7, 6 at order 9), the loner (6 / 3 pairs), the 2000 m crossings, knots, degenerate pairs,
window ends, the depth cap, list shapes.  Order 7 only: the four extreme scales (4 pairs each), 49 and 4096 segments.
Order 9 only: 12 and 20 segments (3 pairs each).  The exact reference sets these counts: it costs 0.1-1 s per pair."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_cases as CC  # noqa: E402
import clearance_exact as CE  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(ctx7, ctx9):
    return {8: ctx7, 10: ctx9}


@pytest.fixture(scope="module")
def solve(ctxs):
    def run(wp, t, nc):
        coef, dur, status = ctxs[nc].solve_batch(wp, t)
        assert (status == 0).all()
        return coef, dur
    return run


# ------------------------------------------------------------------------------------------------ far from the origin
@pytest.fixture(scope="module")
def far(ctxs, solve):
    """Per order, built on first use: the base swarm of 7 drones, the exact D of 15 of its pairs at order 7 and of 6
    at order 9 (the exact reference at degree 18 costs four times as much), the kernel's outputs at the origin."""
    cache = {}

    def get(nc):
        if nc not in cache:
            cache[nc] = CC.far_origin(ctxs[nc], solve, nc, n_pairs=15 if nc == 8 else 6)
        return cache[nc]
    return get


@pytest.mark.parametrize("name", list(CC.OFFSETS))
@pytest.mark.parametrize("nc", [8, 10])
def test_far_from_the_origin(ctxs, far, nc, name):
    CC.check_far(ctxs[nc], far(nc), name)


@pytest.mark.parametrize("nc", [8, 10])
def test_a_loner_at_minus_8000_against_a_swarm_at_plus_5000(ctxs, far, nc):
    CC.check_loner(ctxs[nc], far(nc), n_pairs=6 if nc == 8 else 3)


# ------------------------------------------------------------------------------------------------ scales
@pytest.mark.parametrize("scale_t,scale_w", CC.SCALES)
def test_extreme_scales(ctxs, solve, scale_t, scale_w):
    coef, dur = CC.scaled(solve, 8, scale_t, scale_w)
    CE.check_contract(ctxs[8], coef, dur, CC.all_pairs(6)[:4], with_R=True)     # (the root finder is slow at these scales)


@pytest.mark.parametrize("total", [11.0, 1.1])
@pytest.mark.parametrize("nc", [8, 10])
def test_a_crossing_of_2000_m(ctxs, solve, nc, total):
    CC.check_crossing(ctxs[nc], solve, nc, total)


# ------------------------------------------------------------------------------------------------ long paths
@pytest.mark.parametrize("unequal", [False, True])
def test_order7_at_49_segments(ctxs, solve, unequal):
    """97 slots per pair, more than a wavefront; 15 pairs = 1455 lanes, pairs straddling the 256-lane workgroups."""
    coef, dur = CC.long_paths(solve, 8, 49, unequal=unequal)
    pairs = CC.all_pairs(6)
    assert (pairs.shape[0] * 97) % 256 != 0 and 256 % 97 != 0
    md, tm, lower, _ = CE.check_contract(ctxs[8], coef, dur, pairs, with_R=True)
    if unequal:
        window = np.add.accumulate(dur[0])[-1]
        assert (tm[:5] <= window).all() and window < dur[1:].sum(axis=1).min() - 1.0


def test_order7_at_max_segments(ctxs, solve):
    ctx = ctxs[8]
    coef, dur = CC.stacked(solve, 8, ctx.max_segments, n=2)              # 8191 slots for the one pair
    assert coef.shape[1] == ctx.max_segments == 4096
    CE.check_contract(ctx, coef, dur, CC.all_pairs(2), with_R=True)


@pytest.mark.parametrize("m", [12, 20])
def test_order9_long(ctxs, solve, m):
    coef, dur = CC.long_paths(solve, 10, m)
    CE.check_contract(ctxs[10], coef, dur, CC.all_pairs(6)[:3], with_R=True)


# ------------------------------------------------------------------------------------------------ knots
@pytest.mark.parametrize("kind", ["ulp", "rel", "short"])
@pytest.mark.parametrize("nc", [8, 10])
def test_knots_that_nearly_coincide(ctxs, solve, nc, kind):
    CC.check_knots(ctxs[nc], solve, nc, kind)


# ------------------------------------------------------------------------------------------------ degenerate differences
@pytest.mark.parametrize("nc", [8, 10])
def test_identical_drones_and_a_copy_moved_by_half_a_metre(ctxs, solve, nc):
    CC.check_copies(ctxs[nc], solve, nc)


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("nc", [8, 10])
def test_two_hovering_drones(ctxs, nc, m):
    CC.check_hovering(ctxs[nc], nc, m)


@pytest.mark.parametrize("nc", [8, 10])
def test_a_hovering_drone_against_a_moving_one(ctxs, solve, nc):
    CC.check_hover_against_moving(ctxs[nc], solve, nc)


# ------------------------------------------------------------------------------------------------ the window's ends
@pytest.mark.parametrize("nc", [8, 10])
def test_minimum_at_the_ends_of_the_window(ctxs, nc):
    CC.check_ends_by_hand(ctxs[nc], nc)


@pytest.mark.parametrize("nc", [8, 10])
def test_minimum_at_the_ends_of_the_window_on_solved_paths(ctxs, solve, nc):
    CC.check_ends_solved(ctxs[nc], solve, nc)


# ------------------------------------------------------------------------------------------------ the caps
@pytest.mark.parametrize("dz", [0.0, 1e-7])
@pytest.mark.parametrize("nc", [8, 10])
def test_the_depth_cap(ctxs, solve, nc, dz):
    """CC.fast_crossing: at order 9 the restatement meets the depth cap (tests/test_clearance_cpu.py asserts it on the
    oracle's coefficients); at order 7 the same input closes at depth 40.  Either way lower <= D and no status."""
    CC.check_caps(ctxs[nc], solve, nc, dz)


# ------------------------------------------------------------------------------------------------ the list
@pytest.mark.parametrize("nc,m,counts", [(8, 1, (1, 64, 65, 66)), (8, 4, (1, 64, 55, 46)), (10, 4, (64, 55, 46))])
def test_list_lengths_around_a_wavefront_and_repeated_pairs(ctxs, solve, nc, m, counts):
    """slots = 2 m - 1 lanes per pair: the counts put the last lane at 63, 64 and 65 of a wavefront."""
    ctx = ctxs[nc]
    slots = 2 * m - 1
    assert sorted((c * slots - 1) % 64 for c in counts if c > 1) == [0, 1, 63]
    coef, dur = solve(*CC.swarm(7600 + m, 12, m), nc)
    pairs = CC.all_pairs(12)                                  # 66 pairs
    md, tm, lower = CC.run(ctx, coef, dur, pairs)
    rmd, rtm, rlower = CE.fp64_clearance(coef, dur, pairs)
    np.testing.assert_allclose(md, rmd, rtol=1e-9, atol=CE.ABS_ROUND)
    np.testing.assert_allclose(lower, rlower, rtol=1e-9, atol=CE.ABS_CLOSE)
    CE.check_contract(ctx, coef, dur, pairs[:6 if nc == 8 else 3], with_R=True)
    for c in counts:
        got = CC.run(ctx, coef, dur, pairs[66 - c:])
        for g, w in zip(got, (md, tm, lower)):
            assert np.array_equal(g, w[66 - c:]), c
    # one pair several times, and (a, b) next to (b, a)
    lst = np.array([(3, 7), (7, 3), (0, 1), (3, 7), (7, 3), (7, 3), (3, 7)], dtype=np.int32)
    got = CC.run(ctx, coef, dur, lst)
    k = int(np.nonzero((pairs == (3, 7)).all(axis=1))[0][0])
    for g, w in zip(got, (md, tm, lower)):
        assert (g[[0, 1, 3, 4, 5, 6]] == w[k]).all() and g[2] == w[0]
