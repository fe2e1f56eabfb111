"""Dynamic limits on the GPU where they are not comfortable (include/msnap.h, "dynamic limits"): hand-built polynomials
with closed-form peaks, ties across segments, peaks on the closed ends and at a jump, equioscillating speeds (the case
that needs the coordinate term r_q = c 2^-52 R_q of the contract), the attained value of all four quantities against
mpmath at t_peak, extreme scales, a batch that mixes busy, idle and failed lanes, every documented status, retiming by
powers of two, time_scale's pass-through, each limit alone (the jerk limit is the cbrt path), the corners of the common
scale, and a captured graph.  The inputs are tests/limits_cases.py's; tests/test_limits_edges_cpu.py runs the same
ones through the NumPy restatement of the kernel.  Both orders throughout."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limits_cases as LC  # noqa: E402
import limits_exact as LE  # noqa: E402

pytestmark = pytest.mark.gpu

EXPO = np.array([1.0, 2.0, 3.0, 1.0])      # derivative q of the path run k times slower scales by k^-EXPO[q]


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


@pytest.fixture(scope="module")
def solved(solve):
    """per order, solved once and left unchanged: 8 drones x 4 segments, their peaks"""
    cache = {}

    def get(ctx, nc):
        if nc not in cache:
            coef, dur = LC.solved_swarm(solve, nc)
            cache[nc] = (coef, dur) + _peaks(ctx, coef, dur)
        coef, dur, peak, t_peak = cache[nc]
        return coef.copy(), dur.copy(), peak.copy(), t_peak.copy()
    return get


def _peaks(ctx, coef, dur):
    peak, t_peak, status = ctx.dynamic_peaks(coef, dur)
    assert (status == 0).all()
    return peak, t_peak


def _total(dur_d):
    acc = 0.0
    for T in dur_d:
        acc = acc + float(T)
    return acc


# ------------------------------------------------------------------------------------------------ hand-built, closed form
@pytest.mark.parametrize("nc", [8, 10])
def test_hand_built_polynomials(ctxs, nc):
    import mpmath
    for name, (coef, dur, want) in LC.hand_built(nc).items():
        peak, t_peak = _peaks(ctxs[nc], coef, dur)
        LC.check_contract(coef, dur, peak, t_peak, with_R=False, label=name)
        # (the constant speed of the second segment starts at the knot: the one jump among these)
        LC.check_attained(coef, dur, peak, t_peak, label=name, later={(0, 0)} if coef.shape[1] == 2 else ())
        S, _ = LE.exact_peaks(coef[0], dur[0])
        for q, (value, time) in want.items():
            assert t_peak[0, q] == time, (name, q, t_peak[0, q])
            if value is not None and S[q] == mpmath.mpf(value):       # S is that double: the kernel reports it
                assert peak[0, q] == value, (name, q, peak[0, q])
    # the named cases once more, spelled out
    coef, dur, _ = LC.hand_built(nc)["one segment"]
    peak, t_peak = _peaks(ctxs[nc], coef, dur)
    assert t_peak[0, 0] == 0.5 and t_peak[0, 1] == 0.0 and peak[0, 1] == 1.0 and peak[0, 3] == 3.0
    coef, dur, _ = LC.hand_built(nc)["one segment, dyadic"]
    assert _peaks(ctxs[nc], coef, dur)[0][0].tolist() == [0.75, 3.0, 6.0, 3.0]
    coef, dur, _ = LC.hand_built(nc)["2-D tie of the ends"]
    peak, t_peak = _peaks(ctxs[nc], coef, dur)
    assert t_peak[0, 0] == 0.0 and peak[0, 0] == 1.0
    coef, dur, _ = LC.hand_built(nc)["constant speed after a slower segment"]
    peak, t_peak = _peaks(ctxs[nc], coef, dur)
    assert t_peak[0, 0] == dur[0, 0] and peak[0, 0] == 3.0


# ------------------------------------------------------------------------------------------------ ties across segments
@pytest.mark.parametrize("nc", [8, 10])
def test_ties_across_segments(ctxs, nc):
    coef, dur = LC.tie_segments(nc)
    assert np.array_equal(coef[0, 0], coef[0, 2]) and dur[0, 0] == dur[0, 2]
    peak, t_peak = _peaks(ctxs[nc], coef, dur)
    assert (t_peak[0] <= dur[0, 0]).all(), t_peak
    LC.check_contract(coef, dur, peak, t_peak, with_R=False, label="tie")
    LC.check_attained(coef, dur, peak, t_peak, label="tie")
    coef, dur = LC.tie_segments(nc, bump=True)
    peak2, t_peak2 = _peaks(ctxs[nc], coef, dur)
    assert (t_peak2[0] >= dur[0, 0] + dur[0, 1]).all(), t_peak2
    assert (peak2 > peak).all()
    LC.check_contract(coef, dur, peak2, t_peak2, with_R=False, label="tie, third scaled up")
    later = {(0, q) for q in range(4) if t_peak2[0, q] == dur[0, 0] + dur[0, 1]}      # (the third segment's start)
    LC.check_attained(coef, dur, peak2, t_peak2, label="tie, third scaled up", later=later)


# ------------------------------------------------------------------------------------------------ the closed ends
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("nc", [8, 10])
def test_peaks_on_the_closed_ends(ctxs, nc, mirror):
    ctx = ctxs[nc]
    coef, dur = LC.rising(nc, mirror=mirror)
    peak, t_peak = _peaks(ctx, coef, dur)
    end = 0.0 if mirror else _total(dur[0])
    assert (t_peak[0] == end).all(), (t_peak, end)
    LC.check_contract(coef, dur, peak, t_peak, label="falling" if mirror else "rising")
    LC.check_attained(coef, dur, peak, t_peak)
    out = ctx.eval_flat(coef, dur, np.array([end]))
    assert np.isfinite(out).all()             # the closed end is inside [0, duration]
    for q, cols in ((0, slice(3, 6)), (1, slice(6, 9))):
        v = float(np.linalg.norm(out[0, 0, cols]))
        assert abs(v - peak[0, q]) <= 1e-12 * peak[0, q] + 1e-15, (q, v, peak[0, q])


@pytest.mark.parametrize("later", [False, True])
@pytest.mark.parametrize("nc", [8, 10])
def test_a_jump_at_a_knot(ctxs, nc, later):
    """t_peak names the knot; the value is that of the segment that holds the peak (msnap_eval_flat at the knot
    evaluates the earlier one, so the value is not checked through it)."""
    coef, dur = LC.knot_jump(nc, later)
    peak, t_peak = _peaks(ctxs[nc], coef, dur)
    assert (t_peak[0] == dur[0, 0]).all(), t_peak
    LC.check_contract(coef, dur, peak, t_peak, label=f"jump, larger value {'after' if later else 'before'}")
    R = LE.peaks_R(coef[0], dur[0])
    for q in range(4):
        here = float(LE.exact_value_at(coef[0], dur[0], q, float(t_peak[0, q]), later=later))
        assert abs(peak[0, q] - here) <= LE.round_term(R[q]) + 1e-15, (q, peak[0, q], here)


# ------------------------------------------------------------------------------------------------ equioscillating
@pytest.mark.parametrize("nc", [8, 10])
def test_equioscillating_speed_and_yaw_rate(ctxs, nc):
    """x' and psi' are amp T*_{order-1}(t / T): equal extrema, two of them on the ends, coefficients some 5e4 times
    the value.  The recomputed peak is good to an ulp of sum |d_j| t^j, not of the value: the contract's r_q."""
    coef, dur = LC.equioscillating(nc)
    peak, t_peak = _peaks(ctxs[nc], coef, dur)
    LC.check_contract(coef, dur, peak, t_peak, with_R=True, label=f"order {nc - 1}")
    worst = LC.check_attained(coef, dur, peak, t_peak, label=f"order {nc - 1}")
    print(f"order {nc - 1}: worst |peak - exact at t_peak| / (2^-52 R) {worst:.3f} (C_ROUND_PEAKS {LE.C_ROUND_PEAKS})")
    # the restatement's walk has no fma, so its best time may differ; where it does not, the unfused Horner of both
    # gives the same bits
    rp, rt, _, _ = LE.fp64_walk_peaks(coef, dur)
    same = t_peak == rt
    print("kernel - restatement: peak", np.abs(peak - rp).max(), "t_peak", np.abs(t_peak - rt).max(), "same time", same.sum())
    assert same.any() and np.array_equal(peak[same], rp[same])


@pytest.mark.parametrize("nc", [8, 10])
def test_the_value_at_t_peak_deep_into_a_path(ctxs, nc):
    """1500 equioscillating segments, acceleration and jerk peak on the steep last point: the exact value at t_peak
    is off by the rounding of t_peak itself, within r_q + 2^-52 t_peak R'_q."""
    coef, dur = LC.deep_path(nc, 1500)
    peak, t_peak = _peaks(ctxs[nc], coef, dur)
    res = LE.walk_peaks(coef, dur)
    later = {(d, q) for d, q in LC.later_pairs(res, dur) if t_peak[d, q] == res.t_peak[d, q]}
    LC.check_attained(coef, dur, peak, t_peak, label=f"order {nc - 1}", later=later)
    assert (t_peak[0, 1:3] > dur[0, :-1].sum() * (1 - 1e-12)).all()          # in the last segment


# ------------------------------------------------------------------------------------------------ attained, solved paths
@pytest.mark.parametrize("nc", [8, 10])
def test_all_four_quantities_are_attained_on_a_solved_swarm(ctxs, solved, nc):
    coef, dur, peak, t_peak = solved(ctxs[nc], nc)
    worst = LC.check_attained(coef, dur, peak, t_peak, label=f"order {nc - 1}")
    print(f"order {nc - 1}: worst |peak - exact at t_peak| / (2^-52 R) {worst:.3f}")
    assert worst < 1.0            # (a solved path: within an ulp of R_q; tests/test_limits_gpu.py has the contract)


# ------------------------------------------------------------------------------------------------ scales
@pytest.mark.parametrize("scale_t,scale_w", LC.SCALES)
@pytest.mark.parametrize("nc", [8, 10])
def test_extreme_scales(ctxs, solve, nc, scale_t, scale_w):
    coef, dur = LC.scaled(solve, nc, scale_t, scale_w, n=2)          # (the root finder is slow at these scales)
    peak, t_peak = _peaks(ctxs[nc], coef, dur)
    LC.check_contract(coef, dur, peak, t_peak, with_R=True, candidates=True)
    LC.check_attained(coef, dur, peak, t_peak)


# ------------------------------------------------------------------------------------------------ a mixed batch
@pytest.mark.parametrize("nc", [8, 10])
def test_a_busy_lane_among_idle_and_failed_ones(ctxs, nc):
    ctx = ctxs[nc]
    coef, dur = LC.busy_batch(nc)
    assert coef.shape[0] * coef.shape[1] * 4 == 804 == 3 * 256 + 36
    peak, t_peak, status = ctx.dynamic_peaks(coef, dur)
    want = np.zeros(67, dtype=np.int32)
    want[13], want[40] = 3, 2
    assert np.array_equal(status, want)
    good = status == 0
    assert np.isnan(peak[~good]).all() and np.isnan(t_peak[~good]).all() and np.isfinite(peak[good]).all()
    assert (peak[2::4] == 0.0).all() and (t_peak[2::4] == 0.0).all()             # hovering
    rp, rt, rs = ctx.dynamic_peaks(coef[::-1].copy(), dur[::-1].copy())
    assert np.array_equal(rp[::-1], peak, equal_nan=True) and np.array_equal(rt[::-1], t_peak, equal_nan=True)
    assert np.array_equal(rs[::-1], status)
    for d in range(67):
        p1, t1, s1 = ctx.dynamic_peaks(coef[d:d + 1].copy(), dur[d:d + 1].copy())
        assert np.array_equal(p1[0], peak[d], equal_nan=True) and np.array_equal(t1[0], t_peak[d], equal_nan=True), d
        assert s1[0] == status[d], d
    # and the kernel stays with its restatement (the equioscillating drones: to the rounding of the attained value)
    res = LE.walk_peaks(coef, dur)
    mp_, mt, nodes, capped = res[:4]
    assert not capped.any() and nodes[0::4].max() > 50 and (nodes[1::4][good[1::4]] == 1).all()
    # the equioscillating drones' acceleration jumps at their knots: where the kernel's time is the restatement's, the
    # segment that holds the peak is the restatement's
    later = {(d, q) for d, q in LC.later_pairs(res, dur) if t_peak[d, q] == mt[d, q]}
    idx = np.nonzero(good)[0]
    later = {(int(np.nonzero(idx == d)[0][0]), q) for d, q in later}
    worst = LC.check_attained(coef[good], dur[good], peak[good], t_peak[good], label=f"order {nc - 1}", later=later)
    print(f"order {nc - 1}: worst of the value at t_peak beyond the time term {worst:.3f} x 2^-52 R (C_ROUND_PEAKS {LE.C_ROUND_PEAKS})")
    R = np.stack([LE.peaks_R(coef[d], dur[d]) for d in np.nonzero(good)[0]])
    assert (np.abs(peak[good] - mp_[good]) <= 1e-9 * mp_[good] + 1e-12 + LE.round_term(R)).all()


# ------------------------------------------------------------------------------------------------ status
@pytest.mark.parametrize("nc", [8, 10])
def test_every_documented_status(ctxs, solved, nc):
    ctx = ctxs[nc]
    coef, dur, peak0, t0 = solved(ctx, nc)

    def put(d, what):
        what(coef[d], dur[d])

    def set_dur(i, v):
        return lambda c, t: t.__setitem__(i, v)

    def set_coef(idx, v):
        return lambda c, t: c.__setitem__(idx, v)
    put(0, set_dur(1, np.inf))
    put(1, set_dur(3, np.nan))
    put(2, set_dur(0, 0.0))
    put(3, set_dur(2, -0.0))
    put(4, set_coef((1, 0, 3), np.inf))
    put(5, set_coef((2, 3, 1), np.nan))                # yaw only
    put(6, set_coef((0, 1, 2), np.nan))                # NaN in one segment ...
    put(6, set_dur(3, -1.0))                           # ... a duration <= 0 in another
    peak, t_peak, status = ctx.dynamic_peaks(coef, dur)
    assert status.tolist() == [3, 3, 2, 2, 3, 3, 3, 0]
    assert np.isnan(peak[:7]).all() and np.isnan(t_peak[:7]).all()
    assert np.array_equal(peak[7], peak0[7]) and np.array_equal(t_peak[7], t0[7])
    # both within one segment
    coef, dur, _, _ = solved(ctx, nc)
    coef[0, 2, 1, 4] = np.nan
    dur[0, 2] = 0.0
    coef[1, 1, 0, 0] = -np.inf
    dur[1, 1] = -2.0
    _, _, status = ctx.dynamic_peaks(coef, dur)
    assert status.tolist() == [3, 3, 0, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ retiming
@pytest.mark.parametrize("nc", [8, 10])
def test_retiming_by_powers_of_two_is_exact(ctxs, solved, nc):
    ctx = ctxs[nc]
    coef, dur, peak0, t0 = solved(ctx, nc)
    for k in (2.0, 0.5, 8.0):
        c2, d2 = ctx.time_scale(coef, dur, np.full(8, k))
        assert np.array_equal(c2, coef * k ** -np.arange(nc)) and np.array_equal(d2, dur * k)
        peak, t_peak = _peaks(ctx, c2, d2)
        assert np.array_equal(peak, peak0 * k ** -EXPO), (k, peak, peak0)
        assert np.array_equal(t_peak, t0 * k), (k, t_peak, t0)


@pytest.mark.parametrize("nc", [8, 10])
def test_time_scale_passes_improper_scales_through(ctxs, solved, nc):
    ctx = ctxs[nc]
    coef, dur, _, _ = solved(ctx, nc)
    scale = np.array([0.0, 2.5, -1.0, np.nan, 0.7, np.inf, -np.inf, 1.0])
    c2, d2 = ctx.time_scale(coef, dur, scale)
    for d in (0, 2, 3, 5, 6, 7):
        assert c2[d].tobytes() == coef[d].tobytes() and d2[d].tobytes() == dur[d].tobytes(), d
    for d in (1, 4):                                  # neighbours with a proper scale: as alone
        c1, d1 = ctx.time_scale(coef[d:d + 1], dur[d:d + 1], scale[d:d + 1])
        assert np.array_equal(c2[d], c1[0]) and np.array_equal(d2[d], d1[0])
        assert not np.array_equal(c2[d], coef[d])
        np.testing.assert_allclose(d2[d], dur[d] * scale[d], rtol=1e-15)
    # the host entry in place
    ci, di = coef.copy(), dur.copy()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = ctx._lib.msnap_time_scale(ctx._h, 8, 4, vp(ci), vp(di), vp(scale), vp(ci), vp(di))
    assert rc == 0
    assert ci.tobytes() == c2.tobytes() and di.tobytes() == d2.tobytes()


@pytest.mark.parametrize("q", [0, 1, 2, 3])
@pytest.mark.parametrize("nc", [8, 10])
def test_each_limit_alone(ctxs, solved, nc, q):
    """Only limits[q] is set (the others 0 or +inf, one of each).  q = 2 is the cbrt of retime_factor_kernel."""
    ctx = ctxs[nc]
    coef, dur, peak, _ = solved(ctx, nc)
    lim = np.array([0.0, np.inf, 0.0, np.inf])
    lim[q] = 0.5 * np.median(peak[:, q])
    assert 0.0 in np.delete(lim, q) and np.inf in np.delete(lim, q)
    root = (lambda x: x, np.sqrt, np.cbrt, lambda x: x)[q]
    for fit in (False, True):
        c2, d2, sc = ctx.retime_to_limits(coef, dur, *lim, fit=fit)
        k = root(peak[:, q] * (1 + 2e-9) / lim[q])
        want = np.where(k > 0.0, k, 1.0) if fit else np.maximum(k, 1.0)
        ulps = np.abs(sc - want) / np.spacing(want)
        print(f"order {nc - 1} q {q} fit {fit}: scale against NumPy, worst {ulps.max():.1f} ulp")
        np.testing.assert_allclose(sc, want, rtol=1e-14)
        assert (sc > 1.0).any()
        p2, _ = _peaks(ctx, c2, d2)
        r = np.array([LE.round_term(LE.peaks_R(c2[d], d2[d])[q]) for d in range(8)])
        print("peaks after retiming / limit - 1:", p2[:, q] / lim[q] - 1)
        assert (p2[:, q] <= lim[q] * (1 + 1e-12) + 1e-12 + r).all(), (p2[:, q], lim[q])
        if fit:
            assert (p2[:, q] >= lim[q] * (1 - 5e-9)).all(), (p2[:, q], lim[q])
        else:
            assert (sc >= 1.0).all() and (sc == 1.0).any() == bool((k <= 1.0).any())


@pytest.mark.parametrize("nc", [8, 10])
def test_common_scale_corners(ctxs, solved, nc):
    ctx = ctxs[nc]
    coef, dur, peak, _ = solved(ctx, nc)
    # COMMON without FIT, every drone's own k below 1: nothing moves
    lim = 10.0 * peak.max(axis=0)
    c2, d2, sc = ctx.retime_to_limits(coef, dur, *lim, fit=False, common=True)
    assert (sc == 1.0).all() and c2.tobytes() == coef.tobytes() and d2.tobytes() == dur.tobytes()
    own = ctx.retime_to_limits(coef, dur, *lim, fit=True)[2]
    assert (own < 1.0).all()
    # every drone failed
    bad_c, bad_d = coef.copy(), dur.copy()
    bad_c[:4, 0, 0, 0] = np.nan
    bad_d[4:, 1] = 0.0
    c3, d3, s3 = ctx.retime_to_limits(bad_c, bad_d, *lim, fit=True, common=True)
    assert np.isnan(s3).all() and c3.tobytes() == bad_c.tobytes() and d3.tobytes() == bad_d.tobytes()


@pytest.mark.parametrize("nc", [8, 10])
def test_common_scale_held_by_the_last_drone(ctxs, nc):
    """retime_common_kernel is one workgroup of 1024 threads: 1, exactly 1024 and 1025 drones, the largest factor on the
    last one each time."""
    from drone_path_planning_python_amd.synthetic import swarm
    ctx = ctxs[nc]
    coef, dur, status = ctx.solve_batch(*swarm(1025, 1025, 2))
    assert (status == 0).all()
    for n in (1, 1024, 1025):
        c, d = coef[:n].copy(), dur[:n].copy()
        c[n - 1] *= 64.0
        own = ctx.retime_to_limits(c, d, 1.0, 1.0, fit=True)[2]
        assert int(np.argmax(own)) == n - 1 and (n == 1 or own[n - 1] > own[:n - 1].max())
        c2, d2, com = ctx.retime_to_limits(c, d, 1.0, 1.0, fit=True, common=True)
        assert (com == own[n - 1]).all()
        c1, d1 = ctx.time_scale(c, d, com)
        assert c2.tobytes() == c1.tobytes() and d2.tobytes() == d1.tobytes()


# ------------------------------------------------------------------------------------------------ stream capture
def test_captured_peaks_and_retiming_replay_to_the_eager_result(ctx7):
    """dynamic_peaks_device then retime_to_limits_device on one stream: one chain of kernels, no parallel branches."""
    import torch
    from drone_path_planning_python_amd import Context, MsnapError, synthetic
    from drone_path_planning_python_amd.context import RETIME_FIT
    dev = torch.device("cuda", 0)
    n, m = 64, 5
    coef, dur, status = ctx7.solve_batch(*synthetic.swarm(7700, n, m))
    assert (status == 0).all()
    lim = [1.0, 2.0, 5.0, 0.5]
    with Context(device_id=0, order=7, max_segments=16) as ctx:          # fresh: no scratch yet
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            tc, td = (torch.from_numpy(x).to(dev) for x in (coef, dur))
            peak = torch.empty((n, 4), dtype=torch.float64, device=dev)
            t_peak = torch.empty_like(peak)
            st = torch.empty((n,), dtype=torch.int32, device=dev)
            co, do = torch.empty_like(tc), torch.empty_like(td)
            sc = torch.empty((n,), dtype=torch.float64, device=dev)
            outs = (peak, t_peak, st, co, do, sc)

            def both():
                ctx.dynamic_peaks_device(n, m, tc, td, peak, t_peak, st)
                ctx.retime_to_limits_device(n, m, tc, td, lim, RETIME_FIT, co, do, sc)
            side.synchronize()
            # the first call inside a capture: the scratch would have to grow
            g0 = torch.cuda.CUDAGraph()
            with pytest.raises(MsnapError) as e:
                with torch.cuda.graph(g0, stream=side, capture_error_mode="thread_local"):
                    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                    ctx.dynamic_peaks_device(n, m, tc, td, peak, t_peak, st)
            assert e.value.code == -8
            ctx.set_stream(side.cuda_stream)
            both()                                                       # eagerly: the scratch has its size
            side.synchronize()
            eager = [x.cpu().numpy().copy() for x in outs]
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                both()
            ctx.set_stream(side.cuda_stream)
            for x in outs:
                x.zero_()
            g.replay()
            side.synchronize()
            for got, want in zip(outs, eager):
                assert got.cpu().numpy().tobytes() == want.tobytes()
        ctx.use_own_stream()
    assert (eager[2] == 0).all() and np.isfinite(eager[5]).all() and (eager[5] != 1.0).any()
