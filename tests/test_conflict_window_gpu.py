"""Conflict windows on the GPU (include/msnap.h, "conflict windows"): the kernel against the exact
reference (tests/conflict_exact.py) and, within t_res on the four times, against the NumPy restatement, on the cases of
tests/conflict_window_cases.py (tests/test_conflict_window_cpu.py proves that every fixture of the closing checks has
only transversal crossings); per-pair status, MSNAP_EINVAL, the bit identities on a 65-pair list, stream capture, and
swarm.conflict_windows / latest_replan_time / replan_conflict_windows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_cases as CC  # noqa: E402
import conflict_exact as KE  # noqa: E402
import conflict_window_cases as KC  # noqa: E402
import cross_clearance_cases as XC  # noqa: E402

pytestmark = pytest.mark.gpu


def _device(order=7):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute
    ctx = Context(device_id=0, order=order, max_segments=16)
    dev = torch.device("cuda", 0)
    tt = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    return ctx, DeviceCompute(ctx, torch), tt, torch


def test_one_segment_one_crossing_order7(ctx7):
    KC.check_one_crossing(ctx7, 8, restated=True)


def test_one_segment_one_crossing_order9(ctx9):
    KC.check_one_crossing(ctx9, 10, restated=True)


def test_unequal_segment_counts_and_offsets_order7(ctx7):
    KC.check_unequal(ctx7, 8, restated=True)


def test_unequal_segment_counts_and_offsets_order9(ctx9):
    KC.check_unequal(ctx9, 10, restated=True)


def test_in_conflict_at_the_start_and_at_the_end_of_the_window(ctx7):
    KC.check_ends(ctx7, restated=True)


def test_two_conflicts_in_one_pair(ctx7):
    KC.check_two_conflicts(ctx7, restated=True)


def test_never_close_is_certified_clear(ctx7):
    KC.check_never_close(ctx7)


def test_exact_tangency_is_no_conflict(ctx7):
    KC.check_tangent(ctx7)


def test_windows_disjoint_one_instant_and_inside_a_segment(ctx7):
    KC.check_windows_cases(ctx7, restated=True)


def test_far_origin_and_far_clock(ctx7):
    KC.check_far(ctx7, restated=True)


def test_threshold_zero_is_never_a_conflict(ctx7):
    KC.check_threshold_zero(ctx7)


def test_closing_gap_follows_t_res(ctx7):
    KC.check_t_res(ctx7, restated=True)


def test_identities_on_65_pairs_and_host_against_device_entry(ctx7):
    ref = KC.check_identities(ctx7)
    (ca, da, ta), (cb, db, _), pairs, thr = KC.identity_list()
    ctx, comp, tt, torch = _device()
    with ctx:
        out = comp.cross_conflict_window(tt(ca), tt(da), tt(cb), tt(db), tt(pairs), thr, t0_a=tt(ta))
        torch.cuda.synchronize()
        assert KC.same([x.cpu().numpy() for x in out], ref)
        distinct = pairs[pairs[:, 0] != pairs[:, 1]]
        out = comp.conflict_window(tt(cb), tt(db), tt(distinct), thr)
        torch.cuda.synchronize()
        assert KC.same([x.cpu().numpy() for x in out], ctx7.pair_conflict_window(cb, db, distinct, thr))
        empty = torch.zeros((0, 2), dtype=torch.int32, device=torch.device("cuda", 0))
        assert all(x.shape == (0,) for x in comp.cross_conflict_window(tt(ca), tt(da), tt(cb), tt(db), empty, thr))
        assert all(x.shape == (0,) for x in comp.conflict_window(tt(cb), tt(db), empty, thr))


def test_per_pair_status_precedence_and_guarded_buffers(ctx7):
    (ca, da, ta), (cb, db, _), _, thr = KC.unequal()
    good_pairs = XC.ALL15
    good = ctx7.cross_conflict_window(ca, da, cb, db, good_pairs, thr, t0_a=ta)
    ca, da, ta, cb, db, tb = ca.copy(), da.copy(), ta.copy(), cb.copy(), db.copy(), np.zeros(6)
    ca[4, 1, 3, 2] = np.nan           # (the yaw axis: any coefficient of the drone counts)
    db[5, 7] = 0.0
    tb[4] = np.nan
    da[5, 0] = -1.0
    pairs = np.array([(0, 1), (-1, 2), (0, 2), (3, 6), (6, 3), (2, 2), (1, 5), (4, 5), (4, -1), (0, 4), (5, 4), (5, 5), (5, 3)],
                     dtype=np.int32)
    #       ok      PAIR     ok      PAIR    PAIR    ok      TIMES   NONFIN  PAIR     NONFIN  NONFIN  TIMES   TIMES
    want = [0, 4, 0, 4, 4, 0, 2, 3, 4, 3, 3, 2, 2]
    G = 1024                          # guard margins around every input on the device
    ctx, comp, tt, torch = _device()
    with ctx:
        dev = torch.device("cuda", 0)
        arrs, bufs = (ca, da, ta, cb, db, tb), []
        for arr in arrs:
            g = torch.full((arr.size + 2 * G,), -7.25e300, dtype=torch.float64, device=dev)
            g[G:G + arr.size] = torch.from_numpy(arr.reshape(-1)).to(dev)
            bufs.append(g)
        v = [b[G:G + a.size].view(a.shape) for b, a in zip(bufs, arrs)]
        out = comp.cross_conflict_window(v[0], v[1], v[3], v[4], tt(pairs), thr, t0_a=v[2], t0_b=v[5])
        torch.cuda.synchronize()
        out = [x.cpu().numpy() for x in out]
        for g, arr in zip(bufs, arrs):
            g = g.cpu().numpy()
            assert (g[:G] == -7.25e300).all() and (g[G + arr.size:] == -7.25e300).all()
            assert np.array_equal(g[G:G + arr.size], arr.reshape(-1), equal_nan=True)
    assert out[6].tolist() == want
    lookup = {tuple(p): k for k, p in enumerate(good_pairs.tolist())}
    for k, (p, st) in enumerate(zip(pairs.tolist(), want)):
        if st:
            assert all(np.isnan(x[k]) for x in out[:6])
        elif tuple(p) in lookup:
            assert all(x[k] == y[lookup[tuple(p)]] for x, y in zip(out[:6], good[:6]))
        else:
            assert not any(np.isnan(x[k]) for x in out[:6])      # (2, 2): the same index in both sets is legal
    h = ctx7.cross_conflict_window(ca, da, cb, db, pairs, thr, t0_a=ta, t0_b=tb)      # the host entry gives the same
    assert KC.same(h, out)
    # the pair entry: a == b is no pair
    st = ctx7.pair_conflict_window(cb, db, np.array([(1, 1), (0, 6), (0, 1), (5, 1)], dtype=np.int32), thr)[6]
    assert st.tolist() == [4, 4, 0, 2]


def test_einval_for_a_bad_threshold_or_resolution_and_shape_errors(ctx7):
    from drone_path_planning_python_amd._lib import MsnapError
    (ca, da, ta), (cb, db, _), pairs, thr = KC.unequal()
    for threshold, t_res in ((-0.1, 1e-6), (np.nan, 1e-6), (np.inf, 1e-6), (thr, 0.0), (thr, -1e-6), (thr, np.inf),
                             (thr, np.nan)):
        for n_pairs in (len(pairs), 0):
            with pytest.raises(MsnapError) as err:
                ctx7.cross_conflict_window(ca, da, cb, db, pairs[:n_pairs], threshold, t_res, t0_a=ta)
            assert err.value.code == -1
            with pytest.raises(MsnapError) as err:
                ctx7.pair_conflict_window(cb, db, pairs[:n_pairs], threshold, t_res)
            assert err.value.code == -1
    big = ctx7.max_segments + 1
    with pytest.raises(MsnapError):
        ctx7.cross_conflict_window(ca, da, np.zeros((2, big, 4, 8)), np.ones((2, big)), pairs[:1], thr)
    out = ctx7.cross_conflict_window(ca, da, cb, db, np.zeros((0, 2), dtype=np.int32), thr)
    assert all(x.shape == (0,) for x in out)
    assert (ctx7.pair_conflict_window(cb, db, pairs, 0.0)[1] == np.inf).all()          # threshold 0 is legal


def test_a_captured_call_replays_and_a_capture_that_would_grow_the_scratch_is_refused():
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd._lib import MsnapError
    dev = torch.device("cuda", 0)
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        ca, da = KC.solve(*XC.swarm(7501, 32, 3), 8)
        cb, db = KC.solve(*XC.swarm(7502, 64, 5), 8)
        rng = np.random.default_rng(5)
        pairs = np.stack([rng.integers(0, 32, size=300), rng.integers(0, 64, size=300)], axis=1).astype(np.int32)
        ta = rng.uniform(0.0, 2.0, size=32)
        eager = ctx.cross_conflict_window(ca, da, cb, db, pairs, 3.0, 1e-6, t0_a=ta)
        assert (eager[6] == 0).all() and np.isfinite(eager[1]).any()
        side = torch.cuda.Stream()
        P = pairs.shape[0]
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            tca, tda, tta, tcb, tdb, tp = (torch.from_numpy(x).to(dev) for x in (ca, da, ta, cb, db, pairs))
            outs = [torch.empty((P,), dtype=torch.float64, device=dev) for _ in range(6)]
            outs.append(torch.empty((P,), dtype=torch.int32, device=dev))
            args = (32, 3, tca, tda, tta, 64, 5, tcb, tdb, None, P, tp, 3.0, 1e-6, *outs)
            ctx.cross_conflict_window_device(*args)                   # once eagerly: the scratch has its size
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                ctx.cross_conflict_window_device(*args)
            ctx.set_stream(side.cuda_stream)
            for _ in range(2):
                for x in outs:
                    x.zero_()
                g.replay()
                side.synchronize()
                for got, want in zip(outs, eager):
                    assert np.array_equal(got.cpu().numpy(), want)
            # the first call of a longer list inside a capture: the scratch would have to grow
            tp2 = tp.repeat(4, 1).contiguous()
            outs2 = [torch.empty((4 * P,), dtype=torch.float64, device=dev) for _ in range(6)]
            outs2.append(torch.empty((4 * P,), dtype=torch.int32, device=dev))
            g2 = torch.cuda.CUDAGraph()
            with pytest.raises(MsnapError) as err:
                with torch.cuda.graph(g2, stream=side, capture_error_mode="thread_local"):
                    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                    ctx.cross_conflict_window_device(32, 3, tca, tda, tta, 64, 5, tcb, tdb, None, 4 * P, tp2, 3.0, 1e-6,
                                                     *outs2)
            assert err.value.code == -8                              # MSNAP_ECAPTURE
            ctx.set_stream(side.cuda_stream)
        ctx.use_own_stream()


def test_swarm_conflict_windows_and_latest_replan_time_on_12_drones_2_crossings():
    from drone_path_planning_python_amd.swarm import certify_clearance, conflict_windows, latest_replan_time
    coef, dur = CC.awkward_swarm(KC.solve, offset=0.0)
    ctx, comp, tt, torch = _device()
    with ctx:
        tc, td = tt(coef), tt(dur)
        cres = certify_clearance(comp, tc, td, CC.AWKWARD_RADIUS, CC.AWKWARD_DT, CC.AWKWARD_SAMPLES)
        res = conflict_windows(comp, cres, tc, td, CC.AWKWARD_RADIUS)
        t_r = latest_replan_time(res, 0.3)
        torch.cuda.synchronize()
        KC.check_swarm_windows(res, t_r, coef, dur, 0.3)


def test_replan_conflict_windows_on_12_drones_3_replanned():
    from drone_path_planning_python_amd.swarm import replan_conflict_windows
    coef, dur, new_coef, new_dur = XC.replan_swarm(KC.solve)
    ctx, comp, tt, torch = _device()
    with ctx:
        res = replan_conflict_windows(comp, tt(coef), tt(dur), XC.REPLAN_IDX, tt(np.array(XC.REPLAN_T_R)), tt(new_coef),
                                      tt(new_dur), XC.REPLAN_RADIUS)
        torch.cuda.synchronize()
        KC.check_replan_windows(res, coef, dur, new_coef, new_dur)
