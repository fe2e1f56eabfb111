"""Dynamic limits on the GPU (include/msnap.h, "dynamic limits"): certified peaks against the exact reference
(tests/limits_exact.py), a case a sampled check misses, a large batch against the fp64 reference, determinism, edge
cases, the exactness of the uniform retiming against fresh solves, the limits after retiming, and the node path."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, norm_rel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limits_exact as LE  # noqa: E402

pytestmark = pytest.mark.gpu


def _solved(ctx, cfg, n, m, t0=0.0):
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(cfg, n, m)
    t = t + t0
    coef, dur, status = ctx.solve_batch(wp, t)
    assert (status == 0).all()
    return wp, t, coef, dur


def _check_exact(ctx, coef, dur):
    peak, t_peak, status = ctx.dynamic_peaks(coef, dur)
    assert (status == 0).all()
    for d in range(coef.shape[0]):
        S, _ = LE.exact_peaks(coef[d], dur[d], LE.candidate_segments(coef[d], dur[d]))
        for q in range(4):
            assert LE.in_contract(peak[d, q], S[q]), (d, q, peak[d, q], float(S[q]))
    # attained: eval_flat at t_peak gives the speed and the acceleration back
    for q, cols in ((0, slice(3, 6)), (1, slice(6, 9))):
        for d in range(coef.shape[0]):
            out = ctx.eval_flat(coef[d:d + 1], dur[d:d + 1], t_peak[d:d + 1, q])
            v = float(np.linalg.norm(out[0, 0, cols]))
            assert abs(v - peak[d, q]) <= 1e-12 * peak[d, q] + 1e-15, (q, d, v, peak[d, q])
        assert (t_peak[:, q] >= 0).all() and (t_peak[:, q] <= dur.sum(axis=1) * (1 + 1e-15)).all()
    return peak, t_peak


@pytest.mark.parametrize("m,n", [(1, 8), (2, 8), (10, 10), (49, 6)])
def test_peaks_meet_the_contract_order7(ctx7, m, n):
    _, _, coef, dur = _solved(ctx7, 700 + m, n, m)
    _check_exact(ctx7, coef, dur)


@pytest.mark.parametrize("m,n", [(4, 6), (10, 6), (20, 4)])
def test_peaks_meet_the_contract_order9(ctx9, m, n):
    _, _, coef, dur = _solved(ctx9, 900 + m, n, m)
    _check_exact(ctx9, coef, dur)


def test_a_sampled_check_misses_what_the_peaks_find(ctx7):
    """One 30 ms segment between 250 ms ones: the maximum of eval_flat on the node's 0.1 s sampling grid
    under-reports the speed by several percent; dynamic_peaks meets the contract."""
    from drone_path_planning_python_amd.synthetic import SAMPLE_DT
    t = np.array([0.0, 0.25, 0.513, 0.543, 0.793, 1.043])
    wp = np.zeros((2, 6, 4))
    wp[0, :, 0] = [0, 0, 0, 1, 1, 1]
    wp[1, :, 1] = [0, 1, 0, 1, 0, 1]
    coef, dur, status = ctx7.solve_batch(wp, t)
    assert (status == 0).all()
    peak, _, _ = ctx7.dynamic_peaks(coef, dur)
    ts = np.arange(0.0, float(dur[0].sum()), SAMPLE_DT)
    sampled = np.linalg.norm(ctx7.eval_flat(coef, dur, ts)[:, :, 3:6], axis=2).max(axis=1)
    for d in range(2):
        S, _ = LE.exact_peaks(coef[d], dur[d])
        assert LE.in_contract(peak[d, 0], S[0])
        assert sampled[d] < 0.99 * float(S[0]), (sampled[d], float(S[0]))


def test_large_batch_against_the_fp64_reference(ctx7):
    _, _, coef, dur = _solved(ctx7, 4096, 4096, 20)
    peak, _, status = ctx7.dynamic_peaks(coef, dur)
    assert (status == 0).all()
    ref = LE.fp64_peaks(coef, dur)
    np.testing.assert_allclose(peak, ref, rtol=1e-9, atol=1e-12)
    _, _, coef, dur = _solved(ctx7, 100, 3, 100)              # more segments than a wave has lanes
    peak, _, status = ctx7.dynamic_peaks(coef, dur)
    assert (status == 0).all()
    np.testing.assert_allclose(peak, LE.fp64_peaks(coef, dur), rtol=1e-9, atol=1e-12)


def test_results_are_bit_identical_across_positions_batches_and_entries(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    _, _, coef, dur = _solved(ctx7, 31, 4096, 10)
    one_c, one_d = coef[17:18].copy(), dur[17:18].copy()
    p1, t1, s1 = ctx7.dynamic_peaks(one_c, one_d)
    for pos in (0, 63, 64, 4095):
        c, d = coef.copy(), dur.copy()
        c[pos], d[pos] = one_c[0], one_d[0]
        p, t, s = ctx7.dynamic_peaks(c, d)
        assert np.array_equal(p[pos], p1[0]) and np.array_equal(t[pos], t1[0]) and s[pos] == s1[0]
    p, t, s = ctx7.dynamic_peaks(np.concatenate([coef[:100], one_c]), np.concatenate([dur[:100], one_d]))
    assert np.array_equal(p[-1], p1[0]) and np.array_equal(t[-1], t1[0])
    # the device entry, on a context of its own (DeviceCompute binds it to torch's stream)
    from drone_path_planning_python_amd.swarm import DeviceCompute
    with Context(device_id=0, order=7, max_segments=256) as ctx:
        comp = DeviceCompute(ctx, torch, reuse_outputs=True)
        dev = torch.device("cuda", 0)
        pd, td, sd = comp.dynamic_peaks(torch.from_numpy(one_c).to(dev), torch.from_numpy(one_d).to(dev))
        torch.cuda.synchronize()
        assert np.array_equal(pd.cpu().numpy(), p1) and np.array_equal(td.cpu().numpy(), t1)
        assert np.array_equal(sd.cpu().numpy(), s1)


def test_edge_cases(ctx7, ctx9):
    from drone_path_planning_python_amd._lib import MsnapError
    for ctx in (ctx7, ctx9):
        nc = ctx.ncoef
        wp = np.zeros((1, 4, 4))
        wp[0, :, :3] = [1.0, -2.0, 3.0]
        wp[0, :, 3] = 0.5
        coef, dur, status = ctx.solve_batch(wp, np.array([0.0, 1.0, 2.5, 3.0]))
        assert status[0] == 0
        _, _, c2, d2 = _solved(ctx, 5, 3, 3)
        c = np.concatenate([coef, c2])
        d = np.concatenate([dur, d2])
        c[1, 1, 2, 3] = np.nan                  # what a failed solve leaves (here: one coefficient)
        d[2, 2] = -0.5
        peak, t_peak, st = ctx.dynamic_peaks(c, d)
        assert (peak[0] <= 1e-12).all() and st[0] == 0
        assert st.tolist() == [0, 3, 2, 0]
        assert np.isnan(peak[1:3]).all() and np.isnan(t_peak[1:3]).all()
        assert np.isfinite(peak[3]).all()
        for bad in ((-1.0, 0, 0, 0), (0, float("nan"), 0, 0)):
            with pytest.raises(MsnapError) as e:
                ctx.retime_to_limits(c2, d2, *bad)
            assert e.value.code == -1
        with pytest.raises(MsnapError):
            ctx.dynamic_peaks(np.zeros((1, ctx.max_segments + 1, 4, nc)), np.ones((1, ctx.max_segments + 1)))
        # failed drones pass through the retiming unchanged, scale NaN
        co, do, sc = ctx.retime_to_limits(c, d, 1.0, 1.0, fit=True, common=True)
        assert np.isnan(sc[1:3]).all() and np.isfinite(sc[[0, 3]]).all()
        assert np.array_equal(co[1:3], c[1:3], equal_nan=True) and np.array_equal(do[1:3], d[1:3])


def test_common_scale_over_more_drones_than_the_fold_has_threads(ctx7):
    """retime_common_kernel is one workgroup of 1024 threads: 1029 drones are a second, partial round of both of its
    loops.  The common scale is the exact maximum of the drones' own scales (a maximum does not round) -- here a drone
    of the partial round holds it -- and failed drones keep NaN."""
    _, _, coef, dur = _solved(ctx7, 1029, 1029, 2)
    coef, dur = coef.copy(), dur.copy()
    coef[1027] *= 64.0                        # 64 x the speed and acceleration: the largest factor of the batch
    coef[5, 0, 0, 0] = np.nan
    dur[1028, 1] = -0.5
    own = ctx7.retime_to_limits(coef, dur, 1.0, 1.0, fit=True, common=False)[2]
    bad = np.isnan(own)
    assert bad.nonzero()[0].tolist() == [5, 1028] and int(np.nanargmax(own)) == 1027
    co, do, com = ctx7.retime_to_limits(coef, dur, 1.0, 1.0, fit=True, common=True)
    assert np.isnan(com[bad]).all() and (com[~bad] == own[1027]).all()
    assert np.array_equal(co[bad], coef[bad], equal_nan=True) and np.array_equal(do[bad], dur[bad])


@pytest.mark.parametrize("order,tol", [(7, 1e-10), (9, 1e-9)])
def test_retiming_equals_a_fresh_solve_on_scaled_times(ctx7, ctx9, order, tol):
    ctx = ctx7 if order == 7 else ctx9
    rng = np.random.default_rng(order)
    for t0 in (0.0, 0.3):
        wp, t, coef, dur = _solved(ctx, 60 + order, 24, 8, t0=t0)
        k = rng.uniform(0.3, 5.0, size=24)
        c_s, d_s = ctx.time_scale(coef, dur, k)
        ref_c, ref_d, st = ctx.solve_batch(wp, t * k[:, None])
        assert (st == 0).all()
        assert norm_rel(c_s, ref_c) <= tol
        np.testing.assert_allclose(d_s, ref_d, rtol=1e-14)
        # positions at k s equal the originals at s
        s = np.linspace(0.0, 0.999 * float(dur.sum(axis=1).min()), 37)
        for dd in range(0, 24, 5):
            a = ctx.eval_flat(coef[dd:dd + 1], dur[dd:dd + 1], s)[0, :, :3]
            b = ctx.eval_flat(c_s[dd:dd + 1], d_s[dd:dd + 1], s * k[dd])[0, :, :3]
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())
        # in place on the device
        import torch
        from drone_path_planning_python_amd import Context
        with Context(device_id=0, order=order, max_segments=64) as c2:
            dev = torch.device("cuda", 0)
            tc, td = torch.from_numpy(coef).to(dev), torch.from_numpy(dur).to(dev)
            tk = torch.from_numpy(k).to(dev)
            torch.cuda.synchronize()                  # (the context launches on its own stream)
            c2.time_scale_device(24, 8, tc, td, tk, tc, td)
            c2.sync()
            assert np.array_equal(tc.cpu().numpy(), c_s) and np.array_equal(td.cpu().numpy(), d_s)


def test_limits_hold_after_retiming(ctx7, ctx9):
    for ctx in (ctx7, ctx9):
        _, _, coef, dur = _solved(ctx, 77, 40, 6)
        peak, _, _ = ctx.dynamic_peaks(coef, dur)
        lim = np.array([np.median(peak[:, 0]), np.median(peak[:, 1]) * 2, np.inf, np.median(peak[:, 3])])
        expo = np.array([1.0, 2.0, 3.0, 1.0])
        for fit in (False, True):
            c2, d2, sc = ctx.retime_to_limits(coef, dur, *lim, fit=fit)
            p2, _, st = ctx.dynamic_peaks(c2, d2)
            assert (st == 0).all()
            assert (p2[:, [0, 1, 3]] <= lim[[0, 1, 3]] * (1 + 1e-12) + 1e-12).all()
            if fit:
                binding = (p2[:, [0, 1, 3]] / lim[[0, 1, 3]]).max(axis=1)
                assert (binding >= 1 - 5e-9).all()
            else:
                assert (sc >= 1.0).all() and (d2 >= dur).all()
                relaxed = np.all(peak[:, [0, 1, 3]] * (1 + 2e-9) <= lim[[0, 1, 3]], axis=1)
                assert relaxed.any() and (sc[relaxed] == 1.0).all()
                assert np.array_equal(c2[relaxed], coef[relaxed]) and np.array_equal(d2[relaxed], dur[relaxed])
            # the factor the header states
            k = np.zeros(len(sc))
            for q in (0, 1, 3):
                k = np.maximum(k, (peak[:, q] * (1 + 2e-9) / lim[q]) ** (1 / expo[q]))
            np.testing.assert_allclose(sc, k if fit else np.maximum(k, 1.0), rtol=1e-14)
            cc, dc, scc = ctx.retime_to_limits(coef, dur, *lim, fit=fit, common=True)
            assert (scc == sc.max()).all()
            np.testing.assert_array_equal(dc, dur * sc.max())
        # unconstrained: FIT gives 1
        c3, d3, s3 = ctx.retime_to_limits(coef, dur, fit=True)
        assert (s3 == 1.0).all() and np.array_equal(c3, coef)
        # the device entry, in place, common
        import torch
        from drone_path_planning_python_amd import Context
        from drone_path_planning_python_amd.swarm import DeviceCompute
        with Context(device_id=0, order=ctx.order, max_segments=64) as cx:
            comp = DeviceCompute(cx, torch)
            dev = torch.device("cuda", 0)
            tc, td = torch.from_numpy(coef).to(dev), torch.from_numpy(dur).to(dev)
            co, do, so = comp.retime_to_limits(tc, td, list(lim), fit=True, common=True)
            torch.cuda.synchronize()
            cc, dc, scc = ctx.retime_to_limits(coef, dur, *lim, fit=True, common=True)
            assert np.array_equal(co.cpu().numpy(), cc) and np.array_equal(so.cpu().numpy(), scc)


def test_node_paths_to_pols_with_limits(ctx7):
    from drone_path_planning_python_amd.nodes import drones_pols_generator as dpg
    from drone_path_planning_python_amd.nodes import msgs
    paths = []
    for name in ("Pol_matrix_1.csv", "Pol_matrix_2.csv"):
        mat = np.loadtxt(os.path.join(GOLDEN_DIR, name), delimiter=",")
        # the reference's waypoints: every piece's start, then the last piece's end
        x = mat[:, 1:].reshape(-1, 4, 8)
        pos = np.concatenate([x[:, :3, 0], [[np.polyval(x[-1, a, ::-1], mat[-1, 0]) for a in range(3)]]])
        yaw = np.concatenate([x[:, 3, 0], [np.polyval(x[-1, 3, ::-1], mat[-1, 0])]])
        quat = np.stack([np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
        paths.append(msgs.path_from_arrays(pos, quat))
    # without limits: byte for byte what the node produced before (solve on the grid, pack)
    mat, coef, dur = dpg.paths_to_pols(paths, ctx7)
    wp, t = dpg.paths_to_waypoints(paths)
    c0, d0, _ = ctx7.solve_on_grid(t, wp)
    assert mat.tobytes() == ctx7.pack_pol_matrix(c0, d0).tobytes()
    assert np.array_equal(coef, c0) and np.array_equal(dur, d0)
    # with limits: one common scale, the packed durations are the scaled ones
    peak, _, _ = ctx7.dynamic_peaks(coef, dur)
    lim = (0.5 * peak[:, 0].max(), 0.0, 0.0, 0.0)
    mat2, coef2, dur2 = dpg.paths_to_pols(paths, ctx7, limits=lim)
    k = dur2 / dur
    assert np.allclose(k, k.flat[0], rtol=1e-15) and k.flat[0] > 1.9
    np.testing.assert_array_equal(mat2[..., 0], dur2.astype(np.float32))
    p2, _, _ = ctx7.dynamic_peaks(coef2, dur2)
    assert (p2[:, 0] <= lim[0] * (1 + 1e-12)).all()
    # the one-drone node entry
    msg = dpg.path_to_pol(paths[0], 1, ctx=ctx7, save=False, limits=lim)
    assert msg.durations[0] > mat[0, 0, 0] * 1.9
