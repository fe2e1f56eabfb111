"""Half-space windows on the GPU (include/msnap.h, "half-space windows"): the kernel against the exact
reference (tests/halfspace_exact.py) and, within t_res on the four times, against the NumPy restatement, on the cases of
tests/halfspace_cases.py (tests/test_halfspace_window_cpu.py proves that every solved fixture has only transversal
crossings); the bit identities on 65 drones x 7 planes, v_first / v_last bit for bit from msnap_eval_flat, per-query
status and guarded buffers, MSNAP_EINVAL / MSNAP_ESEGMENTS, stream capture, swarm.geofence_windows and
swarm.certify_corridor, and the corridor against msnap_mesh_clearance on the hole scene."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extent_cases as EC  # noqa: E402
import halfspace_cases as HC  # noqa: E402
import halfspace_exact as HE  # noqa: E402

pytestmark = pytest.mark.gpu


def _device(order=7):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute
    ctx = Context(device_id=0, order=order, max_segments=16)
    dev = torch.device("cuda", 0)
    tt = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    return ctx, DeviceCompute(ctx, torch), tt, torch


@pytest.fixture(params=[7, 9])
def ctx(request, ctx7, ctx9):
    return ctx7 if request.param == 7 else ctx9


def test_parabola_is_outside_on_one_quarter_to_three_quarters(ctx):
    HC.check_parabola(ctx, ctx.order, restated=True)


def test_tangency_is_never_outside(ctx7):
    HC.check_tangency(ctx7)


def test_overshoot_window_contains_t_3(ctx):
    HC.check_overshoot(ctx, ctx.order, restated=True)


def test_two_conflicts_in_one_query_give_the_first_and_the_last(ctx7):
    HC.check_two_conflicts(ctx7, restated=True)


def test_outside_at_the_start_and_at_the_end_of_the_range(ctx7):
    HC.check_ends(ctx7, restated=True)


def test_ranges_inside_a_violation_empty_and_one_instant(ctx7):
    HC.check_ranges(ctx7, restated=True)


def test_partial_segments(ctx7):
    HC.check_partial_segments(ctx7, restated=True)


def test_zero_nonfinite_and_nonunit_planes(ctx7):
    HC.check_planes(ctx7, restated=True)


def test_closing_gap_follows_t_res(ctx7):
    HC.check_t_res(ctx7, restated=True)


@pytest.mark.parametrize("name", sorted(HC.SWARMS))
def test_solved_swarms_near_far_and_long(ctx, name):
    """(check 3 of check_windows is the bit identity of v_first / v_last with msnap_eval_flat and the unfused dot product)"""
    HC.check_swarm(ctx, name, ctx.order, restated=True)


def test_identities_on_65_drones_7_planes_and_host_against_device_entry(ctx7):
    ref = HC.check_identities(ctx7)
    coef, dur, planes, queries = HC.identity_case()
    # v_first / v_last bit for bit from msnap_eval_flat and the unfused dot product, on every query that found a time
    for k in np.nonzero(np.isfinite(ref[1]))[0][::7]:
        d, p = queries[k]
        for t, v in ((ref[1][k], ref[2][k]), (ref[3][k], ref[4][k])):
            pos = ctx7.eval_flat(coef[d:d + 1], dur[d:d + 1], np.array([t]))[0, 0, :3]
            assert HE.unfused_dot(planes[p, :3], pos) == v
    ctx, comp, tt, torch = _device()
    with ctx:
        out = comp.halfspace_window(tt(coef), tt(dur), tt(planes), tt(queries))
        torch.cuda.synchronize()
        assert HC.same([x.cpu().numpy() for x in out], ref)
        total = np.add.accumulate(dur, axis=1)[:, -1]
        out = comp.halfspace_window(tt(coef), tt(dur), tt(planes), tt(queries), t_from=tt(np.zeros(len(queries))),
                                    t_to=tt(total[queries[:, 0]]))
        torch.cuda.synchronize()
        assert HC.same([x.cpu().numpy() for x in out], ref)
        empty = torch.zeros((0, 2), dtype=torch.int32, device=torch.device("cuda", 0))
        assert all(x.shape == (0,) for x in comp.halfspace_window(tt(coef), tt(dur), tt(planes), empty))
        with pytest.raises(ValueError):
            comp.halfspace_window(tt(coef), tt(dur), tt(planes[:, :3]), tt(queries))
        with pytest.raises(ValueError):
            comp.halfspace_window(tt(coef), tt(dur), tt(planes), tt(queries), t_from=tt(np.zeros(3)))


def test_per_query_status_precedence_and_guarded_buffers(ctx7):
    coef, dur, planes, _ = HC.swarm_fixture("m3", 7)[:4]
    coef, dur, planes = coef.copy(), dur.copy(), np.concatenate([planes[:2], [[1.0, np.inf, 0.0, 0.0]]])
    good = ctx7.halfspace_window(coef, dur, planes, np.array([[0, 0], [0, 1]], dtype=np.int32), 1e-6)
    coef[3, 1, 3, 2] = np.nan          # (the yaw axis: any coefficient of the drone counts)
    dur[3, 0] = -1.0
    dur[4, 2] = 0.0
    queries = np.array([(0, 0), (-1, 0), (0, 1), (5, 1), (0, 3), (0, -1), (3, 0), (4, 1), (3, 7), (0, 2), (4, 2), (1, 0), (1, 1),
                        (2, 0)], dtype=np.int32)
    t_from = np.array([0.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, np.nan, 0.0, 0.0])
    t_to = np.array([100.0, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, np.inf, 100.0])
    #       ok PAIR ok PAIR PAIR PAIR NONFIN TIMES PAIR ok(NaN) TIMES(NaN) NONFIN NONFIN ok
    want = [0, 4, 0, 4, 4, 4, 3, 2, 4, 0, 2, 3, 3, 0]
    Q, G = len(queries), 1024            # guard margins around every input and every output on the device
    ctx, comp, tt, torch = _device()
    with ctx:
        dev = torch.device("cuda", 0)

        def guarded(arr):
            fill = -7.25e300 if arr.dtype == np.float64 else -77
            g = torch.full((arr.size + 2 * G,), fill, dtype=getattr(torch, arr.dtype.name), device=dev)
            g[G:G + arr.size] = torch.from_numpy(arr.reshape(-1)).to(dev)
            return g, g[G:G + arr.size].view(arr.shape), fill

        ins = [guarded(a) for a in (coef, dur, planes, queries, t_from, t_to)]
        outs = [guarded(np.zeros(Q)) for _ in range(6)] + [guarded(np.zeros(Q, dtype=np.int32))]
        ctx.halfspace_window_device(5, 3, ins[0][1], ins[1][1], 3, ins[2][1], Q, ins[3][1], ins[4][1], ins[5][1], 1e-6,
                                    *[o[1] for o in outs])
        torch.cuda.synchronize()
        for (g, view, fill), arr in zip(ins, (coef, dur, planes, queries, t_from, t_to)):
            g = g.cpu().numpy()
            assert (g[:G] == fill).all() and (g[G + arr.size:] == fill).all()
            assert np.array_equal(g[G:G + arr.size], arr.reshape(-1), equal_nan=True)
        for g, view, fill in outs:
            g = g.cpu().numpy()
            assert (g[:G] == fill).all() and (g[G + Q:] == fill).all()
        out = [o[1].cpu().numpy() for o in outs]
    assert out[6].tolist() == want
    for k, st in enumerate(want):
        if st or k in (9, 10):
            assert all(np.isnan(x[k]) for x in out[:6]), k
        else:
            assert not any(np.isnan(x[k]) for x in out[:6]), k
    assert all(x[0] == y[0] and x[2] == y[1] for x, y in zip(out[:6], good[:6]))      # beside failed queries: the same bits
    assert HC.same(ctx7.halfspace_window(coef, dur, planes, queries, 1e-6, t_from=t_from, t_to=t_to), out)      # host entry


def test_einval_esegments_and_shape_errors(ctx7):
    from drone_path_planning_python_amd._lib import MsnapError
    coef, dur = HC.parabola(7)
    planes = HC.X_LE(0.75)
    for t_res in (0.0, -1e-6, np.inf, np.nan):
        for n in (1, 0):
            with pytest.raises(MsnapError) as err:
                ctx7.halfspace_window(coef, dur, planes, HC.Q00[:n], t_res)
            assert err.value.code == -1
    big = ctx7.max_segments + 1
    with pytest.raises(MsnapError) as err:
        ctx7.halfspace_window(np.zeros((1, big, 4, 8)), np.ones((1, big)), planes, HC.Q00)
    assert err.value.code == -4
    out = ctx7.halfspace_window(coef, dur, planes, np.zeros((0, 2), dtype=np.int32))
    assert all(x.shape == (0,) for x in out)
    # no planes at all: every plane index is out of range
    assert ctx7.halfspace_window(coef, dur, np.zeros((0, 4)), HC.Q00)[6].tolist() == [4]
    for bad_planes, bad_queries, kw in ((np.zeros((1, 3)), HC.Q00, {}), (planes, np.zeros((1, 3), dtype=np.int32), {}),
                                        (planes, HC.Q00, {"t_from": np.zeros(2)}), (planes, HC.Q00, {"t_to": np.zeros(2)})):
        with pytest.raises(ValueError):
            ctx7.halfspace_window(coef, dur, bad_planes, bad_queries, **kw)


def test_a_captured_call_replays_and_a_capture_that_would_grow_the_scratch_is_refused():
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd._lib import MsnapError
    dev = torch.device("cuda", 0)
    coef, dur, planes, queries = HC.identity_case()
    queries = queries[:300]
    rng = np.random.default_rng(6)
    t_from = rng.uniform(0.0, 2.0, size=300)
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        eager = ctx.halfspace_window(coef, dur, planes, queries, 1e-6, t_from=t_from)
        assert (eager[6] == 0).all() and np.isfinite(eager[1]).any()
        side = torch.cuda.Stream()
        Q = 300
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            tc, td, tp, tq, tf = (torch.from_numpy(x).to(dev) for x in (coef, dur, planes, queries, t_from))
            outs = [torch.empty((Q,), dtype=torch.float64, device=dev) for _ in range(6)]
            outs.append(torch.empty((Q,), dtype=torch.int32, device=dev))
            args = (65, 10, tc, td, 7, tp, Q, tq, tf, None, 1e-6, *outs)
            ctx.halfspace_window_device(*args)                        # once eagerly: the scratch has its size
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                ctx.halfspace_window_device(*args)
            ctx.set_stream(side.cuda_stream)
            for _ in range(2):
                for x in outs:
                    x.zero_()
                g.replay()
                side.synchronize()
                for got, want in zip(outs, eager):
                    assert np.array_equal(got.cpu().numpy(), want)
            # the first call of a longer list inside a capture: the scratch would have to grow
            tq2, tf2 = tq.repeat(4, 1).contiguous(), tf.repeat(4).contiguous()
            outs2 = [torch.empty((4 * Q,), dtype=torch.float64, device=dev) for _ in range(6)]
            outs2.append(torch.empty((4 * Q,), dtype=torch.int32, device=dev))
            g2 = torch.cuda.CUDAGraph()
            with pytest.raises(MsnapError) as err:
                with torch.cuda.graph(g2, stream=side, capture_error_mode="thread_local"):
                    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                    ctx.halfspace_window_device(65, 10, tc, td, 7, tp, 4 * Q, tq2, tf2, None, 1e-6, *outs2)
            assert err.value.code == -8                               # MSNAP_ECAPTURE
            ctx.set_stream(side.cuda_stream)
        ctx.use_own_stream()


def test_swarm_geofence_windows_on_12_drones_of_which_some_overshoot_the_box():
    from drone_path_planning_python_amd.swarm import certify_geofence, geofence_windows, latest_replan_time
    coef, dur = HC.overshoot_swarm(np.linspace(0.3, 1.2, 12))
    ctx, comp, tt, torch = _device()
    with ctx:
        tc, td = tt(coef), tt(dur)
        geo = certify_geofence(comp, tc, td, lo=EC.BOX_LO, hi=EC.BOX_HI)
        res = geofence_windows(comp, geo, tc, td)
        t_r = latest_replan_time(res, 0.3)
        torch.cuda.synchronize()
        cpu = lambda x: x.cpu().numpy()      # noqa: E731
        out = cpu(geo.outside)
        first, last, until, frm, broken = (cpu(x) for x in (res.first_conflict, res.last_conflict, res.inside_until,
                                                             res.inside_from, res.first_broken))
        t_r, idx = cpu(t_r), cpu(res.idx)
    assert 0 < out.sum() < 12 and idx.tolist() == np.nonzero(out | cpu(geo.undecided))[0].tolist()
    ref_geo = certify_geofence(HE.RestatedCompute(), torch.from_numpy(coef), torch.from_numpy(dur), lo=EC.BOX_LO, hi=EC.BOX_HI)
    ref = geofence_windows(HE.RestatedCompute(), ref_geo, torch.from_numpy(coef), torch.from_numpy(dur))
    assert ref_geo.outside.numpy().tolist() == out.tolist() and ref.first_broken.numpy().tolist() == broken.tolist()
    for got, want in ((first, ref.first_conflict), (last, ref.last_conflict), (until, ref.inside_until), (frm, ref.inside_from)):
        want = want.numpy()
        assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.allclose(got[out], want[out], rtol=0, atol=2e-6)
    assert (until[out] <= first[out]).all() and (first[out] < last[out]).all() and (last[out] <= frm[out]).all()
    assert np.isinf(first[~out]).all() and (broken[~out] == -1).all() and (broken[out] >= 0).all()
    assert np.array_equal(t_r[out], np.maximum(first[out] - 0.3, 0.0)) and np.isinf(t_r[~out]).all()


def test_certify_corridor_through_the_hole_and_the_mesh_clearance_of_the_drones_certified_inside():
    """Two independent kernels: a drone certified INSIDE the three-box corridor at radius r has msnap_mesh_clearance's
    lower >= r less the two allowances.  The stand-in and the restated mesh clearance decide every drone first (no
    UNDECIDED verdict, and every certified lower at least 0.05 m from the radius)."""
    import mesh_clearance_exact as ME
    from drone_path_planning_python_amd import stl
    from drone_path_planning_python_amd.swarm import CORRIDOR_INSIDE, certify_corridor
    tris = np.ascontiguousarray(stl.load_stl(os.path.join(GOLDEN_DIR, "env-scene-hole.stl")), dtype=np.float64)
    planes, off = HC.hole_corridor(tris)
    coef, dur = HC.hole_flights()
    r = HC.HOLE_RADIUS
    import torch
    ref = certify_corridor(HE.RestatedCompute(), torch.from_numpy(coef), torch.from_numpy(dur), torch.from_numpy(planes), off,
                           [0, 1, 2], radius=r)
    assert ref.verdict.tolist() == HC.HOLE_VERDICTS and ref.stage.tolist() == HC.HOLE_STAGES
    ref_lower = ME.fp64_mesh_clearance(coef, dur, tris)[3]
    assert (np.abs(ref_lower - r) > 0.05).all()
    ctx, comp, tt, torch = _device()
    with ctx:
        res = certify_corridor(comp, tt(coef), tt(dur), tt(planes), off, [0, 1, 2], radius=r)
        torch.cuda.synchronize()
        verdict, stage, plane = (x.cpu().numpy() for x in (res.verdict, res.stage, res.plane))
        handover, first = res.handover.cpu().numpy(), res.first_conflict.cpu().numpy()
        md, tm, tri, lower, st = ctx.mesh_clearance(coef, dur, tris)
    assert verdict.tolist() == HC.HOLE_VERDICTS and stage.tolist() == HC.HOLE_STAGES
    assert plane.tolist() == ref.plane.tolist()
    assert np.array_equal(np.isnan(handover), np.isnan(ref.handover.numpy()))
    assert np.allclose(np.nan_to_num(handover), np.nan_to_num(ref.handover.numpy()), rtol=0, atol=2e-6)
    assert np.allclose(first[verdict == 1], ref.first_conflict.numpy()[verdict == 1], rtol=0, atol=2e-6)
    assert (st == 0).all()
    for d in np.nonzero(verdict == CORRIDOR_INSIDE)[0]:
        allow = ME.round_terms(ME.mesh_R(coef[d], dur[d], tris)) + max(HE.allowance(coef[d], dur[d], p[:3]) for p in planes)
        assert lower[d] >= r - allow, (d, lower[d])
    assert (lower[verdict != CORRIDOR_INSIDE] < r).all()          # and the drones it stopped do meet the wall
