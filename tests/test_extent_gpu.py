"""Path extent on the GPU (include/msnap.h, "path extent"): closed forms, the position of the maximum in the path, the
contract against the exact reference (tests/extent_exact.py) on every family of tests/extent_cases.py, the attained
claim bit for bit, bit identity, certify_geofence on the motivating overshoot, failures and arguments, stream capture."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extent_cases as EC  # noqa: E402
import extent_exact as EE  # noqa: E402

pytestmark = pytest.mark.gpu


def _ctx(ctx7, ctx9, order):
    return ctx7 if order == 7 else ctx9


def _attained(ctx, coef, dur, dirs, ext, t_ext):
    """msnap_eval_flat at t_ext, then the unfused dot, is ext bit for bit; 0 <= t_ext <= the total"""
    total = np.add.accumulate(dur, axis=1)[:, -1]
    assert (t_ext >= 0.0).all() and (t_ext <= total[:, None]).all()
    for d in range(ext.shape[0]):
        pos = ctx.eval_flat(coef[d:d + 1], dur[d:d + 1], t_ext[d])[0, :, :3]
        assert np.array_equal(EE.unfused_dot(dirs, pos), ext[d]), (d, ext[d], pos)


@pytest.mark.parametrize("order", [7, 9])
def test_closed_forms(ctx7, ctx9, order):
    ctx = _ctx(ctx7, ctx9, order)
    for T in (1.0, 3.0):
        coef, dur = EC.parabola(order, T)
        ext, t_ext, upper, st = ctx.path_extent(coef, dur, EC.AXES[:2])
        print("parabola", T, ext, t_ext, upper)
        assert st[0] == 0
        if T == 1.0:
            assert ext[0, 0] == 0.25 and t_ext[0, 0] == 0.5
        assert abs(ext[0, 0] - 0.25) <= 1e-15 and abs(t_ext[0, 0] - T / 2) <= 1e-7 * T
        assert ext[0, 1] == 0.0 and t_ext[0, 1] == 0.0            # the tie with t = T goes to the earlier time
        for k in range(2):
            r = EE.round_terms(EE.extent_R(coef[0], dur[0], EC.AXES[k]))
            assert ext[0, k] <= upper[0, k] <= ext[0, k] + 1e-9 * abs(ext[0, k]) + 1e-9 + r
        _attained(ctx, coef, dur, EC.AXES[:2], ext, t_ext)


@pytest.mark.parametrize("order", [7, 9])
def test_position_of_the_maximum_in_the_path(ctx7, ctx9, order):
    ctx = _ctx(ctx7, ctx9, order)
    for name in EC.HAND:
        coef, dur, dirs, S, t = EC.hand_case(name, order)
        ext, t_ext, upper, _ = EE.check_contract(ctx.path_extent, ctx.eval_flat, coef, dur, dirs)
        print(name, ext, t_ext, upper)
        assert ext[0, 0] == S and t_ext[0, 0] == t, name
    coef, dur, dirs = EC.constant_path(order)
    ext, t_ext, upper, st = ctx.path_extent(coef, dur, dirs)
    want = EE.unfused_dot(dirs, coef[0, 0, :3, 0][None, :])
    assert st[0] == 0 and np.array_equal(ext[0], want) and np.array_equal(upper[0], want) and (t_ext == 0.0).all()


@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("name", sorted(EC.SWARMS))
def test_contract_against_the_exact_reference(ctx7, ctx9, name, order):
    ctx = _ctx(ctx7, ctx9, order)
    coef, dur, dirs = EC.swarm_case(name, order)
    # (check_contract prints the kernel's worst rounding ratio and asserts it below C_ROUND_EXTENT, and checks the
    # attained claim of every (drone, direction) through msnap_eval_flat)
    ext, t_ext, upper, _ = EE.check_contract(ctx.path_extent, ctx.eval_flat, coef, dur, dirs, pick=EC.PICK.get(name))
    rext, rt, rupper = EE.fp64_extent(coef, dur, dirs)
    R = np.array([[EE.extent_R(coef[d], dur[d], n) for n in dirs] for d in range(len(coef))])
    print("kernel - restatement: ext", np.abs(ext - rext).max(), "upper", np.abs(upper - rupper).max())
    assert (np.abs(ext - rext) <= 1e-9 * np.abs(rext) + EE.ABS_CLOSE + EE.round_terms(R)).all()
    assert (np.abs(upper - rupper) <= 1e-9 * np.abs(rupper) + EE.ABS_CLOSE + EE.round_terms(R)).all()


def test_bit_identity_across_batch_place_size_direction_place_and_entry(ctx7):
    import torch
    coef, dur, dirs = EC.swarm_case("near_n65_m10_k7", 7)
    whole = ctx7.path_extent(coef, dur, dirs)
    assert (whole[3] == 0).all()
    for d in (0, 63, 64):
        alone = ctx7.path_extent(coef[d:d + 1], dur[d:d + 1], dirs)
        for a, w in zip(alone[:3], whole[:3]):
            assert np.array_equal(a[0], w[d]), d
        first = ctx7.path_extent(coef[d:d + 1], dur[d:d + 1], dirs[6:7])             # the last of 7 directions, alone
        moved = ctx7.path_extent(coef[d:d + 1], dur[d:d + 1], np.ascontiguousarray(dirs[::-1]))      # ... and first of 7
        for f, m, w in zip(first[:3], moved[:3], whole[:3]):
            assert f[0, 0] == w[d, 6] and m[0, 0] == w[d, 6] and m[0, 6] == w[d, 0], d
    dev = torch.device("cuda", 0)
    tc, td, tn = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (coef, dur, dirs))
    ext = torch.empty((65, 7), dtype=torch.float64, device=dev)
    te, up = torch.empty_like(ext), torch.empty_like(ext)
    st = torch.empty((65,), dtype=torch.int32, device=dev)
    ctx7.path_extent_device(65, 10, tc, td, 7, tn, ext, te, up, st)
    ctx7.sync()
    for got, w in zip((ext, te, up, st), whole):
        assert np.array_equal(got.cpu().numpy(), w)


@pytest.mark.parametrize("order", [7, 9])
def test_certify_geofence_on_the_fit_that_leaves_the_workspace(order):
    import torch
    from drone_path_planning_python_amd import Context, swarm as sw
    wp, t = EC.overshoot_waypoints()
    with Context(device_id=0, order=order, max_segments=16) as ctx:
        comp = sw.DeviceCompute(ctx, torch)
        coef, dur, st = comp.solve(torch.from_numpy(wp).cuda(), torch.from_numpy(t).cuda())
        res = sw.certify_geofence(comp, coef, dur, lo=EC.BOX_LO, hi=EC.BOX_HI, status=st)
        k = int(res.worst[0])
        print("verdict", res.verdict, "wall", res.normals[k], res.limits[k], "t", res.t_worst, "excess", res.excess)
        assert bool(res.outside[0]) and int(res.verdict[0]) == sw.GEOFENCE_OUTSIDE
        assert res.normals[k].tolist() == [1.0, 0.0, 0.0] and float(res.limits[k]) == 2.2      # through the x = 2.2 wall
        assert abs(float(res.t_worst[0]) - 3.0) <= 1e-6
        assert abs(float(res.excess[0]) - (EC.OVERSHOOT_MAX_X[order] - 2.2)) < 5e-5
        assert float(res.box_hi[0, 0]) >= float(res.ext[0, 0]) > 3.0
        # a swarm shrunk well inside a wide box is all inside
        c2, d2, dirs = EC.swarm_case("near_n5_m3_k7", order)
        tc, td = torch.from_numpy(0.01 * c2).cuda(), torch.from_numpy(d2).cuda()
        res = sw.certify_geofence(comp, tc, td, lo=[-50.0, -50.0, -50.0], hi=[50.0, 50.0, float("inf")], radius=0.5,
                                  planes=[[1.0, 1.0, 0.0, 60.0]])
        assert bool(res.inside.all()) and res.normals.shape[0] == 6 and (res.box_lo <= res.box_hi).all()
        # a limit equal to a drone's own ext: attained, so never certified inside
        n = torch.from_numpy(dirs[6]).cuda()
        ext, _, upper, _ = comp.path_extent(tc, td, n[None, :])
        e0 = float(ext[0, 0])
        res = sw.certify_geofence(comp, tc, td, planes=[[*dirs[6].tolist(), e0]])
        assert int(res.verdict[0]) in (sw.GEOFENCE_UNDECIDED, sw.GEOFENCE_OUTSIDE) and not bool(res.inside[0])
        # a failed drone is refused
        stat = torch.zeros(5, dtype=torch.int32)
        stat[2] = 3
        res = sw.certify_geofence(comp, tc, td, lo=[-50.0] * 3, hi=[50.0] * 3, status=stat)
        assert res.verdict.tolist() == [0, 0, sw.GEOFENCE_FAILED, 0, 0] and bool(res.failed[2]) and int(res.worst[2]) == -1


def test_failed_drones_directions_and_argument_errors(ctx7):
    coef, dur, dirs = EC.swarm_case("near_n5_m3_k7", 7)
    coef, dur = coef[:3].copy(), dur[:3].copy()
    good = ctx7.path_extent(coef, dur, dirs)
    for what in ("nan", "zero duration"):
        c, d = coef.copy(), dur.copy()
        if what == "nan":
            c[1, 2, 3, 1] = np.nan                             # (yaw: a failed solve leaves every axis NaN)
        else:
            d[1, 1] = 0.0
        ext, t_ext, upper, st = ctx7.path_extent(c, d, dirs)
        assert st.tolist() == [0, 3 if what == "nan" else 2, 0], what
        assert np.isnan(ext[1]).all() and np.isnan(t_ext[1]).all() and np.isnan(upper[1]).all()
        for got, want in zip((ext, t_ext, upper), good):       # the neighbours' outputs are unchanged bit for bit
            assert np.array_equal(got[[0, 2]], want[[0, 2]]), what
    odd = dirs.copy()
    odd[2] = [0.0, np.inf, 0.0]
    odd[4] = 0.0
    ext, t_ext, upper, st = ctx7.path_extent(coef, dur, odd)
    assert (st == 0).all() and np.isnan(ext[:, 2]).all() and np.isnan(t_ext[:, 2]).all() and np.isnan(upper[:, 2]).all()
    assert (ext[:, 4] == 0.0).all() and (upper[:, 4] == 0.0).all() and (t_ext[:, 4] == 0.0).all()
    keep = [0, 1, 3, 5, 6]
    for got, want in zip((ext, t_ext, upper), good):
        assert np.array_equal(got[:, keep], want[:, keep])
    ext, t_ext, upper, st = ctx7.path_extent(coef, dur, np.zeros((0, 3)))      # n_dirs == 0: a no-op
    assert ext.shape == (3, 0)
    lib, h = ctx7._lib, ctx7._h
    z = np.zeros(64)
    p = z.ctypes.data
    assert lib.msnap_path_extent(None, 1, 1, p, p, 1, p, p, p, p, p) == -1
    assert lib.msnap_path_extent(h, -1, 1, p, p, 1, p, p, p, p, p) == -1
    assert lib.msnap_path_extent(h, 1, 1, p, p, -1, p, p, p, p, p) == -1
    assert lib.msnap_path_extent(h, 1, 1, p, p, 1, None, p, p, p, p) == -1
    assert lib.msnap_path_extent(h, 1, 1, None, p, 1, p, p, p, p, p) == -1
    assert lib.msnap_path_extent(h, 1, 1, p, p, 1, p, p, None, p, p) == -1
    assert lib.msnap_path_extent_device(h, 1, 1, p, p, 1, p, p, p, p, None) == -1
    assert lib.msnap_path_extent(h, 2 ** 30, 1, p, p, 2 ** 30, p, p, p, p, p) == -1      # the lanes' grid does not fit
    assert lib.msnap_path_extent(h, 1, 0, p, p, 1, p, p, p, p, p) == -4
    assert lib.msnap_path_extent(h, 1, 4097, p, p, 1, p, p, p, p, p) == -4
    assert lib.msnap_path_extent(h, 0, 1, None, None, 1, None, None, None, None, None) == 0
    assert lib.msnap_path_extent(h, 1, 1, None, None, 0, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        ctx7.path_extent(coef, dur, dirs[:, :2])


def test_a_captured_call_replays_to_the_eager_result():
    import torch
    from drone_path_planning_python_amd import Context, MsnapError
    dev = torch.device("cuda", 0)
    coef, dur, dirs = EC.swarm_case("near_n65_m10_k7", 7)
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            tc, td, tn = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (coef, dur, dirs))
            ext = torch.empty((65, 7), dtype=torch.float64, device=dev)
            te, up = torch.empty_like(ext), torch.empty_like(ext)
            st = torch.empty((65,), dtype=torch.int32, device=dev)
            side.synchronize()
            # the first call inside a capture: the scratch would have to grow
            g0 = torch.cuda.CUDAGraph()
            with pytest.raises(MsnapError) as e:
                with torch.cuda.graph(g0, stream=side, capture_error_mode="thread_local"):
                    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                    ctx.path_extent_device(65, 10, tc, td, 7, tn, ext, te, up, st)
            assert e.value.code == -8
            ctx.set_stream(side.cuda_stream)
            ctx.path_extent_device(65, 10, tc, td, 7, tn, ext, te, up, st)      # eagerly: the scratch has its size
            side.synchronize()
            eager = [x.cpu().numpy().copy() for x in (ext, te, up, st)]
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                ctx.path_extent_device(65, 10, tc, td, 7, tn, ext, te, up, st)
            ctx.set_stream(side.cuda_stream)
            for x in (ext, te, up, st):
                x.zero_()
            g.replay()
            side.synchronize()
            for got, want in zip((ext, te, up, st), eager):
                assert np.array_equal(got.cpu().numpy(), want)
        ctx.use_own_stream()
    assert (eager[3] == 0).all()
    whole = EE.fp64_extent(coef, dur, dirs)
    assert np.allclose(eager[0], whole[0], rtol=1e-9, atol=2e-9)
