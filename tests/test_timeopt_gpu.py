"""Time allocation on the GPU (include/msnap.h, "time allocation"; csrc/msnap_timeopt.hip): the closed-form gradient
kernel, Context.optimize_times on the fixture of tests/golden/make_timeopt_golden.py (floor, monotonicity, parity with
the solve entries, optimality against the fixture's reference optimum), edge cases and failed drones, position
independence and power-of-two scaling, weights, stream capture, and the node path.

The tests print what they measure before they assert (run with -s)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, norm_rel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timeopt_entry_cases as E  # noqa: E402
import timeopt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

W1 = (1.0, 1.0, 1.0, 1.0)


def _fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "timeopt_golden.npz"))
    return z, int(z["n"])


def _weighted_cost(ctx, coef, dur, w=W1):
    c = ctx.snap_cost(coef, dur)
    return np.array([R.weighted(c[d], w) for d in range(c.shape[0])])


def _swarm(cfg, n, m):
    from drone_path_planning_python_amd.synthetic import swarm
    return swarm(cfg, n, m)


@pytest.mark.parametrize("order", [7, 9])
def test_gradient_kernel_against_the_closed_form(ctx7, ctx9, order):
    ctx = ctx7 if order == 7 else ctx9
    worst = 0.0
    for n, m in ((1, 10), (5, 4), (16, 10), (67, 7), (1000, 20)):
        wp, t = _swarm(40 + n, n, m)
        coef, dur, status = ctx.solve_batch(wp, t)
        assert (status == 0).all()
        got = ctx.snap_cost_grad(coef, dur)
        assert got.shape == (n, m, 4)
        terms = R.energy_terms(coef)
        ref = R.snap_cost_grad(coef)
        scale = np.abs(terms).sum(axis=(1, 2, 3))[:, None, None]
        err = float((np.abs(got - ref) / scale).max())
        worst = max(worst, err)
    print(f"order {order}: gradient kernel vs NumPy, max |diff| / sum |terms| = {worst:.3e}")
    assert worst <= 1e-13


def test_gradient_is_the_derivative_of_the_solved_cost(ctx7):
    """Central differences of solve + cost on the GPU against the kernel's -E (the envelope theorem)."""
    wp, t = _swarm(2, 3, 10)
    coef, dur, _ = ctx7.solve_batch(wp, t)
    g = ctx7.snap_cost_grad(coef, dur).sum(axis=2)
    for d in range(3):
        for i in (0, 4, 9):
            h = 1e-5 * dur[d, i]
            J = []
            for s in (+1, -1):
                T = dur[d].copy()
                T[i] += s * h
                c2, d2, _ = ctx7.solve_batch(wp[d:d + 1], np.concatenate([[0.0], np.cumsum(T)])[None])
                J.append(ctx7.snap_cost(c2, d2).sum())
            fd = (J[0] - J[1]) / (2 * h)
            assert abs(fd - g[d, i]) <= 1e-6 * abs(g[d]).max(), (d, i, fd, g[d, i])


def test_fixture_floor_parity_and_optimality(ctx7, ctx9):
    z, n = _fixture()
    delta = max(100.0 * float(z["gap4"].max()), 1e-9)
    worst_gap, solves = -1.0, []
    for k in range(n):
        ctx = ctx7 if int(z["order"][k]) == 7 else ctx9
        wp, t, mf = z[f"wp_{k}"][None], z[f"t_{k}"][None], float(z["min_fraction"][k])
        M = t.shape[1] - 1
        t_out, coef, dur, status, info = ctx.optimize_times(wp, t, W1, mf, 500, 1e-4)
        assert status[0] == 0, k
        assert t_out[0, 0] == 0.0 and t_out[0, M] == t[0, M], k
        assert np.array_equal(dur[0], t_out[0, 1:] - t_out[0, :-1]), k
        Tmin = mf * t[0, M] / M
        assert (dur[0] >= Tmin * (1 - 1e-12)).all(), (k, dur[0].min(), Tmin)
        c0, c1 = info["cost"][0]
        assert c1 <= c0, (k, c0, c1)
        # parity with the solve entries at both ends of the run
        ts = R.start_times(t[0], Tmin)[None]
        cs, ds, ss = ctx.solve_batch(wp, ts)
        ce, de, se = ctx.solve_batch(wp, t_out)
        assert ss[0] == 0 and se[0] == 0
        assert abs(c0 - _weighted_cost(ctx, cs, ds)[0]) <= 1e-9 * c0, (k, c0)
        assert abs(c1 - _weighted_cost(ctx, ce, de)[0]) <= 1e-9 * c1, (k, c1)
        assert norm_rel(coef, ce) <= 1e-9, (k, norm_rel(coef, ce))
        assert np.array_equal(dur, de)
        # the fixture's start cost is the oracle's dense solve: coefficient parity with it is held to 1e-6 (smoke()),
        # the cost is quadratic in the coefficients
        assert abs(c0 - float(z["J0"][k])) <= 2e-6 * c0, (k, c0, float(z["J0"][k]))
        gap = c1 / float(z["J_ref"][k]) - 1.0
        worst_gap = max(worst_gap, gap)
        print(f"drone {k}: order {int(z['order'][k])} M {M} min_fraction {mf} J/J0 {c1 / c0:.4g} gap {gap:.3e} "
              f"pg {info['pg'][0]:.2e} iters {int(info['iters'][0])}")
        assert c1 <= float(z["J_ref"][k]) * (1 + delta), (k, gap, delta)
        solves.append(int(info["iters"][0]))
    print(f"fixture: delta {delta:.3e}, worst gap {worst_gap:.3e}, accepted steps mean {np.mean(solves):.1f} "
          f"max {max(solves)}")


def test_max_iter_zero_one_segment_and_argument_errors(ctx7, ctx9):
    from drone_path_planning_python_amd._lib import MsnapError
    for ctx in (ctx7, ctx9):
        wp, t = _swarm(3, 5, 10)
        t_out, coef, dur, status, info = ctx.optimize_times(wp, t, max_iter=0)
        cs, ds, ss = ctx.solve_batch(wp, t)
        assert (status == 0).all() and np.array_equal(t_out, t) and np.array_equal(dur, ds)
        assert norm_rel(coef, cs) <= 1e-9
        assert np.array_equal(info["cost"][:, 0], info["cost"][:, 1]) and (info["iters"] == 0).all()
        # one segment: nothing to move
        wp1 = np.zeros((3, 2, 4))
        wp1[:, 1, :] = [[1, 2, 3, 0.5], [0, 0, 0, 0], [-1, 4, 2, 1]]
        t1 = np.array([0.0, 2.5])
        t_out, coef, dur, status, info = ctx.optimize_times(wp1, t1)
        cs, ds, ss = ctx.solve_batch(wp1, t1)
        assert (status == 0).all() and np.array_equal(t_out, np.tile(t1, (3, 1))) and np.array_equal(dur, ds)
        assert norm_rel(coef, cs) <= 1e-9 and (info["iters"] == 0).all()
        # argument errors
        for kw in ({"weights": (1, -1, 1, 1)}, {"min_fraction": 0.0}, {"min_fraction": 1.5}, {"max_iter": -1},
                   {"tol": -1.0}, {"weights": (1, np.nan, 1, 1)}):
            with pytest.raises(MsnapError) as e:
                ctx.optimize_times(wp, t, **kw)
            assert e.value.code == -1, kw
        big = 81 if ctx.order == 7 else 59
        with pytest.raises(MsnapError) as e:
            ctx.optimize_times(np.zeros((1, big + 1, 4)), np.arange(big + 1.0))
        assert e.value.code == -4
        ok = ctx.optimize_times(np.cumsum(np.ones((2, big, 4)), axis=1) ** 2, np.arange(float(big)), max_iter=3)
        assert (ok[3] == 0).all()


def test_failed_drones_among_good_ones(ctx7):
    wp, t = _swarm(7, 40, 10)
    good = ctx7.optimize_times(wp, t)
    assert (good[3] == 0).all()
    wpb, tb = wp.copy(), t.copy()
    wpb[3, 4, 1] = np.nan
    tb[17, 5] = tb[17, 4]
    tb[30] = tb[30] + 0.5
    bad = ctx7.optimize_times(wpb, tb)
    assert bad[3][3] == 3 and bad[3][17] == 2 and bad[3][30] == 2
    for d in (3, 17, 30):
        assert np.isnan(bad[0][d]).all() and np.isnan(bad[1][d]).all() and np.isnan(bad[2][d]).all()
        assert np.isnan(bad[4]["cost"][d]).all() and np.isnan(bad[4]["pg"][d]) and bad[4]["iters"][d] == 0
    keep = np.array([d for d in range(40) if d not in (3, 17, 30)])
    only = ctx7.optimize_times(wp[keep], t[keep])
    for a, b, c in zip(bad[:4], good[:4], only[:4]):
        assert np.array_equal(a[keep], b[keep]) and np.array_equal(a[keep], c)
    for key in ("cost", "pg", "iters"):
        assert np.array_equal(bad[4][key][keep], only[4][key])


def test_position_independence_entries_and_scaling(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    wp, t = _swarm(2, 1000, 10)
    one = ctx7.optimize_times(wp[5:6], t[5:6])
    assert one[3][0] == 0 and one[4]["iters"][0] > 5

    def same(res, pos):
        return all(np.array_equal(a[pos], b[0]) for a, b in zip(res[:4], one[:4])) and \
            all(np.array_equal(res[4][k][pos], one[4][k][0]) for k in ("cost", "pg", "iters"))

    for pos in (0, 999):
        w2, t2 = wp.copy(), t.copy()
        w2[pos], t2[pos] = wp[5], t[5]
        assert same(ctx7.optimize_times(w2, t2), pos), pos
    # the device entry, on a context of its own
    dev = torch.device("cuda", 0)
    with Context(device_id=0, order=7, max_segments=64) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dw, dt = torch.from_numpy(wp[5:6]).to(dev), torch.from_numpy(t[5:6]).to(dev)
        o_t = torch.empty((1, 11), dtype=torch.float64, device=dev)
        o_c = torch.empty((1, 10, 4, 8), dtype=torch.float64, device=dev)
        o_d = torch.empty((1, 10), dtype=torch.float64, device=dev)
        o_s = torch.empty((1,), dtype=torch.int32, device=dev)
        o_j = torch.empty((1, 2), dtype=torch.float64, device=dev)
        o_p = torch.empty((1,), dtype=torch.float64, device=dev)
        o_i = torch.empty((1,), dtype=torch.int32, device=dev)
        ctx.optimize_times_device(1, 10, dw, dt, 0, W1, 0.1, 200, 1e-4, o_t, o_c, o_d, o_s, o_j, o_p, o_i)
        torch.cuda.synchronize()
        dres = tuple(x.cpu().numpy() for x in (o_t, o_c, o_d, o_s)) + \
            ({"cost": o_j.cpu().numpy(), "pg": o_p.cpu().numpy(), "iters": o_i.cpu().numpy()},)
        assert same(dres, 0)
        # cost, pg, iters are optional
        o_c.zero_()
        ctx.optimize_times_device(1, 10, dw, dt, 0, W1, 0.1, 200, 1e-4, o_t, o_c, o_d, o_s)
        torch.cuda.synchronize()
        assert np.array_equal(o_c.cpu().numpy(), one[1])
    # ... for the host entry too (one full 16-drone tile and a tail of one)
    E.assert_host_entry_without_optionals_is_the_device_entry(ctx7, "", *_swarm(2, 17, 3))
    # waypoints times 4: every quantity scales by a power of two
    four = ctx7.optimize_times(4.0 * wp[5:6], t[5:6])
    assert np.array_equal(four[0], one[0]) and np.array_equal(four[2], one[2])
    assert np.array_equal(four[4]["iters"], one[4]["iters"]) and np.array_equal(four[4]["pg"], one[4]["pg"])
    assert np.array_equal(four[1], 4.0 * one[1]) and np.array_equal(four[4]["cost"], 16.0 * one[4]["cost"])


def test_zero_weight_ignores_the_axis(ctx7):
    wp, t = _swarm(2, 6, 10)
    w = (1.0, 1.0, 1.0, 0.0)
    a = ctx7.optimize_times(wp, t, weights=w)
    wp2 = wp.copy()
    wp2[:, :, 3] = np.random.default_rng(1).normal(size=wp[:, :, 3].shape) * 3.0
    b = ctx7.optimize_times(wp2, t, weights=w)
    assert (a[3] == 0).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[4]["cost"], b[4]["cost"])
    # and it is the optimum of the position-only cost: the restatement with the same weights agrees
    for d in range(6):
        r = R.optimize(wp[d], t[d], w, 0.1, 200, 1e-4, 8, R.fast_cost)
        assert abs(a[4]["cost"][d, 1] - r["cost"]) <= 1e-6 * r["cost"], (d, a[4]["cost"][d, 1], r["cost"])
    full = ctx7.optimize_times(wp, t)
    assert not np.array_equal(full[0], a[0])


def test_device_entry_in_a_captured_graph(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    dev = torch.device("cuda", 0)
    n, m = 37, 10
    inputs = [_swarm(60 + k, n, m) for k in range(2)]
    eager = [ctx7.optimize_times(wp, t) for wp, t in inputs]
    dw = torch.empty((n, m + 1, 4), dtype=torch.float64, device=dev)
    dt = torch.empty((n, m + 1), dtype=torch.float64, device=dev)
    o_t = torch.empty((n, m + 1), dtype=torch.float64, device=dev)
    o_c = torch.empty((n, m, 4, 8), dtype=torch.float64, device=dev)
    o_d = torch.empty((n, m), dtype=torch.float64, device=dev)
    o_s = torch.empty((n,), dtype=torch.int32, device=dev)
    o_j = torch.empty((n, 2), dtype=torch.float64, device=dev)
    o_p = torch.empty((n,), dtype=torch.float64, device=dev)
    o_i = torch.empty((n,), dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()

    def call(ctx):
        ctx.optimize_times_device(n, m, dw, dt, 0, W1, 0.1, 200, 1e-4, o_t, o_c, o_d, o_s, o_j, o_p, o_i)

    with Context(order=7, max_segments=16) as ctx:
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            dw.copy_(torch.from_numpy(inputs[0][0]))
            dt.copy_(torch.from_numpy(inputs[0][1]))
            call(ctx)                                   # once outside the capture (msnap.h, "Stream capture")
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                call(ctx)
            ctx.set_stream(side.cuda_stream)
            for k in (1, 0):
                dw.copy_(torch.from_numpy(inputs[k][0]))
                dt.copy_(torch.from_numpy(inputs[k][1]))
                o_c.zero_()
                o_t.zero_()
                g.replay()
                side.synchronize()
                for got, want in zip((o_t, o_c, o_d, o_s), eager[k][:4]):
                    assert np.array_equal(got.cpu().numpy(), want), k
                assert np.array_equal(o_j.cpu().numpy(), eager[k][4]["cost"])
                assert np.array_equal(o_i.cpu().numpy(), eager[k][4]["iters"])


def test_node_path_lowers_the_cost_and_keeps_the_duration(ctx7):
    from drone_path_planning_python_amd.nodes import msgs
    from drone_path_planning_python_amd.nodes.drones_pols_generator import paths_to_pols
    rng = np.random.default_rng(5)
    paths = []
    for _ in range(2):                                   # the reference's shape: 50 poses, 49 segments
        pos = np.cumsum(rng.normal(size=(50, 3)) * 0.3, axis=0)
        quat = np.tile([0.0, 0.0, 0.0, 1.0], (50, 1))
        paths.append(msgs.path_from_arrays(pos, quat))
    m0, c0, d0 = paths_to_pols(paths, ctx7)
    m1, c1, d1 = paths_to_pols(paths, ctx7, optimize_times=True)
    J0, J1 = ctx7.snap_cost(c0, d0).sum(axis=1), ctx7.snap_cost(c1, d1).sum(axis=1)
    print("node path: cost ratio", J1 / J0)
    assert (J1 < J0).all() and J1.sum() < J0.sum()
    np.testing.assert_allclose(d1.sum(axis=1), d0.sum(axis=1), rtol=1e-14)
    assert m1.shape == m0.shape and np.isfinite(m1).all()


def test_c_abi_from_plain_c(tmp_path):
    """include/msnap.h's time-allocation entries consumed by a C99 program compiled with gcc."""
    import subprocess
    from conftest import ROOT
    from drone_path_planning_python_amd import _lib
    exe = str(tmp_path / "abi_timeopt")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "abi_timeopt.c"), "-o", exe, "-L", libdir, "-lmsnap", "-lm",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "gradient rel err" in r.stdout, (r.returncode, r.stdout, r.stderr)
