"""Time allocation from and to given end states on the GPU (include/msnap.h, msnap_optimize_times_states;
csrc/msnap_timeopt.hip, timeopt_kernel<K, true>): the fixture of tests/golden/make_timeopt_states_golden.py (floor,
monotonicity, parity with msnap_solve_states at both ends of the run, optimality against the fixture's reference), the
prefix of the iteration against the restatement's knots, the end states through msnap_eval_state, the shapes at which
the kernel can go wrong, msnap_optimize_times on the rest-to-rest problem, position independence, entries and stream
capture, a zero weight, swarm.replan(optimize=...), and the argument errors.

The tests print what they measure before they assert (run with -s)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, norm_rel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import states_exact as SE  # noqa: E402
import timeopt_entry_cases as E  # noqa: E402
import timeopt_ref as R  # noqa: E402
import timeopt_states_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

W1 = (1.0, 1.0, 1.0, 1.0)
ULP4 = 4 * 2.0 ** -52                # the end-state bar of tests/test_states_gpu.py
MARGIN_MIN = 1e-3                    # prefix runs below it were left out by the generator
_Z = {}
_RUN = {}


def _fixture():
    if not _Z:
        z = np.load(os.path.join(GOLDEN_DIR, "timeopt_states_golden.npz"))
        _Z["z"], _Z["cases"] = z, S.unpack_cases(z)
    return _Z["z"], _Z["cases"]


def _ctx(order, ctx7, ctx9):
    return ctx7 if order == 7 else ctx9


def _group_inputs(drones):
    """One call's arrays for the drones of a group: a drone without a block gets a row of zeros in it"""
    c0 = drones[0]
    nd = (c0["order"] + 1) // 2 - 1
    wp = np.stack([c["wp"] for c in drones])
    t = c0["t"] if c0["shared"] else np.stack([c["t"] for c in drones])
    start = np.stack([np.zeros((4, nd)) if c["start"] is None else c["start"] for c in drones])
    end = np.stack([np.zeros((4, nd)) if c["end"] is None else c["end"] for c in drones])
    return wp, t, start, end


def _groups():
    _, cases = _fixture()
    out = {}
    for c in cases:
        out.setdefault(c["group"], []).append(c)
    return out


def _run_group(ctx, g, max_iter=500):
    """The fixture's group g through the host entry at the GPU test's settings, computed once"""
    key = (g, max_iter)
    if key not in _RUN:
        drones = _groups()[g]
        wp, t, start, end = _group_inputs(drones)
        _RUN[key] = ctx.optimize_times_states(wp, t, start, end, drones[0]["weights"], drones[0]["min_fraction"],
                                              max_iter, 1e-4)
    return _RUN[key]


def _delta(z):
    """The optimality margin as tests/test_timeopt_wide_gpu.py takes it: 100 x the restatement's largest gap over the
    drones on which it converged (the others are held to the restatement's own cost)."""
    return max(100.0 * float(z["gap4"][z["conv4"]].max()), 1e-9)


def _weighted_cost(ctx, coef, dur, w):
    c = ctx.snap_cost(coef, dur)
    return np.array([R.weighted(c[d], w) for d in range(c.shape[0])])


def _same(a, b, ia=slice(None), ib=slice(None)):
    return all(np.array_equal(x[ia], y[ib], equal_nan=True) for x, y in zip(a[:4], b[:4])) and \
        all(np.array_equal(a[4][k][ia], b[4][k][ib], equal_nan=True) for k in ("cost", "pg", "iters"))


# ---- 1. the fixture -------------------------------------------------------------------------------------------------
def test_fixture_floor_parity_and_optimality(ctx7, ctx9):
    z, cases = _fixture()
    delta = _delta(z)
    worst_gap, worst_held, steps = -1.0, -1.0, []
    for g, drones in _groups().items():
        c0 = drones[0]
        ctx = _ctx(c0["order"], ctx7, ctx9)
        w, mf = c0["weights"], c0["min_fraction"]
        wp, t, start, end = _group_inputs(drones)
        t_out, coef, dur, status, info = _run_group(ctx, g)
        N, M = wp.shape[0], wp.shape[1] - 1
        tt = np.tile(t, (N, 1)) if t.ndim == 1 else t
        assert (status == 0).all(), (g, status)
        assert (t_out[:, 0] == 0.0).all() and np.array_equal(t_out[:, M], tt[:, M]), g
        assert np.array_equal(dur, t_out[:, 1:] - t_out[:, :-1]), g
        Tmin = mf * tt[:, M] / M
        assert (dur >= Tmin[:, None] * (1 - 1e-12)).all(), (g, dur.min(), Tmin)
        c_0, c_1 = info["cost"][:, 0], info["cost"][:, 1]
        assert (c_1 <= c_0).all(), g
        # parity with the solve entry at both ends of the run
        ts = np.stack([R.start_times(tt[d], Tmin[d]) for d in range(N)])
        cs, ds, ss = ctx.solve_states(wp, ts, start, end)
        ce, de, se = ctx.solve_states(wp, t_out, start, end)
        assert (ss == 0).all() and (se == 0).all()
        assert (np.abs(c_0 - _weighted_cost(ctx, cs, ds, w)) <= 1e-9 * c_0).all(), g
        assert (np.abs(c_1 - _weighted_cost(ctx, ce, de, w)) <= 1e-9 * c_1).all(), g
        assert norm_rel(coef, ce) <= 1e-9, (g, norm_rel(coef, ce))
        assert np.array_equal(dur, de)
        if M == 1:
            assert (info["iters"] == 0).all() and np.array_equal(t_out, tt)
        for d, c in enumerate(drones):
            k = c["k"]
            gap = c_1[d] / float(z["J_ref"][k]) - 1.0
            print(f"drone {k}: order {c['order']} M {M} {c['combo']} min_fraction {mf} J/J0 {c_1[d] / c_0[d]:.4g} "
                  f"gap {gap:.3e} pg {info['pg'][d]:.2e} iters {int(info['iters'][d])}")
            if bool(z["conv4"][k]):
                worst_gap = max(worst_gap, gap)
                assert c_1[d] <= float(z["J_ref"][k]) * (1 + delta), (k, gap, delta)
            else:       # the restatement itself stopped on max_iter: held to its cost
                held = c_1[d] / float(z["J4"][k]) - 1.0
                worst_held = max(worst_held, held)
                assert c_1[d] <= float(z["J4"][k]) * (1 + 1e-6), (k, held)
            steps.append(int(info["iters"][d]))
    print(f"fixture: delta {delta:.3e}, worst gap to J_ref {worst_gap:.3e}, worst against a max_iter stop "
          f"{worst_held:.3e}, accepted steps mean {np.mean(steps):.1f} max {max(steps)}")


# ---- 2. the prefix of the iteration -----------------------------------------------------------------------------------
def test_prefix_of_the_iteration(ctx7, ctx9):
    """At max_iter 1 and 3 the knots are the restatement's within 10 x prefix_sens, its own response to gradients off
    by 2e-6, over the runs the generator kept (Armijo margin at least 1e-3)."""
    z, cases = _fixture()
    worst, kept = 0.0, 0
    for g, drones in _groups().items():
        ctx = _ctx(drones[0]["order"], ctx7, ctx9)
        M = drones[0]["wp"].shape[0] - 1
        if M == 1:
            continue
        for j, mi in enumerate((1, 3)):
            t_out, coef, dur, status, info = _run_group(ctx, g, mi)
            assert (status == 0).all()
            for d, c in enumerate(drones):
                k = c["k"]
                if z["p_margin"][k, j] < MARGIN_MIN:
                    continue
                kept += 1
                assert int(info["iters"][d]) == int(z["p_iters"][k, j]), (k, mi)
                diff = float(np.abs(t_out[d] - c["p_t"][j]).max() / c["t"][-1])
                ratio = diff / float(z["prefix_sens"][k, j])
                worst = max(worst, ratio)
                assert ratio <= 10.0, (k, mi, diff, float(z["prefix_sens"][k, j]))
    print(f"prefix: {kept} runs, worst |dt| / t[M] = {worst:.3f} x prefix_sens")
    assert kept > 0


# ---- 3. the end states ------------------------------------------------------------------------------------------------
def test_the_given_end_states_are_honoured(ctx7, ctx9):
    """eval_state at 0 returns start and wp[0], at sum(dur) end and wp[M], measured as tests/test_states_gpu.py measures
    the solve entry: the start relative, the end in units of the Horner sum's scale, both at 4 * 2^-52."""
    worst0, worst1, over = 0.0, 0.0, []
    for g, drones in _groups().items():
        order = drones[0]["order"]
        ctx = _ctx(order, ctx7, ctx9)
        K = (order + 1) // 2
        wp, t, start, end = _group_inputs(drones)
        t_out, coef, dur, status, info = _run_group(ctx, g)
        N, M = wp.shape[0], wp.shape[1] - 1
        assert np.array_equal(coef[:, 0, :, 0], wp[:, 0, :])
        p0, d0 = ctx.eval_state(coef, dur, np.zeros(N))
        assert np.array_equal(p0, wp[:, 0, :])
        rel = np.abs(d0 - start) / np.where(start == 0, 1.0, np.abs(start))
        worst0 = max(worst0, rel.max())
        if not (rel <= ULP4).all():
            over.append((g, "start", rel.max() / 2.0 ** -52))
        total = np.zeros(N)
        for i in range(M):
            total = total + dur[:, i]
        p1, d1 = ctx.eval_state(coef, dur, total)
        assert np.isfinite(d1).all()
        T = dur[:, -1]
        last = np.abs(coef[:, -1])
        for q in range(0, K):
            want = wp[:, M, :] if q == 0 else end[:, :, q - 1]
            got = p1 if q == 0 else d1[:, :, q - 1]
            scale = sum(SE.falling(j, q) * last[:, :, j] * T[:, None] ** (j - q) for j in range(q, 2 * K))
            r = np.abs(got - want) / np.maximum(np.abs(want), scale)
            worst1 = max(worst1, r.max())
            if not (r <= ULP4).all():
                over.append((g, "end", q, r.max() / 2.0 ** -52))
    print(f"end states: start within {worst0 / 2.0 ** -52:.2f} ulp, end within {worst1 / 2.0 ** -52:.2f} ulp of its scale")
    assert not over, over


# ---- 4. shapes where the kernel can go wrong --------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
def test_one_and_two_segments_tiles_and_null_blocks(ctx7, ctx9, order):
    ctx = _ctx(order, ctx7, ctx9)
    # one segment: recover_segment alone
    wp, t, start, end = SE.case(order, 1)
    r = ctx.optimize_times_states(wp, t, start, end)
    cs, ds, ss = ctx.solve_states(wp, t, start, end)
    assert (r[3] == 0).all() and (r[4]["iters"] == 0).all() and np.array_equal(r[0], t) and np.array_equal(r[2], ds)
    assert norm_rel(r[1], cs) <= 1e-12, norm_rel(r[1], cs)
    # two segments: the one knot receives both end terms; 17 drones: a full tile and a tail of one
    for M in (2, 10):
        wp, t, start, end = SE.case(order, M)
        assert wp.shape[0] == 17
        r = ctx.optimize_times_states(wp, t, start, end)
        assert (r[3] == 0).all() and (r[4]["cost"][:, 1] <= r[4]["cost"][:, 0]).all()
        ce, de, se = ctx.solve_states(wp, r[0], start, end)
        # (the trial runs the solve entry's own elimination, chain_solve: the coefficients are its bits)
        assert np.array_equal(r[2], de) and np.array_equal(r[1], ce), (M, norm_rel(r[1], ce))
        assert (r[4]["iters"] > 0).any()
        for d in (0, 15, 16):
            one = ctx.optimize_times_states(wp[d:d + 1], t[d:d + 1], start[d:d + 1], end[d:d + 1])
            assert _same(r, one, slice(d, d + 1)), (M, d)
        # NULL against blocks of zeros: the same bits
        zero = np.zeros_like(start)
        both = ctx.optimize_times_states(wp, t, zero, zero)
        assert _same(ctx.optimize_times_states(wp, t, None, None), both)
        assert _same(ctx.optimize_times_states(wp, t, None, end), ctx.optimize_times_states(wp, t, zero, end))
        assert _same(ctx.optimize_times_states(wp, t, start, None), ctx.optimize_times_states(wp, t, start, zero))


def test_the_eight_drone_tile_groups(ctx7, ctx9):
    """The groups above the 16-drone LDS limit (11 drones: a full 8-drone tile and a tail of 3): every drone alone gives
    the bits it gives in the group."""
    z, cases = _fixture()
    seen = set()
    for g, drones in _groups().items():
        if len(drones) != 11:
            continue
        order = drones[0]["order"]
        ctx = _ctx(order, ctx7, ctx9)
        M = drones[0]["wp"].shape[0] - 1
        assert M == {7: 40, 9: 29}[order]
        seen.add(order)
        wp, t, start, end = _group_inputs(drones)
        whole = _run_group(ctx, g)
        assert (whole[3] == 0).all()
        for d in (0, 7, 8, 10):
            one = ctx.optimize_times_states(wp[d:d + 1], t[d:d + 1], start[d:d + 1], end[d:d + 1], W1, 0.1, 500, 1e-4)
            assert _same(whole, one, slice(d, d + 1)), (g, d)
    assert seen == {7, 9}


@pytest.mark.parametrize("n", [16, 13])
def test_failed_drones_at_the_edges_of_a_tile(ctx7, n):
    """A NaN state value (status 3) and t[0] != 0 (status 2) at the first and last place of a full and of a partial
    tile: NaN outputs, neighbours untouched."""
    wp, t, start, end = SE.case(7, 10, N=n)
    good = ctx7.optimize_times_states(wp, t, start, end)
    assert (good[3] == 0).all()
    for first, last in ((3, 2), (2, 3)):
        s2, e2, t2 = start.copy(), end.copy(), t.copy()
        for d, code in ((0, first), (n - 1, last)):
            if code == 3:
                (s2 if d == 0 else e2)[d, 2, 1] = np.nan
            else:
                t2[d] = t2[d] + 0.25
        bad = ctx7.optimize_times_states(wp, t2, s2, e2)
        assert bad[3][0] == first and bad[3][n - 1] == last, bad[3]
        for d in (0, n - 1):
            assert np.isnan(bad[0][d]).all() and np.isnan(bad[1][d]).all() and np.isnan(bad[2][d]).all()
            assert np.isnan(bad[4]["cost"][d]).all() and np.isnan(bad[4]["pg"][d]) and bad[4]["iters"][d] == 0
        assert _same(bad, good, slice(1, n - 1), slice(1, n - 1))


# ---- 5. against msnap_optimize_times ----------------------------------------------------------------------------------
def test_zero_states_are_the_rest_to_rest_allocation(ctx7):
    """With both blocks zero the problem is msnap_optimize_times's: the same accepted steps at max_iter 1 and 3, knots
    within 10 x the fixture's prefix_sens of its order-7, 10-segment group, and the same final cost within delta."""
    from drone_path_planning_python_amd.synthetic import swarm
    z, cases = _fixture()
    delta = _delta(z)
    ks = [c["k"] for c in cases if c["order"] == 7 and c["wp"].shape[0] == 11 and c["min_fraction"] == 0.1
          and c["weights"] == W1 and not c["shared"]]
    sens = z["prefix_sens"][ks]
    sens = sens[np.isfinite(sens) & (z["p_margin"][ks] >= MARGIN_MIN)]
    bar = 10.0 * float(sens.max())
    wp, t = swarm(2, 6, 10)
    zero = np.zeros((6, 4, 3))
    for mi in (1, 3):
        a = ctx7.optimize_times(wp, t, W1, 0.1, mi, 1e-4)
        b = ctx7.optimize_times_states(wp, t, zero, zero, W1, 0.1, mi, 1e-4)
        assert (a[3] == 0).all() and (b[3] == 0).all()
        diff = float((np.abs(a[0] - b[0]).max(axis=1) / t[:, -1]).max())
        print(f"max_iter {mi}: accepted {a[4]['iters'].tolist()} / {b[4]['iters'].tolist()}, |dt| / t[M] {diff:.3e} "
              f"(bar {bar:.3e})")
        assert np.array_equal(a[4]["iters"], b[4]["iters"])
        assert diff <= bar
    a = ctx7.optimize_times(wp, t, W1, 0.1, 500, 1e-4)
    b = ctx7.optimize_times_states(wp, t, zero, zero, W1, 0.1, 500, 1e-4)
    rel = np.abs(a[4]["cost"][:, 1] - b[4]["cost"][:, 1]) / a[4]["cost"][:, 1]
    print(f"tol 1e-4: final costs agree within {rel.max():.3e} (delta {delta:.3e})")
    assert (rel <= delta).all()


# ---- 6. position independence, entries, capture -------------------------------------------------------------------------
def test_position_independence_entries_and_capture(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    wp, t, start, end = SE.case(7, 10, N=50)
    one = ctx7.optimize_times_states(wp[5:6], t[5:6], start[5:6], end[5:6])
    assert one[3][0] == 0 and one[4]["iters"][0] > 2
    for n, pos in ((50, 25), (17, 16)):
        w2, t2, s2, e2 = wp[:n].copy(), t[:n].copy(), start[:n].copy(), end[:n].copy()
        w2[pos], t2[pos], s2[pos], e2[pos] = wp[5], t[5], start[5], end[5]
        assert _same(ctx7.optimize_times_states(w2, t2, s2, e2), one, slice(pos, pos + 1)), (n, pos)
    # the host entry without its optional outputs, each state block given and NULL, against the device entry (one full
    # 16-drone tile and a tail of one)
    w3, t3, s3, e3 = SE.case(7, 3, N=17)
    for states in ((s3, e3), (s3, None), (None, e3), (None, None)):
        E.assert_host_entry_without_optionals_is_the_device_entry(ctx7, "_states", w3, t3, states)
    # the device entry, eager and inside a captured graph, on a context of its own
    dev = torch.device("cuda", 0)
    n, m = 17, 10
    host = ctx7.optimize_times_states(wp[:n], t[:n], start[:n], end[:n])
    dw, dt = torch.from_numpy(wp[:n]).to(dev), torch.from_numpy(t[:n]).to(dev)
    ds, de = torch.from_numpy(start[:n]).to(dev), torch.from_numpy(end[:n]).to(dev)
    o_t = torch.empty((n, m + 1), dtype=torch.float64, device=dev)
    o_c = torch.empty((n, m, 4, 8), dtype=torch.float64, device=dev)
    o_d = torch.empty((n, m), dtype=torch.float64, device=dev)
    o_s = torch.empty((n,), dtype=torch.int32, device=dev)
    o_j = torch.empty((n, 2), dtype=torch.float64, device=dev)
    o_p = torch.empty((n,), dtype=torch.float64, device=dev)
    o_i = torch.empty((n,), dtype=torch.int32, device=dev)
    outs = (o_t, o_c, o_d, o_s, o_j, o_p, o_i)

    def result():
        return tuple(x.cpu().numpy() for x in (o_t, o_c, o_d, o_s)) + \
            ({"cost": o_j.cpu().numpy(), "pg": o_p.cpu().numpy(), "iters": o_i.cpu().numpy()},)

    def call(ctx):
        ctx.optimize_times_states_device(n, m, dw, dt, 0, ds, de, W1, 0.1, 200, 1e-4, *outs)

    side = torch.cuda.Stream()
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            call(ctx)                                   # once outside the capture (msnap.h, "Stream capture")
            side.synchronize()
            assert _same(result(), host)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                call(ctx)
            ctx.set_stream(side.cuda_stream)
            for x in outs:
                x.zero_()
            g.replay()
            side.synchronize()
            assert _same(result(), host)
        del g


# ---- 7. a zero weight -----------------------------------------------------------------------------------------------------
def test_zero_weight_ignores_the_axis(ctx7):
    wp, t, start, end = SE.case(7, 10, N=6)
    w = (1.0, 1.0, 1.0, 0.0)
    a = ctx7.optimize_times_states(wp, t, start, end, weights=w)
    rng = np.random.default_rng(1)
    wp2, s2, e2 = wp.copy(), start.copy(), end.copy()
    wp2[:, :, 3] = rng.normal(size=wp[:, :, 3].shape) * 3.0
    s2[:, 3, :] = rng.normal(size=s2[:, 3, :].shape)
    e2[:, 3, :] = rng.normal(size=e2[:, 3, :].shape)
    b = ctx7.optimize_times_states(wp2, t, s2, e2, weights=w)
    assert (a[3] == 0).all() and (a[4]["iters"] > 0).any()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[4]["cost"], b[4]["cost"])
    assert not np.array_equal(ctx7.optimize_times_states(wp, t, start, end)[0], a[0])


# ---- 8. swarm.replan(optimize=...) -------------------------------------------------------------------------------------
def test_replan_with_allocated_times(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute, replan
    wp, t, _, _ = SE.case(7, 10, N=8)
    rng = np.random.default_rng(11)
    dev = torch.device("cuda", 0)
    with Context(device_id=0, order=7, max_segments=16) as dctx:
        comp = DeviceCompute(dctx, torch)
        coef, dur, st = comp.solve_states(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
        t_r = 0.4 * dur.sum(dim=1)
        wp_new = torch.from_numpy(np.cumsum(rng.uniform(-2.0, 2.0, (8, 4, 4)), axis=1)).to(dev)
        t_new = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64, device=dev)
        c0, d0, s0, (pos, deriv) = replan(comp, coef, dur, t_r, wp_new, t_new)
        c0, d0 = c0.clone(), d0.clone()
        c1, d1, s1, (pos1, deriv1) = replan(comp, coef, dur, t_r, wp_new, t_new,
                                            optimize={"min_fraction": 0.1, "max_iter": 200, "tol": 1e-4})
        torch.cuda.synchronize()
        assert (s0.cpu().numpy() == 0).all() and (s1.cpu().numpy() == 0).all()
        with pytest.raises(ValueError):
            replan(comp, coef, dur, t_r, wp_new, t_new, optimize={"steps": 3})
        c0, d0, c1, d1 = (x.cpu().numpy() for x in (c0, d0, c1, d1))
        pos, deriv = pos.cpu().numpy(), deriv.cpu().numpy()
    J0, J1 = ctx7.snap_cost(c0, d0).sum(axis=1), ctx7.snap_cost(c1, d1).sum(axis=1)
    print("replan: cost with allocated times / with the given times:", np.round(J1 / J0, 4).tolist())
    assert (J1 < J0).all()
    assert c1.shape == (8, 4, 4, 8) and (np.abs(d1.sum(axis=1) - 4.0) <= 1e-14).all()      # the last time is kept
    # the hand-over: position bit for bit, derivatives 1 .. K-1 within the start bar of tests/test_states_gpu.py
    assert np.array_equal(c1[:, 0, :, 0], pos)
    p, dd = ctx7.eval_state(c1, d1, np.zeros(8))
    assert np.array_equal(p, pos)
    rel = np.abs(dd - deriv) / np.where(deriv == 0, 1.0, np.abs(deriv))
    print(f"replan: derivatives continue within {rel.max() / 2.0 ** -52:.2f} ulp")
    assert (rel <= ULP4).all()


# ---- 9. argument errors --------------------------------------------------------------------------------------------------
def test_argument_errors(ctx7, ctx9):
    from drone_path_planning_python_amd._lib import MsnapError
    for ctx in (ctx7, ctx9):
        wp, t, start, end = SE.case(ctx.order, 3, N=2)
        for kw in ({"weights": (1, -1, 1, 1)}, {"min_fraction": 0.0}, {"min_fraction": 1.5}, {"max_iter": -1},
                   {"tol": -1.0}, {"weights": (1, np.nan, 1, 1)}):
            with pytest.raises(MsnapError) as e:
                ctx.optimize_times_states(wp, t, start, end, **kw)
            assert e.value.code == -1, kw
        top = ctx.optimize_times_states_max_segments()
        assert top == {7: 79, 9: 57}[ctx.order]
        with pytest.raises(MsnapError) as e:
            ctx.optimize_times_states(np.zeros((1, top + 2, 4)), np.arange(top + 2.0))
        assert e.value.code == -4
        ok = ctx.optimize_times_states(np.cumsum(np.ones((2, top + 1, 4)), axis=1) ** 2, np.arange(top + 1.0), max_iter=3)
        assert (ok[3] == 0).all()
        nd = (ctx.order + 1) // 2 - 1
        empty = ctx.optimize_times_states(np.zeros((0, 4, 4)), np.arange(4.0), np.zeros((0, 4, nd)), None)
        assert empty[0].shape == (0, 4) and empty[1].shape == (0, 3, 4, ctx.ncoef)
