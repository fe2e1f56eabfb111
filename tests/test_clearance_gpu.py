"""Pairwise clearance on the GPU (include/msnap.h, "pairwise clearance"): the contract against the exact reference
(tests/clearance_exact.py), a shared grid, unequal totals, the crossing pair the sampled pass misses, attained values,
bit identity, per-pair status, a large list against the fp64 restatement, the certify_clearance pipeline on the
formation fixture's swarm and on an awkward swarm of 12 (every pair), and stream capture."""
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_cases as CC  # noqa: E402
import clearance_exact as CE  # noqa: E402

pytestmark = pytest.mark.gpu

ALL15 = np.array(list(itertools.combinations(range(6), 2)), dtype=np.int32)


def _solve(ctx, wp, t):
    coef, dur, status = ctx.solve_batch(wp, t)
    assert (status == 0).all()
    return coef, dur


def _solved(ctx, cfg, n, m, shared=False):
    from drone_path_planning_python_amd.synthetic import swarm
    return _solve(ctx, *swarm(cfg, n, m, shared_times=shared))


def _check_contract(ctx, coef, dur, pairs):
    """The shared helper (tests/clearance_exact.py) with the allowance of inputs near the origin: no coordinate term."""
    return CE.check_contract(ctx, coef, dur, pairs, with_R=False, restated=False)[:3]


@pytest.mark.parametrize("m", [1, 2, 10])
def test_contract_against_the_exact_reference_order7(ctx7, m):
    coef, dur = _solved(ctx7, 7000 + m, 6, m)
    _check_contract(ctx7, coef, dur, ALL15)


def test_contract_against_the_exact_reference_order9(ctx9):
    coef, dur = _solved(ctx9, 9004, 6, 4)
    _check_contract(ctx9, coef, dur, ALL15)


def test_shared_grid_with_every_second_slot_empty(ctx7):
    coef, dur = _solved(ctx7, 7110, 6, 10, shared=True)
    assert (dur == dur[0]).all()
    _check_contract(ctx7, coef, dur, ALL15)


def test_unequal_totals_end_the_window_inside_a_segment(ctx7):
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(7210, 6, 10)
    t = t.copy()
    t[0] *= 0.63
    coef, dur = _solve(ctx7, wp, t)
    pairs = ALL15[:5]                                    # the pairs of drone 0
    md, tm, lower = _check_contract(ctx7, coef, dur, pairs)
    window = np.minimum(np.add.accumulate(dur[0])[-1], np.add.accumulate(dur[1:6], axis=1)[:, -1])
    assert (tm <= window).all()
    assert (window < dur[1:6].sum(axis=1) - 0.1).any()   # some window does end early


def test_the_crossing_pair_the_sampled_pass_misses(ctx7):
    """Two rest-to-rest drones cross at right angles, 2 m in 1.1 s each, both at the origin at t = 0.55 s.  The
    samples at 0.5 s and 0.6 s see them 0.279 m apart (tests/test_clearance_cpu.py has the oracle's figure): no hit at
    radius 0.1.  pair_clearance finds the collision, certify_clearance reports both drones."""
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute, certify_clearance, default_sample_count
    from drone_path_planning_python_amd.synthetic import SAMPLE_DT
    wp = np.zeros((2, 2, 4))
    wp[0, :, 0] = [-1.0, 1.0]
    wp[1, :, 1] = [-1.0, 1.0]
    coef, dur = _solve(ctx7, wp, np.array([0.0, 1.1]))
    S = default_sample_count(1.1, SAMPLE_DT)
    pos = ctx7.sample(coef, dur, SAMPLE_DT, S, 3)
    smd, _, shit = ctx7.formation_collide(pos, pos, 0.1)
    assert not shit.any() and (smd >= 0.25).all()
    md, tm, lower, status = ctx7.pair_clearance(coef, dur, np.array([[0, 1]], dtype=np.int32))
    print("crossing pair:", md, tm, lower)
    assert status[0] == 0 and md[0] < 1e-6 and abs(tm[0] - 0.55) < 1e-6
    assert not CE.contract_violations(md[0], lower[0], 0.0)
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        comp = DeviceCompute(ctx, torch)
        dev = torch.device("cuda", 0)
        res = certify_clearance(comp, torch.from_numpy(coef).to(dev), torch.from_numpy(dur).to(dev), 0.1, SAMPLE_DT, S)
        torch.cuda.synchronize()
        assert res.hit.tolist() == [True, True] and not res.sampled_hit.any()
        assert res.pairs.tolist() == [[0, 1]] and float(res.certified_lower.max()) <= 1e-6


@pytest.fixture(scope="module")
def big(ctx7):
    coef, dur = _solved(ctx7, 7300, 256, 10)
    rng = np.random.default_rng(7300)
    a = rng.integers(0, 256, size=20000)
    b = (a + rng.integers(1, 256, size=20000)) % 256
    pairs = np.stack([a, b], axis=1).astype(np.int32)
    out = ctx7.pair_clearance(coef, dur, pairs)
    return coef, dur, pairs, out


def test_large_list_against_the_fp64_restatement(big):
    coef, dur, pairs, (md, tm, lower, status) = big
    assert (status == 0).all()
    st = {}
    rmd, rtm, rlower = CE.fp64_clearance(coef, dur, pairs, stats=st)
    print("nodes per lane: mean", st["nodes"].mean(), "max", st["nodes"].max(), "capped", int(st["capped"].sum()))
    assert st["nodes"].max() < CE.MAX_NODES and int(st["capped"].sum()) == 0       # every walk of this list closes
    np.testing.assert_allclose(md, rmd, rtol=1e-9, atol=CE.ABS_ROUND)
    np.testing.assert_allclose(lower, rlower, rtol=1e-9, atol=CE.ABS_CLOSE)
    assert (lower <= md).all() and (lower >= md * (1 - CE.REL_CLOSE) - CE.ABS_CLOSE - CE.ABS_ROUND).all()
    assert (tm >= 0).all() and (tm <= np.minimum(dur[pairs[:, 0]].sum(axis=1), dur[pairs[:, 1]].sum(axis=1)) * (1 + 1e-15)).all()


def test_results_are_bit_identical_across_positions_lists_orders_and_entries(ctx7, big):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute
    coef, dur, pairs, (md, tm, lower, status) = big
    one = np.array([[17, 201]], dtype=np.int32)
    m1, t1, l1, s1 = ctx7.pair_clearance(coef, dur, one)
    assert s1[0] == 0
    lst = pairs[:1000].copy()
    for pos in (0, 999):
        lst2 = lst.copy()
        lst2[pos] = one[0]
        m, t, lo, s = ctx7.pair_clearance(coef, dur, lst2)
        assert (m[pos], t[pos], lo[pos], s[pos]) == (m1[0], t1[0], l1[0], s1[0])
        other = np.arange(1000) != pos
        assert np.array_equal(m[other], md[:1000][other]) and np.array_equal(lo[other], lower[:1000][other])
    m, t, lo, s = ctx7.pair_clearance(coef, dur, lst[::-1])
    assert np.array_equal(m[::-1], md[:1000]) and np.array_equal(t[::-1], tm[:1000]) and np.array_equal(lo[::-1], lower[:1000])
    m, t, lo, s = ctx7.pair_clearance(coef, dur, lst[:, ::-1])
    assert np.array_equal(m, md[:1000]) and np.array_equal(t, tm[:1000]) and np.array_equal(lo, lower[:1000])
    # lanes that straddle a workgroup boundary: 27 pairs x 19 slots = 513 = 2 * 256 + 1
    m, t, lo, s = ctx7.pair_clearance(coef, dur, pairs[:27])
    assert np.array_equal(m, md[:27]) and np.array_equal(t, tm[:27]) and np.array_equal(lo, lower[:27])
    # the device entry, on a context of its own
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        comp = DeviceCompute(ctx, torch)
        dev = torch.device("cuda", 0)
        out = comp.pair_clearance(torch.from_numpy(coef).to(dev), torch.from_numpy(dur).to(dev),
                                  torch.from_numpy(pairs[:1000].copy()).to(dev))
        torch.cuda.synchronize()
        for got, want in zip(out, (md, tm, lower, status)):
            assert np.array_equal(got.cpu().numpy(), want[:1000])
        # an empty list is a no-op
        out = comp.pair_clearance(torch.from_numpy(coef).to(dev), torch.from_numpy(dur).to(dev),
                                  torch.zeros((0, 2), dtype=torch.int32, device=dev))
        assert all(x.shape == (0,) for x in out)


def test_per_pair_status_and_guarded_buffers(ctx7):
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd._lib import MsnapError
    from drone_path_planning_python_amd.swarm import DeviceCompute
    coef, dur = _solved(ctx7, 7400, 6, 3)
    good = ctx7.pair_clearance(coef, dur, ALL15)
    c, d = coef.copy(), dur.copy()
    c[4, 1, 3, 2] = np.nan            # (the yaw axis: any coefficient of the drone counts)
    d[5, 2] = 0.0
    pairs = np.array([(0, 1), (-1, 2), (0, 2), (3, 6), (0, 3), (2, 2), (1, 2), (1, 4), (1, 3), (5, 0), (2, 3), (4, 5)],
                     dtype=np.int32)
    want = [0, 4, 0, 4, 0, 4, 0, 3, 0, 2, 0, 3]
    G = 1024                          # guard margins around coef and dur on the device
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        comp = DeviceCompute(ctx, torch)
        dev = torch.device("cuda", 0)
        bufs = []
        for arr in (c, d):
            g = torch.full((arr.size + 2 * G,), -7.25e300, dtype=torch.float64, device=dev)
            g[G:G + arr.size] = torch.from_numpy(arr.reshape(-1)).to(dev)
            bufs.append(g)
        md, tm, lower, status = comp.pair_clearance(bufs[0][G:G + c.size].view(c.shape), bufs[1][G:G + d.size].view(d.shape),
                                                    torch.from_numpy(pairs).to(dev))
        torch.cuda.synchronize()
        md, tm, lower, status = (x.cpu().numpy() for x in (md, tm, lower, status))
        for g, arr in zip(bufs, (c, d)):
            g = g.cpu().numpy()
            assert (g[:G] == -7.25e300).all() and (g[G + arr.size:] == -7.25e300).all()
            assert np.array_equal(g[G:G + arr.size], arr.reshape(-1), equal_nan=True)
    assert status.tolist() == want
    lookup = {tuple(p): k for k, p in enumerate(ALL15.tolist())}
    for k, (p, st) in enumerate(zip(pairs.tolist(), want)):
        if st:
            assert np.isnan(md[k]) and np.isnan(tm[k]) and np.isnan(lower[k])
        else:
            j = lookup[tuple(p)]
            assert (md[k], tm[k], lower[k]) == (good[0][j], good[1][j], good[2][j])
    # the host entry gives the same; shape errors are refused
    h = ctx7.pair_clearance(c, d, pairs)
    assert np.array_equal(h[3], status) and np.array_equal(h[0], md, equal_nan=True)
    with pytest.raises(MsnapError):
        ctx7.pair_clearance(np.zeros((2, ctx7.max_segments + 1, 4, 8)), np.ones((2, ctx7.max_segments + 1)), pairs[:1])
    out = ctx7.pair_clearance(coef, dur, np.zeros((0, 2), dtype=np.int32))
    assert all(x.shape == (0,) for x in out)


def test_outputs_are_the_bits_recorded_before_the_pair_kernels_were_merged(ctx7, ctx9):
    """tests/golden/clearance_bits_golden.npz holds what msnap_pair_clearance computed when it had a kernel file of its
    own (tests/golden/make_clearance_bits_golden.py): 1, 2 and 10 segments with every pair both ways round, a shared
    grid, unequal totals, invalid pairs, a zero duration and a NaN coefficient at order 7, 4 segments at order 9.  The
    host and the device entry give every stored bit."""
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute
    dev = torch.device("cuda", 0)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    cases = CC.bits_cases("pair")
    assert len(cases) == 7 and sorted(int(c["order"]) for _, c in cases) == [7] * 6 + [9]
    for order, host in ((7, ctx7), (9, ctx9)):
        with Context(device_id=0, order=order, max_segments=16) as ctx:
            comp = DeviceCompute(ctx, torch)
            for name, c in cases:
                if int(c["order"]) != order:
                    continue
                CC.check_bits(name + ", host entry", host.pair_clearance(c["coef"], c["dur"], c["pairs"]), c)
                out = comp.pair_clearance(tt(c["coef"]), tt(c["dur"]), tt(c["pairs"]))
                torch.cuda.synchronize()
                CC.check_bits(name + ", device entry", out, c)


def test_certify_clearance_on_the_formation_swarm(ctx7):
    import torch
    from drone_path_planning_python_amd import Context, synthetic
    from drone_path_planning_python_amd.swarm import DeviceCompute, certify_clearance
    fgold = np.load(os.path.join(GOLDEN_DIR, "formation_golden.npz"))
    rb, off, t = synthetic.formation_config(2)
    G, m, _ = rb.shape
    poses = ctx7.formation_transform(rb.reshape(G * m, 7), off)
    N = 512
    wp = synthetic.formation_waypoints(poses, G)[:N]
    coef, dur = _solve(ctx7, wp, t)
    S = synthetic.formation_sample_count(t)
    radius = synthetic.DRONE_RADIUS
    assert fgold["cfg2_pair_min_dist"].shape == (4096,)
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        comp = DeviceCompute(ctx, torch)
        dev = torch.device("cuda", 0)
        res = certify_clearance(comp, torch.from_numpy(coef).to(dev), torch.from_numpy(dur).to(dev), radius,
                                synthetic.SAMPLE_DT, S)
        torch.cuda.synchronize()
    hit, cleared = res.hit.cpu().numpy(), res.cleared_by_sampling.cpu().numpy()
    shit, spartner = res.sampled_hit.cpu().numpy().astype(bool), res.sampled_partner.cpu().numpy()
    cl = res.certified_lower.cpu().numpy()
    print(f"formation swarm {N}: |U| {res.n_uncertain}, pairs {res.pairs.shape[0]}, sampled hits {int(shit.sum())}, "
          f"certified hits {int(hit.sum())}, undecided {int(res.undecided.sum())}, gap {res.gap}")
    assert shit.any() and (hit[shit]).all()                  # every sampled hit is a certified hit
    assert not res.undecided.any()
    rng = np.random.default_rng(512)
    chosen = rng.choice(N, size=50, replace=False)
    check = np.unique(np.concatenate([chosen, np.nonzero(cleared)[0][:8]]))
    pairs = np.stack([check, spartner[check]], axis=1)
    cands = CE.candidate_intervals(coef, dur, pairs)
    for k, (a, b) in enumerate(pairs):
        D, _, _ = CE.exact_clearance(coef[a], dur[a], coef[b], dur[b], cands[k])
        D = float(D)
        if a in chosen:
            assert cl[a] <= D * (1 + CE.REL_ROUND) + CE.ABS_ROUND, (a, b, cl[a], D)
        if cleared[a]:
            assert D >= 2 * radius, (a, b, D)


def test_certify_clearance_on_an_awkward_swarm_every_pair(ctx7):
    """clearance_cases.awkward_swarm: 12 drones at +5000 m, two pairs crossing between samples, one pair touching at
    exactly 2 radius, one drone that lands early.  All 66 pairs against the exact reference."""
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.swarm import DeviceCompute, certify_clearance
    coef, dur = CC.awkward_swarm(lambda wp, t, nc: _solve(ctx7, wp, t))
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        comp = DeviceCompute(ctx, torch)
        dev = torch.device("cuda", 0)
        res = certify_clearance(comp, torch.from_numpy(coef).to(dev), torch.from_numpy(dur).to(dev), CC.AWKWARD_RADIUS,
                                CC.AWKWARD_DT, CC.AWKWARD_SAMPLES)
        torch.cuda.synchronize()
        got = {k: getattr(res, k).cpu().numpy() for k in ("certified_lower", "hit", "undecided", "cleared_by_sampling",
                                                          "pairs")}
    CC.check_certified(got, coef, dur)


def test_a_captured_call_replays_to_the_eager_result():
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.synthetic import swarm
    dev = torch.device("cuda", 0)
    with Context(device_id=0, order=7, max_segments=16) as ctx:
        wp, t = swarm(7500, 64, 5)
        coef, dur, status = ctx.solve_batch(wp, t)
        assert (status == 0).all()
        rng = np.random.default_rng(5)
        a = rng.integers(0, 64, size=300)
        pairs = np.stack([a, (a + rng.integers(1, 64, size=300)) % 64], axis=1).astype(np.int32)
        eager = ctx.pair_clearance(coef, dur, pairs)
        side = torch.cuda.Stream()
        P = pairs.shape[0]
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            tc, td, tp = (torch.from_numpy(x).to(dev) for x in (coef, dur, pairs))
            md = torch.empty((P,), dtype=torch.float64, device=dev)
            tm, lower = torch.empty_like(md), torch.empty_like(md)
            st = torch.empty((P,), dtype=torch.int32, device=dev)
            ctx.pair_clearance_device(64, 5, tc, td, P, tp, md, tm, lower, st)      # once eagerly: the scratch has its size
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                ctx.pair_clearance_device(64, 5, tc, td, P, tp, md, tm, lower, st)
            ctx.set_stream(side.cuda_stream)
            for _ in range(2):
                for x in (md, tm, lower, st):
                    x.zero_()
                g.replay()
                side.synchronize()
                for got, want in zip((md, tm, lower, st), eager):
                    assert np.array_equal(got.cpu().numpy(), want)
        ctx.use_own_stream()
