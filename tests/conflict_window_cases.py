"""Hand-built and seeded inputs of the conflict windows (include/msnap.h, "conflict windows"), shared by
tests/test_conflict_window_cpu.py (the NumPy restatement) and tests/test_conflict_window_gpu.py (the kernel).  Every
case is (A, B, pairs, threshold) with A, B = (coef [N, M, 4, nc], dur [N, M], t0 [N] or None), solved by the C oracle so
that both files see the same numbers: what the CPU file proves about a fixture (only transversal crossings) holds for
the GPU file's run of it.  The check_* functions are the test bodies; `ctx` is a Context of the right order or
conflict_exact.RestatedContext."""
from __future__ import annotations

import numpy as np

import c_oracle
import clearance_cases as CC
import conflict_exact as KE
import cross_clearance_cases as XC

T_RES = (1e-3, 1e-6, 1e-9)


def solve(wp, t, nc):
    coef, dur, info, _ = c_oracle.solve_batch(wp, t, ncoef=nc)
    assert not info.any()
    return coef, dur


def one_crossing(nc=8, t0_a=3.7, t0_b=3.7):
    """1 x 1 segment: the crossing the 0.1 s samples miss (cross_clearance_cases.crossing), both drones through one
    point at t0 + 0.55 s: one lane, one conflict, 0.25 m."""
    return XC.crossing(solve, nc, t0_a, t0_b) + (0.25,)


def unequal(nc=8, ma=3, mb=10, threshold=2.5):
    """(ma, mb) = (3, 10) with offsets: slots, ties, coincident knots; every other pair of
    ALL15, at 2.5 m (order 9, (2, 5): 4 m): about half of them are in conflict, one of them already at S, one twice."""
    A, B, pairs = XC.unequal(solve, nc, ma, mb)
    return A, B, pairs[::2].copy(), threshold


def far_origin():
    A, B, pairs = XC.far_origin(solve)
    return A, B, pairs[::2].copy(), 2.5


def far_clock():
    A, B, pairs = XC.far_clock(solve, offset=5000.0)
    return A, B, pairs[::2].copy(), 2.5


def windows(threshold):
    """cross_clearance_cases.windows: pair 0 W < S, pair 1 W == S (4.83 m apart at that instant), pairs 2 and 3 windows
    that start / end inside a segment (7.04 m, and 4.81 m at the window's end)."""
    return XC.windows(solve) + (threshold,)


def inside_one_segment(nc=8):
    """The window lies strictly inside B's single segment: A (1 segment, 1.1 s) starts 0.2 s after B."""
    return XC.crossing(solve, nc, 3.9, 3.7) + (1.0,)


def ends(nc=8):
    """clearance_cases.ends_case against the hover at the origin, threshold 1.75 m: drone 1 (x = 1 + t) is in conflict at
    S = 0 and leaves at 0.75 s; drone 2 (x = 3 - t, then 2 - t / 2) enters at 1.5 s and is in conflict at W = 2."""
    coef, dur = CC.ends_case(nc)
    return (coef, dur, None), (coef, dur, None), np.array([[0, 1], [0, 2], [1, 0]], dtype=np.int32), 1.75


def two_conflicts(nc=8):
    """A hover at the origin and x(t) = 0.5 + (t - 1)^2 (t - 3)^2, y = 0.3 on [0, 4], as one segment (drone 1) and cut
    at t = 2 (drone 2, Taylor shift by hand): closer than 1 m around t = 1 and around t = 3, 1.53 m apart at t = 2."""
    x = [9.5, -24.0, 22.0, -8.0, 1.0]
    x2 = [1.5, 0.0, -2.0, 0.0, 1.0]          # the same in (t - 2)
    coef, dur = CC.hand([[[[0.0], [0.0], [0.0]]] * 2, [[x, [0.3], [0.0]], [x, [0.3], [0.0]]], [[x, [0.3], [0.0]], [x2, [0.3], [0.0]]]],
                        [[2.0, 2.0], [4.0, 1.0], [2.0, 2.0]], nc)
    return (coef, dur, None), (coef, dur, None), np.array([[0, 1], [0, 2]], dtype=np.int32), 1.0


def tangent(nc=8):
    """A hover at the origin and x(t) = 0.25 + (t - 1)^2 on [0, 2]: the distance touches 0.25 m at t = 1 and is never
    below it.  Symmetric about the middle of the one interval."""
    coef, dur = CC.hand([[[[0.0], [0.0], [0.0]]], [[[1.25, -2.0, 1.0], [0.0], [0.0]]]], [[2.0], [2.0]], nc)
    return (coef, dur, None), (coef, dur, None), np.array([[0, 1]], dtype=np.int32), 0.25


# the fixtures of the closing checks (check 4): tests/test_conflict_window_cpu.py asserts that each has only transversal
# crossings, so that none of their pairs has to be excluded as a graze
CLOSING = {
    "one crossing, order 7": lambda: one_crossing(8),
    "one crossing, order 9": lambda: one_crossing(10),
    "unequal (3, 10)": unequal,
    "unequal (2, 5), order 9": lambda: unequal(10, 2, 5, 4.0),
    "far origin": far_origin,
    "far clock": far_clock,
    "windows, 5 m": lambda: windows(5.0),
    "windows, 4 m": lambda: windows(4.0),
    "inside one segment": inside_one_segment,
    "ends": ends,
    "two conflicts": two_conflicts,
}


_MEMO = {}


def fixture(name):
    """(A, B, pairs, threshold, exact_of) of a CLOSING fixture, built once."""
    if name not in _MEMO:
        A, B, pairs, threshold = CLOSING[name]()
        _MEMO[name] = (A, B, pairs, threshold, KE.exact_of(A, B, pairs, threshold))
    return _MEMO[name]


def run(ctx, name, t_res=1e-6, restated=False, **kw):
    A, B, pairs, threshold, kw["exact"] = fixture(name)
    ref = None
    if restated:
        ref = KE.fp64_conflict_window(A[0], A[1], A[2], B[0], B[1], B[2], pairs, threshold, t_res)
    return (A, B, pairs, threshold), KE.check_windows(ctx, A, B, pairs, threshold, t_res, restated=ref, **kw)


def check_one_crossing(ctx, nc, **kw):
    _, (cu, tf, df, tl, dl, cf, _) = run(ctx, f"one crossing, order {nc - 1}", verdict=["conflict"], **kw)
    assert 3.7 + 0.5 < tf[0] < 3.7 + 0.55 < tl[0] < 3.7 + 0.6 and df[0] < 0.25 and dl[0] < 0.25


def check_unequal(ctx, nc=8, **kw):
    name = "unequal (3, 10)" if nc == 8 else "unequal (2, 5), order 9"
    (A, B, pairs, _), (cu, tf, df, tl, dl, cf, _) = run(ctx, name, **kw)
    found = np.isfinite(tf)
    assert 3 <= found.sum() < len(pairs)
    # some conflict enters in one slot and leaves in another: a knot of either drone lies strictly inside it
    (ca, da, ta), (cb, db, _) = A, B
    spans = 0
    for k in np.nonzero(found)[0]:
        a, b = pairs[k]
        kn = np.concatenate([ta[a] + np.add.accumulate(da[a]), np.add.accumulate(db[b])])
        spans += bool(((kn > tf[k]) & (kn < tl[k])).any())
    assert spans >= 1


def check_ends(ctx, **kw):
    _, (cu, tf, df, tl, dl, cf, _) = run(ctx, "ends", verdict=["conflict"] * 3, **kw)
    assert tf[0] == cu[0] == 0.0 and abs(tl[0] - 0.75) <= 1e-6 and abs(cf[0] - 0.75) <= 2e-6      # in conflict at S
    assert tl[1] == cf[1] == 2.0 and abs(tf[1] - 1.5) <= 1e-6                                      # in conflict at W
    assert all(x[2] == x[0] for x in (cu, tf, df, tl, dl, cf))                                     # (b, a) is (a, b)


def check_two_conflicts(ctx, **kw):
    """The first entry comes from the first conflict, the last exit from the second; the gap between is not reported."""
    _, (cu, tf, df, tl, dl, cf, _) = run(ctx, "two conflicts", verdict=["conflict"] * 2, **kw)
    for k in range(2):
        assert 0.0 < cu[k] <= tf[k] < 1.0 and 3.0 < tl[k] <= cf[k] < 4.0, (k, tf[k], tl[k])


def check_never_close(ctx):
    """Set B of `unequal` moved 100 m away, threshold 0.05 m: certified clear, and in the restatement the root's bound
    (or its children's) proves every lane -- at most 3 nodes: the prune at the root works."""
    A, (cb, db, tb), pairs, _ = unequal()
    B, pairs = (CC.moved(CC.quantised(cb), (100.0, 0.0, 0.0)), db, tb), pairs[:3]
    KE.check_windows(ctx, A, B, pairs, 0.05, verdict=["clear"] * len(pairs))
    st = {}
    KE.fp64_conflict_window(A[0], A[1], A[2], B[0], B[1], B[2], pairs, 0.05, stats=st)
    print("nodes per lane and direction: max", st["nodes"].max(), "mean", st["nodes"].mean())
    assert st["lanes"] > 0 and st["nodes"].max() <= 3


def check_tangent(ctx):
    """Clear by the strict rule: certified clear or undecided pass (checks 1 and 5), a conflict fails."""
    A, B, pairs, threshold = tangent()
    cu, tf, df, tl, dl, cf, _ = KE.check_windows(ctx, A, B, pairs, threshold, cross=False, closing=False)
    assert tf[0] == np.inf and tl[0] == -np.inf and df[0] == np.inf and dl[0] == np.inf
    print("tangency:", "certified clear" if cu[0] == np.inf else f"undecided from {cu[0]!r} to {cf[0]!r}")


def check_windows_cases(ctx, **kw):
    """W < S: certified clear.  W == S: the one instant decides (4.83 m: in conflict at 5 m, clear at 4 m).  Windows that
    start or end inside a segment; pair 3 is still in conflict at W at 5 m."""
    _, (cu, tf, df, tl, dl, cf, _) = run(ctx, "windows, 5 m", verdict=["clear", "conflict", "clear", "conflict"], **kw)
    assert cu[1] == tf[1] == tl[1] == cf[1] == 1.75 and df[1] == dl[1] and 4.8 < df[1] < 4.9
    assert tl[3] == cf[3] == 1.75
    run(ctx, "windows, 4 m", verdict=["clear"] * 4, **kw)
    run(ctx, "inside one segment", verdict=["conflict"], **kw)


def check_far(ctx, **kw):
    """5000 m from the origin, and t0 = 1e4 s: the allowance r with its R and clock terms."""
    for name in ("far origin", "far clock"):
        _, out = run(ctx, name, **kw)
        assert np.isfinite(out[1]).sum() >= 3


def check_threshold_zero(ctx):
    """No conflict ever, even where the paths cross (D = 0): the inequality is strict."""
    for A, B, pairs, _ in (one_crossing(8), unequal()):
        cu, tf, df, tl, dl, cf, _ = KE.check_windows(ctx, A, B, pairs[:2], 0.0, closing=False)
        assert (tf == np.inf).all() and (tl == -np.inf).all()


def check_t_res(ctx, **kw):
    """The closing gap follows t_res (check 4 at each), and a finer resolution moves the bracket inwards."""
    gaps = []
    for t_res in T_RES:
        _, (cu, tf, df, tl, dl, cf, _) = run(ctx, "one crossing, order 7", t_res=t_res, **kw)
        gaps.append(max(tf[0] - cu[0], cf[0] - tl[0]))
    print("closing gaps:", gaps)
    assert gaps[0] > 1e-6 >= gaps[1] > 1e-9 and gaps[2] <= 1.01e-9


# ------------------------------------------------------------------------------------------------ identities
def identity_list(n=65):
    """65 pairs (more than one wave, and a partial one) of `unequal`, with repeats."""
    A, B, pairs, threshold = unequal()
    rng = np.random.default_rng(65)
    return A, B, pairs[rng.integers(0, len(pairs), size=n)].copy(), threshold


def same(x, y):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y))


def check_identities(ctx):
    """Place in the list and its length; NULL against zeros; the sets exchanged with the pairs flipped; A == B with
    zero offsets against the pair entry; (b, a) against (a, b)."""
    (ca, da, ta), (cb, db, _), pairs, thr = identity_list()
    ref = ctx.cross_conflict_window(ca, da, cb, db, pairs, thr, t0_a=ta)
    assert (ref[6] == 0).all() and np.isfinite(ref[1]).any() and not np.isfinite(ref[1]).all()
    assert same(ref, ctx.cross_conflict_window(cb, db, ca, da, pairs[:, ::-1].copy(), thr, t0_b=ta))
    assert same(ref, ctx.cross_conflict_window(ca, da, cb, db, pairs, thr, t0_a=ta, t0_b=np.zeros(6)))
    rev = ctx.cross_conflict_window(ca, da, cb, db, pairs[::-1].copy(), thr, t0_a=ta)
    assert same(ref, [x[::-1] for x in rev])
    one = ctx.cross_conflict_window(ca, da, cb, db, pairs[40:41], thr, t0_a=ta)
    assert same([x[40:41] for x in ref], one)
    distinct = pairs[pairs[:, 0] != pairs[:, 1]]
    want = ctx.pair_conflict_window(cb, db, distinct, thr)
    assert np.isfinite(want[1]).any()
    for t0 in (None, np.zeros(6)):
        assert same(want, ctx.cross_conflict_window(cb, db, cb, db, distinct, thr, t0_a=t0, t0_b=t0))
    assert same(want, ctx.pair_conflict_window(cb, db, distinct[:, ::-1].copy(), thr))
    return ref


# ------------------------------------------------------------------------------------------------ swarm helpers
def check_swarm_windows(res, t_replan, coef, dur, margin):
    """swarm.conflict_windows / latest_replan_time on clearance_cases.awkward_swarm (at the origin): the two drones of
    each crossing get the start of their window, the others +inf."""
    f = lambda x: np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x)      # noqa: E731
    first, t_r, pairs, cu = f(res.first_conflict), f(t_replan), f(res.pairs).tolist(), f(res.t_clear_until)
    assert [0, 1] in pairs and [2, 3] in pairs
    for a, b in ((0, 1), (2, 3)):
        k = pairs.index([a, b])
        pcs, _ = KE.pieces(coef[a], dur[a], 0.0, coef[b], dur[b], 0.0)
        ranges, _, _ = KE.exact_crossings(pcs, 2 * CC.AWKWARD_RADIUS)
        assert len(ranges) == 1 and -1e-9 <= float(ranges[0][0]) - cu[k] <= 2e-6
        assert first[a] == first[b] == cu[k]
        assert t_r[a] == t_r[b] == max(cu[k] - margin, 0.0)
    assert np.isinf(first[4:]).all() and np.isinf(t_r[4:]).all()


def check_replan_windows(res, coef, dur, new_coef, new_dur):
    """swarm.replan_conflict_windows on cross_clearance_cases.replan_swarm: certify_replan's pairs; the replanned
    drones that hit (REPLAN_HIT) get the start of their first conflict, the clear one +inf."""
    f = lambda x: np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x)      # noqa: E731
    first, pairs, cu, tf = f(res.first_conflict), f(res.pairs), f(res.t_clear_until), f(res.t_first)
    idx, t_r, n, K = XC.REPLAN_IDX, XC.REPLAN_T_R, coef.shape[0], len(XC.REPLAN_IDX)
    stay = [j for j in range(n) if j not in idx]
    want = [(idx[i], j) for i in range(K) for j in stay] + [(idx[i], idx[j]) for i in range(K) for j in range(i + 1, K)]
    assert pairs.tolist() == [list(p) for p in want]
    assert np.isfinite(first).tolist() == XC.REPLAN_HIT
    loc = {d: k for k, d in enumerate(idx)}
    for k, (a, b) in enumerate(want):
        B = (new_coef[loc[b]], new_dur[loc[b]], t_r[loc[b]]) if b in loc else (coef[b], dur[b], 0.0)
        pcs, _ = KE.pieces(new_coef[loc[a]], new_dur[loc[a]], t_r[loc[a]], *B)
        ranges, _, _ = KE.exact_crossings(pcs, 2 * XC.REPLAN_RADIUS)
        assert bool(ranges) == bool(np.isfinite(tf[k])), (a, b)
        if ranges:
            assert -1e-9 <= float(ranges[0][0]) - cu[k] <= 2e-6, (a, b)
            assert first[loc[a]] <= cu[k] and (b not in loc or first[loc[b]] <= cu[k])
