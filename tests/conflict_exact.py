"""References for the conflict windows (include/msnap.h, "conflict windows"), test side only.

Exact.  `pieces` gives, per interval between consecutive exact knots of the two drones inside the window [S, W]
(cross_clearance_exact's rules: coefficients, running sums and offsets as Fractions), g = |p_a - p_b|^2 as an exact
rational polynomial in the time since the interval's start.  From those:
  exact_infimum      the infimum of the distance over any sub-range [t0, t1] of the window (clearance_exact's
                     exact_interval_min on the clipped intervals);
  exact_crossings    the real roots of g - threshold^2 (mpmath.polyroots at 60 digits on the square-free part where
                     they are multiple), the
                     maximal open ranges on which the pair is in conflict, hence the exact first-entry and last-exit
                     times, and the crossing speed |d/dt distance| at every entry and exit;
  the exact distance at a time is cross_clearance_exact.exact_cross_distance_at.
fp64_conflict_window: a plain NumPy fp64 restatement of the lane and fold rules of csrc/msnap_conflict.hip, vectorised
over the (pair, interval) lanes.  Not bit-exact with the kernel (no fused multiply-add here).
check_windows: the per-pair checks of the issue against the exact reference, shared by the CPU and the GPU tests."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

import clearance_exact as CE
import cross_clearance_exact as XE
from clearance_exact import DPS, MAX_DEPTH, MAX_NODES, _mpf, _shift, _squarefree, _t0, exact_interval_min, knots
from dyadic_walk import ABS_ROUND, EPS, _bernstein_weights, _positions, _taylor, trailing_ones

OUTPUTS = ("t_clear_until", "t_first", "d_first", "t_last", "d_last", "t_clear_from")


# ------------------------------------------------------------------------------------------------ exact
def pieces(coef_a, dur_a, t0a, coef_b, dur_b, t0b):
    """[(t0, t1, g)] over the window, t0 < t1 Fractions on the common clock, g ascending Fractions in (t - t0); for
    W == S one piece (S, S, g); [] for W < S.  Also returns (S, W) as Fractions."""
    S, W = XE.window(dur_a, t0a, dur_b, t0b)
    if W < S:
        return [], (Fraction(S), Fraction(W))
    S, W = Fraction(S), Fraction(W)
    ta, tb = Fraction(float(t0a)), Fraction(float(t0b))
    ka = [ta + Fraction(x) for x in knots(dur_a)]
    kb = [tb + Fraction(x) for x in knots(dur_b)]
    sa, sb = [ta] + ka[:-1], [tb] + kb[:-1]
    cuts = sorted({S, W} | {x for x in ka + kb if S < x < W})
    ca, cb = np.asarray(coef_a, dtype=np.float64), np.asarray(coef_b, dtype=np.float64)

    def g_at(t0, t1):
        ia, ib = XE._segment(ka, t1), XE._segment(kb, t1)
        g = [Fraction(0)] * (2 * ca.shape[2] - 1)
        for ax in range(3):
            pa = _shift([Fraction(float(x)) for x in ca[ia, ax]], t0 - sa[ia])
            pb = _shift([Fraction(float(x)) for x in cb[ib, ax]], t0 - sb[ib])
            d = [x - y for x, y in zip(pa, pb)]
            for i, x in enumerate(d):
                if x:
                    for j, y in enumerate(d):
                        g[i + j] += x * y
        return g

    if len(cuts) == 1:
        return [(S, S, g_at(S, S))], (S, W)
    return [(t0, t1, g_at(t0, t1)) for t0, t1 in zip(cuts[:-1], cuts[1:])], (S, W)


def exact_infimum(pcs, lo, hi):
    """The infimum of the distance over [lo, hi] (floats or Fractions inside the window) as mpf; +inf for an empty
    range."""
    lo, hi = Fraction(lo), Fraction(hi)
    best = None
    with mpmath.workdps(DPS):
        for t0, t1, g in pcs:
            a, b = max(t0, lo), min(t1, hi)
            if a > b:
                continue
            v, _ = exact_interval_min(_shift(g, a - t0), a, b) if b > a else (_mpf(_shift(g, a - t0)[0]), None)
            best = v if best is None or v < best else best
        return mpmath.inf if best is None else mpmath.sqrt(max(best, mpmath.mpf(0)))


def _real_roots(p, h):
    """The real roots of p (ascending Fractions) in [0, h], each once, as sorted mpf."""
    p = list(p)
    while p and p[-1] == 0:
        p.pop()
    if len(p) < 2:
        return []
    q = list(p)
    while q and q[0] == 0:          # a root at 0 is a candidate already
        q.pop(0)
    if len(q) < 2:
        return []
    try:
        roots = mpmath.polyroots([_mpf(x) for x in reversed(q)], maxsteps=200, extraprec=DPS)
    except mpmath.libmp.NoConvergence:            # multiple roots: the square-free part has the same ones, each once
        q = _squarefree(q)
        roots = mpmath.polyroots([_mpf(x) for x in reversed(q)], maxsteps=4000, extraprec=20 * DPS) if len(q) >= 2 else []
    out = []
    for z in roots:
        z = mpmath.mpc(z)
        if abs(z.imag) <= mpmath.mpf(10) ** (-DPS // 2) * (1 + abs(z.real)) and 0 <= z.real <= h:
            out.append(z.real)
    return sorted(out)


def exact_crossings(pcs, threshold):
    """The ranges on which the exact distance is < threshold: (ranges, speeds, touches).  ranges: [(t_in, t_out)] as
    mpf, maximal, in time order (a range that starts at S or ends at W is closed there by the window); speeds: the
    crossing speed |d/dt distance| [m/s] at every entry and exit that is a root (not the window's ends); touches: the
    roots at which the distance only touches the threshold from above (no range on either side)."""
    L = Fraction(float(threshold)) ** 2
    raw, speeds, touches = [], [], []
    with mpmath.workdps(DPS):
        for t0, t1, g in pcs:
            p = [g[0] - L] + list(g[1:])
            pm = [_mpf(x) for x in reversed(p)]
            dm = [_mpf((i + 1) * p[i + 1]) for i in range(len(p) - 1)][::-1]
            if t1 == t0:
                if p[0] < 0:
                    raw.append((_mpf(t0), _mpf(t0), None, None))
                continue
            h = _mpf(t1 - t0)
            c = [mpmath.mpf(0)] + [r for r in _real_roots(p, h) if 0 < r < h] + [h]
            inside = [mpmath.polyval(pm, (x + y) / 2) < 0 for x, y in zip(c[:-1], c[1:])]
            for k, (x, y) in enumerate(zip(c[:-1], c[1:])):
                if inside[k]:
                    raw.append((_mpf(t0) + x, _mpf(t0) + y, x if k > 0 else None, y if k < len(inside) - 1 else None))
                    for r in (raw[-1][2], raw[-1][3]):
                        if r is not None:
                            speeds.append(abs(mpmath.polyval(dm, r)) / (2 * mpmath.mpf(float(threshold))))
            for k in range(1, len(c) - 1):
                if not inside[k - 1] and not inside[k]:
                    touches.append(_mpf(t0) + c[k])
        ranges = []
        for t_in, t_out, _, _ in raw:          # ranges that continue across a knot are one
            if ranges and ranges[-1][1] == t_in:
                ranges[-1] = (ranges[-1][0], t_out)
            else:
                ranges.append((t_in, t_out))
    return ranges, speeds, touches


# ------------------------------------------------------------------------------------------------ fp64 restatement
def _first_crossing(e, h, L, t_res, Wt):
    """csrc/msnap_conflict.hip, first_crossing, for the lanes e [n, 3, D + 1] of lengths h [n]: (hit_u, clear_u, nodes)."""
    n, D = len(h), e.shape[2] - 1
    hit, clear = np.full(n, np.inf), np.full(n, np.inf)
    idx, lvl, nodes = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    act = np.arange(n)
    while len(act):
        hh = np.ldexp(1.0, -lvl[act])
        a = idx[act].astype(np.float64) * hh
        G = np.zeros((len(act), 2 * D + 1))
        g0, gm, g1 = np.zeros(len(act)), np.zeros(len(act)), np.zeros(len(act))
        scale = hh[:, None] ** np.arange(D + 1)
        for s in range(3):
            f = _taylor(e[act, s, :], a) * scale
            for i in range(D + 1):
                G[:, i:i + D + 1] += f[:, i:i + 1] * f
            vm = np.zeros(len(act))
            for j in range(D, -1, -1):
                vm = vm * 0.5 + f[:, j]
            v1 = f[:, ::-1].cumsum(axis=1)[:, -1]
            g0 += f[:, 0] ** 2
            gm += vm ** 2
            g1 += v1 ** 2
        bound = (G @ Wt.T).min(axis=1)
        open_ = ~(bound >= L)
        at_start = open_ & (g0 < L)
        leaf = (h[act] * hh <= t_res) | (lvl[act] >= MAX_DEPTH)
        in_mid, at_end = gm < L, g1 < L
        found = at_start | (open_ & leaf & (in_mid | at_end))
        undecided = open_ & ~found & leaf
        split = open_ & ~found & ~leaf
        at = np.where(at_start, a, np.where(in_mid, a + 0.5 * hh, a + hh))
        ix = idx[act]
        up = trailing_ones(ix)
        nodes[act] += 1
        finished = ~split & (up == lvl[act])
        guard = ~finished & (nodes[act] >= MAX_NODES)
        hit[act] = np.where(found, at, hit[act])
        clear[act] = np.where(found | undecided | guard, np.fmin(clear[act], a), clear[act])
        idx[act] = np.where(split, ix << np.uint64(1), (ix >> up.astype(np.uint64)) + np.uint64(1))
        lvl[act] = np.where(split, lvl[act] + 1, lvl[act] - up)
        act = act[~(found | finished | guard)]
    return hit, clear, nodes


def fp64_conflict_window(coef_a, dur_a, t0_a, coef_b, dur_b, t0_b, pairs, threshold, t_res=1e-6, stats=None):
    """coef_x [Nx, Mx, 4, nc], dur_x [Nx, Mx], t0_x [Nx] or None, pairs [P, 2] (valid, finite) -> the six arrays of
    OUTPUTS, by the kernel's method in NumPy fp64.  `stats` receives the nodes per live lane and direction ("nodes"
    [L, 2]) and the lane count ("lanes")."""
    coef_a, coef_b = np.asarray(coef_a, dtype=np.float64), np.asarray(coef_b, dtype=np.float64)
    dur_a, dur_b = np.asarray(dur_a, dtype=np.float64), np.asarray(dur_b, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P, Ma, Mb, nc = len(pairs), dur_a.shape[1], dur_b.shape[1], coef_a.shape[3]
    D = nc - 1
    Wt = _bernstein_weights(2 * D)
    a_i, b_i = pairs[:, 0], pairs[:, 1]
    ta, tb = _t0(t0_a, dur_a.shape[0])[a_i], _t0(t0_b, dur_b.shape[0])[b_i]
    # the lane set-up of clearance_exact.fp64_cross_clearance (csrc/msnap_pair_interval.h)
    LA, LB = np.add.accumulate(dur_a[a_i], axis=1), np.add.accumulate(dur_b[b_i], axis=1)
    KA, KB = ta[:, None] + LA, tb[:, None] + LB
    S, Wend = np.maximum(ta, tb), np.minimum(KA[:, -1], KB[:, -1])
    ends = np.concatenate([KA[:, :Ma - 1], KB[:, :Mb - 1], Wend[:, None]], axis=1)
    ends = np.sort(np.maximum(np.minimum(ends, Wend[:, None]), S[:, None]), axis=1)
    starts = np.concatenate([S[:, None], ends[:, :-1]], axis=1)
    h_all = ends - starts
    live = (h_all > 0) & (Wend >= S)[:, None]
    pi, si = np.nonzero(live)
    E, t0, h = ends[pi, si], starts[pi, si], h_all[pi, si]
    Ln = len(pi)
    e = np.zeros((Ln, 3, D + 1))
    for coef, drone, K, Lk, tx, M, sign in ((coef_a, a_i[pi], KA[pi], LA[pi], ta[pi], Ma, 1.0),
                                            (coef_b, b_i[pi], KB[pi], LB[pi], tb[pi], Mb, -1.0)):
        seg = np.minimum((E[:, None] > K).sum(axis=1), M - 1)
        off = np.concatenate([np.zeros((Ln, 1)), Lk], axis=1)[np.arange(Ln), seg]
        for ax in range(3):
            e[:, ax, :] += sign * _taylor(coef[drone, seg, ax, :], (t0 - tx) - off)
    e *= (h[:, None] ** np.arange(D + 1))[:, None, :]

    L = float(threshold) * float(threshold)
    hit_f, clear_f, nodes_f = _first_crossing(e, h, L, t_res, Wt)
    back = np.stack([_taylor(e[:, s, :], np.ones(Ln)) for s in range(3)], axis=1)      # e_s(1 - u)
    back[:, :, 1::2] *= -1.0
    hit_b, clear_b, nodes_b = _first_crossing(back, h, L, t_res, Wt)
    fwd = lambda u: np.where(np.isfinite(u), np.minimum(h * np.where(np.isfinite(u), u, 0.0) + t0, E), np.inf)      # noqa: E731
    bwd = lambda u: np.where(np.isfinite(u), np.maximum(E - h * np.where(np.isfinite(u), u, 0.0), t0), -np.inf)     # noqa: E731

    tf, cu, tl, cf = np.full(P, np.inf), np.full(P, np.inf), np.full(P, -np.inf), np.full(P, -np.inf)
    np.minimum.at(tf, pi, fwd(hit_f))
    np.minimum.at(cu, pi, fwd(clear_f))
    np.maximum.at(tl, pi, bwd(hit_b))
    np.maximum.at(cf, pi, bwd(clear_b))
    lo = np.minimum(tf, np.where(tl > -np.inf, tl, np.inf))
    hi = np.maximum(tl, np.where(tf < np.inf, tf, -np.inf))
    tf, tl = lo, hi
    cu, cf = np.minimum(cu, tf), np.maximum(cf, tl)
    instant = Wend == S
    tf, tl = np.where(instant, S, tf), np.where(instant, S, tl)

    def dist(t):
        t = np.where(np.isfinite(t), t, S)
        tau_a = np.minimum(np.maximum(t - ta, 0.0), LA[:, -1])
        tau_b = np.minimum(np.maximum(t - tb, 0.0), LB[:, -1])
        d = _positions(coef_a, dur_a, a_i, tau_a) - _positions(coef_b, dur_b, b_i, tau_b)
        return np.sqrt(d[:, 2] ** 2 + (d[:, 1] ** 2 + d[:, 0] ** 2))

    found = np.isfinite(tf)
    df, dl = np.where(found, dist(tf), np.inf), np.where(found, dist(tl), np.inf)
    in_conflict = instant & (df < threshold)
    clear_instant = instant & ~in_conflict
    cu, cf = np.where(in_conflict, S, cu), np.where(in_conflict, S, cf)
    none = clear_instant | (Wend < S)
    cu, tf, df, dl = (np.where(none, np.inf, x) for x in (cu, tf, df, dl))
    tl, cf = np.where(none, -np.inf, tl), np.where(none, -np.inf, cf)
    if stats is not None:
        stats["nodes"], stats["lanes"], stats["lane_pair"] = np.stack([nodes_f, nodes_b], axis=1), Ln, pi
    return cu, tf, df, tl, dl, cf


class RestatedContext(XE.RestatedContext):
    """fp64_conflict_window behind Context's two conflict-window methods, beside cross_clearance_exact's stand-ins:
    the CPU tests run the GPU tests' checks on the restatement."""

    def cross_conflict_window(self, coef_a, dur_a, coef_b, dur_b, pairs, threshold, t_res=1e-6, t0_a=None, t0_b=None):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        out = fp64_conflict_window(coef_a, dur_a, t0_a, coef_b, dur_b, t0_b, pairs, threshold, t_res)
        return out + (np.zeros(len(pairs), dtype=np.int32),)

    def pair_conflict_window(self, coef, dur, pairs, threshold, t_res=1e-6):
        return self.cross_conflict_window(coef, dur, coef, dur, pairs, threshold, t_res)


# ------------------------------------------------------------------------------------------------ the allowance
def allowance(args, cross=True):
    """r of include/msnap.h for one pair, args = (coef_a, dur_a, t0a, coef_b, dur_b, t0b): the cross entry's, or (one
    batch on one clock) the pair entry's."""
    if cross:
        return XE.allowance(XE.pair_R(*args), XE.T_c(args[1], args[2], args[4], args[5]), XE.pair_Rprime(*args))
    return CE.round_terms(CE.pair_R(args[0], args[1], args[3], args[4]))


def ulp(x):
    return float(np.spacing(abs(float(x))))


# ------------------------------------------------------------------------------------------------ shared test helper
def exact_of(A, B, pairs, threshold):
    """Per pair (pieces, (S, W), exact_crossings) -- computed once per fixture and shared by the tests that need it."""
    (ca, da, t0a), (cb, db, t0b) = A, B
    ta, tb = _t0(t0a, len(da)), _t0(t0b, len(db))
    out = []
    for a, b in np.asarray(pairs).reshape(-1, 2):
        pcs, SW = pieces(ca[a], da[a], ta[a], cb[b], db[b], tb[b])
        out.append((pcs, SW, exact_crossings(pcs, threshold) if pcs else ([], [], [])))
    return out


def assert_transversal(A, B, pairs, threshold, min_speed=1e-3, min_gap=1e-6, exact=None):
    """The fixture's exact crossings are all transversal: every entry and exit at >= min_speed m/s, no touch of the
    threshold, and no pair whose exact infimum over the window lies within min_gap of the threshold."""
    exact = exact_of(A, B, pairs, threshold) if exact is None else exact
    for (a, b), (pcs, (S, W), (_, speeds, touches)) in zip(np.asarray(pairs).reshape(-1, 2), exact):
        if not pcs:
            continue
        D = exact_infimum(pcs, S, W)
        assert not touches, (a, b, touches)
        assert all(s >= min_speed for s in speeds), (a, b, [float(s) for s in speeds])
        assert abs(float(D) - threshold) > min_gap, (a, b, float(D))


def check_windows(ctx, A, B, pairs, threshold, t_res=1e-6, cross=True, closing=True, verdict=None, restated=None,
                  exact=None):
    """The conflict-window entry through `ctx` (a Context or RestatedContext) on `pairs`, A and B as (coef, dur, t0 or
    None), against the exact reference, per pair:
      1. the exact infimum over [S, t_clear_until] and over [t_clear_from, W] is >= threshold - r;
      2. the exact distance at t_first and at t_last is < threshold + r;
      3. eval_flat at t_first / t_last (clamped local times) gives d_first / d_last, within check_contract's tolerance;
      4. closing: t_first - t_clear_until <= t_res + 2 ulp(W), t_clear_from - t_last likewise, and a conflict is found
         exactly when the exact reference has one, within t_res + 2 ulp(W) of the exact first entry and last exit;
      5. S <= t_clear_until <= t_first <= t_last <= t_clear_from <= W where finite.
    cross = False: through pair_conflict_window (A is B, no offsets), with the pair entry's r.  verdict: per pair
    "clear", "conflict" or None (not asserted).  restated: the six arrays of the restatement -- the four times of
    `ctx` lie within t_res + 2 ulp(W) of them.  exact: exact_of of the fixture, when the caller has it.  Returns the
    outputs."""
    (ca, da, t0a), (cb, db, t0b) = A, B
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    if cross:
        out = ctx.cross_conflict_window(ca, da, cb, db, pairs, threshold, t_res, t0_a=t0a, t0_b=t0b)
    else:
        out = ctx.pair_conflict_window(ca, da, pairs, threshold, t_res)
    cu, tf, df, tl, dl, cf, status = out
    assert (status == 0).all(), status
    ta, tb = _t0(t0a, len(da)), _t0(t0b, len(db))
    exact = exact_of(A, B, pairs, threshold) if exact is None else exact
    for k, (a, b) in enumerate(pairs):
        args = (ca[a], da[a], ta[a], cb[b], db[b], tb[b])
        pcs, (S, W), (ranges, speeds, _) = exact[k]
        line = (f"pair ({a}, {b}) window [{float(S)!r}, {float(W)!r}]: clear until {cu[k]!r} first {tf[k]!r} "
                f"({df[k]!r} m) last {tl[k]!r} ({dl[k]!r} m) clear from {cf[k]!r}")
        if not pcs:
            print(line, "disjoint")
            assert (cu[k], tf[k], df[k], tl[k], dl[k], cf[k]) == (np.inf, np.inf, np.inf, -np.inf, np.inf, -np.inf)
            continue
        r = allowance(args, cross)
        tol = t_res + 2 * ulp(W)
        print(line, f"r {r:.3g} exact ranges {[(float(x), float(y)) for x, y in ranges]}")
        # 5. order
        chain = [float(S)] + [x for x in (cu[k], tf[k], tl[k], cf[k]) if np.isfinite(x)] + [float(W)]
        assert all(x <= y for x, y in zip(chain[:-1], chain[1:])), (a, b, chain)
        assert np.isfinite(tf[k]) == np.isfinite(tl[k]) == np.isfinite(df[k]) == np.isfinite(dl[k])
        if np.isfinite(tf[k]):
            assert np.isfinite(cu[k]) and np.isfinite(cf[k])
        # 1. the proven ranges
        # (the proven ranges are half open: in conflict at S, [S, t_clear_until) is empty; likewise at W)
        if not np.isfinite(cu[k]):
            assert float(exact_infimum(pcs, S, W)) >= threshold - r, (a, b, "certified clear")
            assert cf[k] == -np.inf and tf[k] == np.inf and tl[k] == -np.inf
        elif not (cu[k] == tf[k] == float(S)):
            assert float(exact_infimum(pcs, S, Fraction(float(cu[k])))) >= threshold - r, (a, b, "clear until")
        if np.isfinite(cf[k]) and not (cf[k] == tl[k] == float(W)):
            assert float(exact_infimum(pcs, Fraction(float(cf[k])), W)) >= threshold - r, (a, b, "clear from")
        # 2., 3. the conflicts found
        for t, d in ((tf[k], df[k]), (tl[k], dl[k])):
            if not np.isfinite(t):
                continue
            assert float(XE.exact_cross_distance_at(*args, t)) < threshold + r, (a, b, t)
            tau_a = min(max(t - ta[a], 0.0), knots(da[a])[-1])
            tau_b = min(max(t - tb[b], 0.0), knots(db[b])[-1])
            pa = ctx.eval_flat(ca[a:a + 1], da[a:a + 1], np.array([tau_a]))[0, 0, :3]
            pb = ctx.eval_flat(cb[b:b + 1], db[b:b + 1], np.array([tau_b]))[0, 0, :3]
            dd = float(np.linalg.norm(pa - pb))
            assert abs(dd - d) <= 1e-12 * d + ABS_ROUND + XE.C_ROUND_CROSS * EPS * XE.pair_R(*args), (a, b, dd, d)
        # 4. the search closes on a transversal fixture
        if closing:
            assert bool(ranges) == bool(np.isfinite(tf[k])), (a, b, ranges, tf[k])
            if ranges:
                assert tf[k] - cu[k] <= tol and cf[k] - tl[k] <= tol, (a, b, tf[k] - cu[k], cf[k] - tl[k])
                # against the exact entry and exit: an error of r on the distance moves a crossing at `speed` m/s by
                # r / speed to first order (twice that allows for the curvature)
                slack = tol + 2 * r / float(min(speeds)) if speeds else tol
                assert abs(tf[k] - float(ranges[0][0])) <= slack and abs(float(ranges[-1][1]) - tl[k]) <= slack, (a, b)
            else:
                assert cu[k] == np.inf and cf[k] == -np.inf, (a, b, "not certified clear")
        if verdict is not None and verdict[k] == "clear":
            assert cu[k] == np.inf and cf[k] == -np.inf and tf[k] == np.inf and tl[k] == -np.inf, (a, b)
        if verdict is not None and verdict[k] == "conflict":
            assert np.isfinite(tf[k]) and np.isfinite(tl[k]), (a, b)
        if restated is not None:
            for name, got, want in zip(OUTPUTS, out[:6], restated):
                if name.startswith("t_"):
                    assert (got[k] == want[k]) or abs(got[k] - want[k]) <= tol, (a, b, name, got[k], want[k])
    return out
