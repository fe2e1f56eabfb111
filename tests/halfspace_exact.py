"""References for the half-space windows (include/msnap.h, "half-space windows"), test side only.

Exact.  `pieces` gives, per segment of one drone clipped to the query's range [S, W] (the coefficients, the fp64 running
sums of the durations and the plane taken as exact Fractions), p = n.p - b as an exact rational polynomial in the time
since the piece's start.  From those:
  exact_supremum     the supremum of n.p - b over any sub-range of [S, W] (clearance_exact's exact_interval_min);
  exact_outside      the real roots of p (conflict_exact._real_roots: mpmath.polyroots at 60 digits), the maximal open
                     ranges on which the path is outside, hence the exact first exit and last re-entry, the crossing
                     speed |d/dt n.p| at every one of them, and the touches;
  the exact value at a time is extent_exact.exact_value_at.
fp64_halfspace_window: a plain NumPy fp64 restatement of the lane and fold rules of csrc/msnap_halfspace.hip, vectorised
over the (query, segment) lanes.  Not bit-exact with the kernel (no fused multiply-add here).
check_windows: the per-query checks against the exact reference, shared by the CPU and the GPU tests.

Rounding (tools/halfspace_window_rounding.py, on the restatement, t_res = 1e-14, both orders, offsets up to 1e5 m): the
worst deviation of a proven range or of a time found outside is WORST_MEASURED in units of 2^-52 R_k.  Ten times that is
below extent_exact.C_ROUND_EXTENT = 9, so the entry keeps K12's allowance r = 1e-13 + 9 2^-52 R_k unchanged."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

import extent_exact as XE
from clearance_exact import DPS, MAX_DEPTH, MAX_NODES, _mpf, _shift, exact_interval_min, knots
from conflict_exact import _real_roots, ulp
from dyadic_walk import EPS, _bernstein_weights, _positions, _taylor, trailing_ones
from extent_exact import unfused_dot

OUTPUTS = ("t_inside_until", "t_first", "v_first", "t_last", "v_last", "t_inside_from")
WORST_MEASURED = 0.697         # order 9, 5 drones x 3 segments at +1e5 m
C_ROUND_HALFSPACE = XE.C_ROUND_EXTENT      # K12's constant, unchanged: 10 WORST_MEASURED < 9


def allowance(coef_d, dur_d, n):
    """r of include/msnap.h for one drone and one normal: msnap_path_extent's, 1e-13 + 9 2^-52 R_k."""
    return XE.ABS_ROUND + C_ROUND_HALFSPACE * EPS * XE.extent_R(coef_d, dur_d, n)


def query_range(dur_d, t_from=None, t_to=None):
    """[S, W] of a query as the kernel forms it (floats)."""
    total = knots(dur_d)[-1]
    return max(0.0 if t_from is None else float(t_from), 0.0), min(total if t_to is None else float(t_to), total)


# ------------------------------------------------------------------------------------------------ exact
def pieces(coef_d, dur_d, plane, S, W):
    """[(t0, t1, p)] over [S, W]: t0 < t1 Fractions, p = n.p - b ascending Fractions in (t - t0), one per segment that
    meets the range; for W == S one piece (S, S, p) of the segment msnap_eval_flat's lookup selects; [] for W < S."""
    if W < S:
        return []
    S, W = Fraction(float(S)), Fraction(float(W))
    k = [Fraction(x) for x in knots(dur_d)]
    starts = [Fraction(0)] + k[:-1]
    coef_d = np.asarray(coef_d, dtype=np.float64)
    b = Fraction(float(plane[3]))

    def p_at(i, t0):
        q = _shift(XE._scalar(coef_d, i, plane[:3]), t0 - starts[i])
        return [q[0] - b] + list(q[1:])

    if W == S:
        i = next((i for i, x in enumerate(k) if S <= x), len(k) - 1)
        return [(S, S, p_at(i, S))]
    out = []
    for i in range(len(k)):
        t0, t1 = max(S, starts[i]), min(W, k[i])
        if t1 > t0:
            out.append((t0, t1, p_at(i, t0)))
    return out


def exact_supremum(pcs, lo, hi):
    """The supremum of n.p - b over [lo, hi] (floats or Fractions inside the range) as mpf; -inf for an empty range."""
    lo, hi = Fraction(lo), Fraction(hi)
    best = None
    with mpmath.workdps(DPS):
        for t0, t1, p in pcs:
            a, c = max(t0, lo), min(t1, hi)
            if a > c:
                continue
            q = _shift(p, a - t0)
            v = -exact_interval_min([-x for x in q], a, c)[0] if c > a else _mpf(q[0])
            best = v if best is None or v > best else best
        return -mpmath.inf if best is None else best


def exact_outside(pcs):
    """The ranges on which the exact n.p is > b: (ranges, speeds, touches).  ranges: [(t_out, t_in)] as mpf, maximal, in
    time order (a range that starts at S or ends at W is closed there by the query's range); speeds: |d/dt n.p| at every
    end of a range that is a root; touches: the roots at which n.p only touches b from below."""
    raw, speeds, touches = [], [], []
    with mpmath.workdps(DPS):
        for t0, t1, p in pcs:
            pm = [_mpf(x) for x in reversed(p)]
            dm = [_mpf((i + 1) * p[i + 1]) for i in range(len(p) - 1)][::-1]
            if t1 == t0:
                if p[0] > 0:
                    raw.append((_mpf(t0), _mpf(t0)))
                continue
            h = _mpf(t1 - t0)
            c = [mpmath.mpf(0)] + [r for r in _real_roots(p, h) if 0 < r < h] + [h]
            out = [mpmath.polyval(pm, (x + y) / 2) > 0 for x, y in zip(c[:-1], c[1:])]
            for k, (x, y) in enumerate(zip(c[:-1], c[1:])):
                if out[k]:
                    raw.append((_mpf(t0) + x, _mpf(t0) + y))
                    for r in ((x,) if k > 0 else ()) + ((y,) if k < len(out) - 1 else ()):
                        speeds.append(abs(mpmath.polyval(dm, r)) if dm else mpmath.mpf(0))
            for k in range(1, len(c) - 1):
                if not out[k - 1] and not out[k]:
                    touches.append(_mpf(t0) + c[k])
        ranges = []
        for a, c in raw:          # ranges that continue across a knot are one
            if ranges and ranges[-1][1] == a:
                ranges[-1] = (ranges[-1][0], c)
            else:
                ranges.append((a, c))
    return ranges, speeds, touches


# ------------------------------------------------------------------------------------------------ fp64 restatement
def _first_crossing(e, h, L, t_res, Wt):
    """csrc/msnap_walk.h, first_crossing, on the scalar lanes e [n, D + 1] of lengths h [n] against the levels L [n]:
    (hit_u, clear_u, nodes)."""
    n, D = len(h), e.shape[1] - 1
    hit, clear = np.full(n, np.inf), np.full(n, np.inf)
    idx, lvl, nodes = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    act = np.arange(n)
    while len(act):
        hh = np.ldexp(1.0, -lvl[act])
        a = idx[act].astype(np.float64) * hh
        f = _taylor(e[act], a) * hh[:, None] ** np.arange(D + 1)
        gm, g1 = np.zeros(len(act)), np.zeros(len(act))
        for j in range(D, -1, -1):
            gm = gm * 0.5 + f[:, j]
            g1 = g1 + f[:, j]
        g0 = f[:, 0]
        bound = (f @ Wt.T).min(axis=1)
        Ln = L[act]
        open_ = ~(bound >= Ln)
        at_start = open_ & (g0 < Ln)
        leaf = (h[act] * hh <= t_res) | (lvl[act] >= MAX_DEPTH)
        in_mid, at_end = gm < Ln, g1 < Ln
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


def fp64_halfspace_window(coef, dur, planes, queries, t_res=1e-6, t_from=None, t_to=None, stats=None):
    """coef [N, M, 4, nc], dur [N, M] (finite, durations > 0), planes [K, 4], queries [Q, 2] (in range), t_from / t_to
    [Q] (finite) or None -> the six arrays of OUTPUTS, by the kernel's method in NumPy fp64.  `stats` receives the nodes
    per live lane and direction ("nodes" [L, 2]), the lane count ("lanes") and the lanes' queries ("lane_query")."""
    coef, dur, planes = (np.asarray(x, dtype=np.float64) for x in (coef, dur, planes))
    planes = planes.reshape(-1, 4)
    queries = np.asarray(queries, dtype=np.int64).reshape(-1, 2)
    Q, M, D = len(queries), dur.shape[1], coef.shape[3] - 1
    Wt = _bernstein_weights(D)
    d_i, p_i = queries[:, 0], queries[:, 1]
    ends = np.add.accumulate(dur, axis=1)
    starts = np.concatenate([np.zeros((dur.shape[0], 1)), ends[:, :-1]], axis=1)
    total = ends[d_i, -1] if Q else np.zeros(0)
    S = np.maximum(np.zeros(Q) if t_from is None else np.asarray(t_from, dtype=np.float64), 0.0)
    W = np.minimum(total if t_to is None else np.asarray(t_to, dtype=np.float64), total)
    n, b = planes[p_i, :3], planes[p_i, 3]
    plane_ok = np.isfinite(planes[p_i]).all(axis=1)
    st, E = starts[d_i], starts[d_i] + dur[d_i]                                     # [Q, M]
    lo_all, hi_all = np.maximum(S[:, None], st), np.minimum(W[:, None], E)
    h_all = hi_all - lo_all
    qi, si = np.nonzero((h_all > 0) & plane_ok[:, None])
    lo, hi, h = lo_all[qi, si], hi_all[qi, si], h_all[qi, si]
    Ln = len(qi)
    c, nn = coef[d_i[qi], si, :3, :], n[qi]
    q = nn[:, 2:3] * c[:, 2, :] + (nn[:, 1:2] * c[:, 1, :] + nn[:, 0:1] * c[:, 0, :])
    e = -(_taylor(q, lo - st[qi, si]) * h[:, None] ** np.arange(D + 1))
    L = -b[qi]
    hit_f, clear_f, nodes_f = _first_crossing(e, h, L, t_res, Wt)
    back = _taylor(e, np.ones(Ln))                                                  # m(1 - u)
    back[:, 1::2] *= -1.0
    hit_b, clear_b, nodes_b = _first_crossing(back, h, L, t_res, Wt)
    fwd = lambda u: np.where(np.isfinite(u), np.minimum(h * np.where(np.isfinite(u), u, 0.0) + lo, hi), np.inf)      # noqa: E731
    bwd = lambda u: np.where(np.isfinite(u), np.maximum(hi - h * np.where(np.isfinite(u), u, 0.0), lo), -np.inf)     # noqa: E731

    tf, iu, tl, ifr = np.full(Q, np.inf), np.full(Q, np.inf), np.full(Q, -np.inf), np.full(Q, -np.inf)
    np.minimum.at(tf, qi, fwd(hit_f))
    np.minimum.at(iu, qi, fwd(clear_f))
    np.maximum.at(tl, qi, bwd(hit_b))
    np.maximum.at(ifr, qi, bwd(clear_b))
    first = np.minimum(tf, np.where(tl > -np.inf, tl, np.inf))
    last = np.maximum(tl, np.where(tf < np.inf, tf, -np.inf))
    tf, tl = first, last
    iu, ifr = np.minimum(iu, tf), np.maximum(ifr, tl)
    instant = W == S
    tf, tl = np.where(instant, S, tf), np.where(instant, S, tl)

    def value(t):
        return unfused_dot(n, _positions(coef, dur, d_i, np.where(np.isfinite(t), t, S))) if Q else np.zeros(0)

    found = np.isfinite(tf)
    vf, vl = np.where(found, value(tf), -np.inf), np.where(found, value(tl), -np.inf)
    out_instant = instant & (vf > b)
    iu, ifr = np.where(out_instant, S, iu), np.where(out_instant, S, ifr)
    none = (instant & ~out_instant) | (W < S)
    iu, tf = np.where(none, np.inf, iu), np.where(none, np.inf, tf)
    vf, vl, tl, ifr = (np.where(none, -np.inf, x) for x in (vf, vl, tl, ifr))
    outs = tuple(np.where(plane_ok, x, np.nan) for x in (iu, tf, vf, tl, vl, ifr))
    if stats is not None:
        stats["nodes"], stats["lanes"], stats["lane_query"] = np.stack([nodes_f, nodes_b], axis=1), Ln, qi
    return outs


class RestatedContext(XE.CE.RestatedContext):
    """fp64_halfspace_window behind Context.halfspace_window, beside clearance_exact's restated eval_flat: the CPU tests
    run the GPU tests' checks on the restatement."""

    def halfspace_window(self, coef, dur, planes, queries, t_res=1e-6, t_from=None, t_to=None):
        queries = np.asarray(queries, dtype=np.int64).reshape(-1, 2)
        out = fp64_halfspace_window(coef, dur, planes, queries, t_res, t_from, t_to)
        return out + (np.zeros(len(queries), dtype=np.int32),)


class RestatedCompute:
    """DeviceCompute's halfspace_window, path_extent and eval_state on CPU tensors through the restatements: what
    swarm.geofence_windows and swarm.certify_corridor need of their compute object."""

    def halfspace_window(self, coef, dur, planes, queries, t_res=1e-6, t_from=None, t_to=None):
        import torch
        n = lambda x: None if x is None else x.numpy()      # noqa: E731
        out = fp64_halfspace_window(n(coef), n(dur), n(planes), n(queries), t_res, n(t_from), n(t_to))
        return tuple(torch.from_numpy(x) for x in out + (np.zeros(len(out[0]), dtype=np.int32),))

    def path_extent(self, coef, dur, dirs):
        import torch
        return tuple(torch.from_numpy(x) for x in XE.restated(coef.numpy(), dur.numpy(), dirs.numpy()))

    def eval_state(self, coef, dur, tq):
        import torch
        pos = np.zeros((len(tq), 4))
        pos[:, :3] = _positions(coef.numpy(), dur.numpy(), np.arange(len(tq)), tq.numpy())
        return torch.from_numpy(pos), None


# ------------------------------------------------------------------------------------------------ shared test helper
def exact_of(coef, dur, planes, queries, t_from=None, t_to=None):
    """Per query (pieces, (S, W), exact_outside) -- computed once per fixture and shared by the tests that need it."""
    out = []
    for k, (d, p) in enumerate(np.asarray(queries).reshape(-1, 2)):
        S, W = query_range(dur[d], None if t_from is None else t_from[k], None if t_to is None else t_to[k])
        pcs = pieces(coef[d], dur[d], planes[p], S, W)
        out.append((pcs, (S, W), exact_outside(pcs) if pcs else ([], [], [])))
    return out


def assert_transversal(exact, min_speed=1e-3, min_gap=1e-6):
    """The fixture's exact crossings are all transversal: every exit and re-entry at >= min_speed (units of n.p per
    second), no touch of the limit, and no query whose exact supremum of n.p - b over its range lies within min_gap of 0."""
    for k, (pcs, (S, W), (_, speeds, touches)) in enumerate(exact):
        if not pcs:
            continue
        assert not touches, (k, touches)
        assert all(s >= min_speed for s in speeds), (k, [float(s) for s in speeds])
        assert abs(float(exact_supremum(pcs, S, W))) > min_gap, (k, float(exact_supremum(pcs, S, W)))


def check_windows(ctx, coef, dur, planes, queries, t_res=1e-6, t_from=None, t_to=None, closing=True, verdict=None,
                  restated=None, exact=None, bitwise=True):
    """The half-space window entry through `ctx` (a Context or RestatedContext) against the exact reference, per query,
    with r = msnap_path_extent's allowance for (drone, n):
      1. the exact supremum of n.p over [S, t_inside_until] and over [t_inside_from, W] is <= b + r;
      2. the exact n.p at t_first and at t_last is > b - r;
      3. eval_flat at t_first / t_last and the unfused dot product give v_first / v_last (bitwise: bit for bit);
      4. closing: t_first - t_inside_until <= t_res + 2 ulp(W), t_inside_from - t_last likewise, and something is found
         outside exactly when the exact reference has a range, within t_res + 2 ulp(W) + 2 r / speed of the exact first
         exit and last re-entry;
      5. S <= t_inside_until <= t_first <= t_last <= t_inside_from <= W where finite.
    verdict: per query "inside", "outside" or None (not asserted).  restated: the six arrays of the restatement -- the
    four times of `ctx` lie within t_res + 2 ulp(W) of them.  exact: exact_of of the fixture.  Returns the outputs."""
    coef, dur, planes = (np.asarray(x, dtype=np.float64) for x in (coef, dur, planes))
    queries = np.asarray(queries, dtype=np.int32).reshape(-1, 2)
    out = ctx.halfspace_window(coef, dur, planes, queries, t_res, t_from=t_from, t_to=t_to)
    iu, tf, vf, tl, vl, ifr, status = out
    assert (status == 0).all(), status
    exact = exact_of(coef, dur, planes, queries, t_from, t_to) if exact is None else exact
    for k, (d, p) in enumerate(queries):
        n, b = planes[p, :3], planes[p, 3]
        pcs, (S, W), (ranges, speeds, _) = exact[k]
        line = (f"query ({d}, {p}) range [{S!r}, {W!r}]: inside until {iu[k]!r} first {tf[k]!r} ({vf[k]!r}) last "
                f"{tl[k]!r} ({vl[k]!r}) inside from {ifr[k]!r}")
        if not pcs:
            print(line, "empty range")
            assert (iu[k], tf[k], vf[k], tl[k], vl[k], ifr[k]) == (np.inf, np.inf, -np.inf, -np.inf, -np.inf, -np.inf)
            continue
        r = allowance(coef[d], dur[d], n)
        tol = t_res + 2 * ulp(W)
        print(line, f"r {r:.3g} exact ranges {[(float(x), float(y)) for x, y in ranges]}")
        # 5. order
        chain = [S] + [x for x in (iu[k], tf[k], tl[k], ifr[k]) if np.isfinite(x)] + [W]
        assert all(x <= y for x, y in zip(chain[:-1], chain[1:])), (d, p, chain)
        assert np.isfinite(tf[k]) == np.isfinite(tl[k]) == np.isfinite(vf[k]) == np.isfinite(vl[k])
        if np.isfinite(tf[k]):
            assert np.isfinite(iu[k]) and np.isfinite(ifr[k])
        # 1. the proven ranges (half open: outside at S, [S, t_inside_until) is empty; likewise at W)
        if not np.isfinite(iu[k]):
            assert float(exact_supremum(pcs, S, W)) <= r, (d, p, "certified inside")
            assert ifr[k] == -np.inf and tf[k] == np.inf and tl[k] == -np.inf
        elif not (iu[k] == tf[k] == S):
            assert float(exact_supremum(pcs, S, float(iu[k]))) <= r, (d, p, "inside until")
        if np.isfinite(ifr[k]) and not (ifr[k] == tl[k] == W):
            assert float(exact_supremum(pcs, float(ifr[k]), W)) <= r, (d, p, "inside from")
        # 2., 3. the times found outside
        for t, v in ((tf[k], vf[k]), (tl[k], vl[k])):
            if not np.isfinite(t):
                continue
            assert float(XE.exact_value_at(coef[d], dur[d], n, t)) - b > -r, (d, p, t)
            pos = ctx.eval_flat(coef[d:d + 1], dur[d:d + 1], np.array([t]))[0, 0, :3]
            vv = float(unfused_dot(n, pos))
            assert (vv == v) if bitwise else abs(vv - v) <= r, (d, p, vv, v)
        # 4. the search closes on a transversal fixture
        if closing:
            assert bool(ranges) == bool(np.isfinite(tf[k])), (d, p, ranges, tf[k])
            if ranges:
                assert tf[k] - iu[k] <= tol and ifr[k] - tl[k] <= tol, (d, p, tf[k] - iu[k], ifr[k] - tl[k])
                slack = tol + 2 * r / float(min(speeds)) if speeds else tol
                assert abs(tf[k] - float(ranges[0][0])) <= slack and abs(float(ranges[-1][1]) - tl[k]) <= slack, (d, p)
            else:
                assert iu[k] == np.inf and ifr[k] == -np.inf, (d, p, "not certified inside")
        if verdict is not None and verdict[k] == "inside":
            assert iu[k] == np.inf and ifr[k] == -np.inf and tf[k] == np.inf and tl[k] == -np.inf, (d, p)
        if verdict is not None and verdict[k] == "outside":
            assert np.isfinite(tf[k]) and np.isfinite(tl[k]), (d, p)
        if restated is not None:
            for name, got, want in zip(OUTPUTS, out[:6], restated):
                if name.startswith("t_"):
                    assert (got[k] == want[k]) or abs(got[k] - want[k]) <= tol, (d, p, name, got[k], want[k])
    return out
