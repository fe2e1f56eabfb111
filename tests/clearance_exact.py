"""References for the pairwise clearance (include/msnap.h, "pairwise clearance"), test side only.

exact_clearance: the coefficients and the fp64 knot times (running sums, as the library forms them) taken as exact
Fractions; the merged knots with the window's end included; on every interval g = |p_a - p_b|^2 as an exact rational
polynomial in the time since the interval's start, the real roots of g' from mpmath.polyroots at 60 digits, g there and
at both ends; D = sqrt of the minimum.
fp64_cross_clearance: a plain NumPy fp64 restatement of the kernel's lanes and fold (csrc/msnap_clearance.hip),
vectorised over the (pair, interval) lanes, in the kernel's general form: two sets, each with its own segment count and
start times (K14) -- for large lists, for the node counts, and for measuring the rounding of the fp64 method against
the exact references.  Not bit-exact with the kernel (no fused multiply-add here).
fp64_clearance: the same with one set given twice and no start times (K9), as the kernel's CROSS = false instance is."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

import dyadic_walk as DW
# (re-exported: the contract's constants that the mesh clearance shares, and the restatements' common pieces)
from dyadic_walk import ABS_CLOSE, ABS_ROUND, EPS, REL_CLOSE, REL_ROUND, _bernstein_weights, _positions, _taylor  # noqa: F401

DPS = 60
# include/msnap.h, "pairwise clearance": lower <= D (1 + REL_ROUND) + ABS_ROUND + C_ROUND 2^-52 R, the same for
# D <= min_dist, and lower >= min_dist (1 - REL_CLOSE) - ABS_CLOSE when the walk closes
C_ROUND = 8.0           # ten times the worst measured, 0.69 (tools/clearance_rounding.py), rounded up
# csrc/msnap_clearance.hip
MAX_DEPTH = 40
MAX_NODES = 4096
PRUNE_REL = 2e-9
PRUNE_ABS = 1e-18


def knots(dur):
    """fp64 running sums acc = acc + T of one drone's durations (the library's knot times), as floats."""
    out, acc = [], 0.0
    for T in dur:
        acc = acc + float(T)
        out.append(acc)
    return out


def _shift(c, a):
    """Exact Taylor shift: coefficients (ascending) of c(x + a)."""
    c = list(c)
    n = len(c)
    for k in range(n - 1):
        for j in range(n - 2, k - 1, -1):
            c[j] = c[j] + a * c[j + 1]
    return c


def _mpf(x):
    return mpmath.mpf(x.numerator) / x.denominator


def _polyrem(a, b):
    """Remainder of a by b, ascending exact coefficients, b's leading coefficient non-zero."""
    a = list(a)
    while len(a) >= len(b):
        q = a[-1] / b[-1]
        if q:
            for i in range(len(b)):
                a[len(a) - len(b) + i] -= q * b[i]
        a.pop()
        while a and a[-1] == 0:
            a.pop()
    return a


def _squarefree(p):
    """p / gcd(p, p') over the rationals: the same roots, each once (mpmath.polyroots converges slowly, or not at
    all, on the multiple roots that rest-to-rest ends and symmetric paths give g')."""
    d = [(i + 1) * p[i + 1] for i in range(len(p) - 1)]
    while d and d[-1] == 0:
        d.pop()
    a, b = list(p), d
    while b:
        a, b = b, _polyrem(a, b)
    if len(a) <= 1:
        return list(p)
    q, r = [Fraction(0)] * (len(p) - len(a) + 1), list(p)      # exact division p / a
    while len(r) >= len(a):
        c = r[-1] / a[-1]
        q[len(r) - len(a)] = c
        for i in range(len(a)):
            r[len(r) - len(a) + i] -= c * a[i]
        r.pop()
    assert not any(r)
    return q


def exact_interval_min(ga, t0, t1):
    """min over tau in [0, t1 - t0] of the exact polynomial ga (ascending Fractions): (value, tau) as mpf."""
    with mpmath.workdps(DPS):
        h = _mpf(t1 - t0)
        cands = [mpmath.mpf(0), h]
        gp = [(i + 1) * ga[i + 1] for i in range(len(ga) - 1)]
        while gp and gp[-1] == 0:
            gp.pop()
        while gp and gp[0] == 0:                          # roots at tau = 0 (a start from rest): a candidate already
            gp.pop(0)
        if len(gp) >= 2:
            coeffs = [_mpf(x) for x in reversed(gp)]
            try:
                roots = mpmath.polyroots(coeffs, maxsteps=200, extraprec=DPS)
            except mpmath.libmp.NoConvergence:            # multiple roots: the square-free part has the same ones
                coeffs = [_mpf(x) for x in reversed(_squarefree([Fraction(x) for x in gp]))]
                roots = mpmath.polyroots(coeffs, maxsteps=4000, extraprec=20 * DPS) if len(coeffs) >= 2 else []
            for z in roots:
                z = mpmath.mpc(z)
                if abs(z.imag) <= mpmath.mpf(10) ** (-DPS // 2) * (1 + abs(z.real)):
                    cands.append(min(max(z.real, mpmath.mpf(0)), h))
        gm = [_mpf(x) for x in reversed(ga)]
        best, bt = None, None
        for t in cands:
            v = mpmath.polyval(gm, t)
            if best is None or v < best or (v == best and t < bt):
                best, bt = v, t
        return best, bt


def exact_clearance(coef_a, dur_a, coef_b, dur_b, candidates=None):
    """coef [M, 4, nc], dur [M] of two drones -> (D, t, window) as mpf: the infimum of |p_a - p_b| over [0, window],
    window = min of the two totals, and a time at which it is attained.  `candidates`: the start times (floats) of the
    intervals that can hold the infimum (default: all) -- candidate_intervals tells them from the fp64 bounds."""
    ka, kb = knots(dur_a), knots(dur_b)
    W = min(ka[-1], kb[-1])
    cuts = sorted({Fraction(0)} | {Fraction(x) for x in ka + kb if x <= W})
    assert cuts[-1] == Fraction(W)
    starts_a, starts_b = [0.0] + ka[:-1], [0.0] + kb[:-1]
    best, bt = None, None
    with mpmath.workdps(DPS):
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            if candidates is not None and float(t0) not in candidates:
                continue
            ia = next(i for i, x in enumerate(ka) if t1 <= Fraction(x))
            ib = next(i for i, x in enumerate(kb) if t1 <= Fraction(x))
            g = [Fraction(0)]
            for ax in range(3):
                pa = _shift([Fraction(float(x)) for x in coef_a[ia, ax]], t0 - Fraction(starts_a[ia]))
                pb = _shift([Fraction(float(x)) for x in coef_b[ib, ax]], t0 - Fraction(starts_b[ib]))
                d = [x - y for x, y in zip(pa, pb)]
                sq = [Fraction(0)] * (2 * len(d) - 1)
                for i, x in enumerate(d):
                    if x:
                        for j, y in enumerate(d):
                            sq[i + j] += x * y
                g = [(g[i] if i < len(g) else 0) + sq[i] for i in range(len(sq))]
            v, tau = exact_interval_min(g, t0, t1)
            if best is None or v < best:
                best, bt = v, _mpf(t0) + tau
        return mpmath.sqrt(max(best, mpmath.mpf(0))), bt, mpmath.mpf(W)


def exact_distance_at(coef_a, dur_a, coef_b, dur_b, t):
    """|p_a(t) - p_b(t)| as mpf at an absolute time t (a float or an mpf) inside the window."""
    with mpmath.workdps(DPS):
        t = mpmath.mpf(t)
        s = mpmath.mpf(0)
        pos = []
        for coef, dur in ((coef_a, dur_a), (coef_b, dur_b)):
            k = knots(dur)
            i = next((i for i, x in enumerate(k) if t <= x), len(k) - 1)
            tl = t - ([0.0] + k)[i]
            pos.append([mpmath.polyval([mpmath.mpf(float(x)) for x in coef[i, ax][::-1]], tl) for ax in range(3)])
        for x, y in zip(*pos):
            s += (x - y) ** 2
        return mpmath.sqrt(s)


def pair_R(coef_a, dur_a, coef_b, dur_b):
    """R of include/msnap.h: the largest sum_k |c_k| T_i^k over x, y, z, both drones and every segment that meets the
    pair's window (a segment that starts before the window's end; the first one always)."""
    ka, kb = knots(dur_a), knots(dur_b)
    W = min(ka[-1], kb[-1])
    R = 0.0
    for coef, dur, k in ((coef_a, dur_a, ka), (coef_b, dur_b, kb)):
        coef = np.asarray(coef, dtype=np.float64)
        for i, start in enumerate([0.0] + k[:-1]):
            if i == 0 or start < W:
                R = max(R, float((np.abs(coef[i, :3]) * float(dur[i]) ** np.arange(coef.shape[2])).sum(axis=1).max()))
    return R


def round_terms(R):
    """The part of the rounding allowance that does not scale with the distance: ABS_ROUND + C_ROUND 2^-52 R."""
    return DW.round_terms(R, C_ROUND)


def contract_violations(min_dist, lower, D, closed=True, R=0.0):
    """The inequalities of include/msnap.h that (min_dist, lower) break against the exact D (an mpf): a list of text.
    `R`: pair_R of the pair (0: the allowance without its coordinate term, which is stricter)."""
    return DW.contract_violations(min_dist, lower, D, closed, R, C_ROUND, lower_le_min_dist=False)


def round_ratio(min_dist, lower, D, R, attained=None):
    """What C_ROUND has to cover, in units of 2^-52 R: dyadic_walk.round_ratio."""
    return DW.round_ratio(min_dist, lower, D, R, attained)


# ------------------------------------------------------------------------------------------------ fp64 restatement
def _t0(t0, n):
    return np.zeros(n) if t0 is None else np.asarray(t0, dtype=np.float64)


def fp64_cross_clearance(coef_a, dur_a, t0_a, coef_b, dur_b, t0_b, pairs, stats=None):
    """coef_x [Nx, Mx, 4, nc], dur_x [Nx, Mx], t0_x [Nx] or None (zeros), pairs [P, 2] (valid, finite) -> (min_dist [P],
    t_min [P], lower [P]) by the kernel's method in NumPy fp64 (drone a of set A against drone b of set B, include/msnap.h
    "cross clearance").  `stats` (a dict) receives the nodes per live lane ("nodes") and the lanes that met the depth
    cap or the node guard ("capped")."""
    coef_a, coef_b = np.asarray(coef_a, dtype=np.float64), np.asarray(coef_b, dtype=np.float64)
    dur_a, dur_b = np.asarray(dur_a, dtype=np.float64), np.asarray(dur_b, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P, Ma, Mb, nc = len(pairs), dur_a.shape[1], dur_b.shape[1], coef_a.shape[3]
    D, n = nc - 1, 2 * (nc - 1)
    Wt = _bernstein_weights(n)
    a_i, b_i = pairs[:, 0], pairs[:, 1]
    ta, tb = _t0(t0_a, dur_a.shape[0])[a_i], _t0(t0_b, dur_b.shape[0])[b_i]
    LA, LB = np.add.accumulate(dur_a[a_i], axis=1), np.add.accumulate(dur_b[b_i], axis=1)      # local knots
    KA, KB = ta[:, None] + LA, tb[:, None] + LB                                                # on the common clock
    S, Wend = np.maximum(ta, tb), np.minimum(KA[:, -1], KB[:, -1])
    ends = np.concatenate([KA[:, :Ma - 1], KB[:, :Mb - 1], Wend[:, None]], axis=1)             # [P, Ma + Mb - 1]
    ends = np.sort(np.maximum(np.minimum(ends, Wend[:, None]), S[:, None]), axis=1)
    starts = np.concatenate([S[:, None], ends[:, :-1]], axis=1)
    h_all = ends - starts
    live = (h_all > 0) & (Wend >= S)[:, None]
    pi, si = np.nonzero(live)
    E, t0, h = ends[pi, si], starts[pi, si], h_all[pi, si]
    L = len(pi)
    e = np.zeros((L, 3, D + 1))
    for coef, drone, K, Lk, tx, M, sign in ((coef_a, a_i[pi], KA[pi], LA[pi], ta[pi], Ma, 1.0),
                                            (coef_b, b_i[pi], KB[pi], LB[pi], tb[pi], Mb, -1.0)):
        seg = np.minimum((E[:, None] > K).sum(axis=1), M - 1)
        off = np.concatenate([np.zeros((L, 1)), Lk], axis=1)[np.arange(L), seg]
        for ax in range(3):
            e[:, ax, :] += sign * _taylor(coef[drone, seg, ax, :], (t0 - tx) - off)
    e *= (h[:, None] ** np.arange(D + 1))[:, None, :]

    def node(act, a, hh, best, best_u):
        G = np.zeros((len(act), n + 1))
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
        nb, nu = DW.take_attained(((g0, a), (gm, a + 0.5 * hh), (g1, a + hh)), best, best_u)
        return bound, nb, nu, bound < nb - PRUNE_REL * nb - PRUNE_ABS

    best, best_u, low, nodes, capped = DW.walk(L, node, MAX_DEPTH, MAX_NODES)

    tm = np.minimum(h * best_u + t0, E)
    g_pair = np.full(P, np.inf)
    np.minimum.at(g_pair, pi, best)
    t_pair = np.full(P, np.inf)
    winners = best == g_pair[pi]
    np.minimum.at(t_pair, pi[winners], tm[winners])
    t_pair = np.where(np.isfinite(t_pair), t_pair, S)                  # no live slot: Wend == S, the one instant
    low_pair = np.full(P, np.inf)
    np.minimum.at(low_pair, pi, low)
    tau_a = np.minimum(np.maximum(t_pair - ta, 0.0), LA[:, -1])
    tau_b = np.minimum(np.maximum(t_pair - tb, 0.0), LB[:, -1])
    diff = _positions(coef_a, dur_a, a_i, tau_a) - _positions(coef_b, dur_b, b_i, tau_b)
    md = np.sqrt(diff[:, 2] ** 2 + (diff[:, 1] ** 2 + diff[:, 0] ** 2))
    lower = np.minimum(np.sqrt(np.maximum(low_pair, 0.0)), md)
    disjoint = Wend < S
    md, lower, t_pair = np.where(disjoint, np.inf, md), np.where(disjoint, np.inf, lower), np.where(disjoint, np.nan, t_pair)
    if stats is not None:
        stats["lane_pair"], stats["lane_start"], stats["lane_low"], stats["pair_best"] = pi, t0, low, g_pair
        stats["nodes"], stats["capped"], stats["lanes"] = nodes, capped, L
    return md, t_pair, lower


def cross_candidate_intervals(coef_a, dur_a, t0_a, coef_b, dur_b, t0_b, pairs, rel=1e-6):
    """Per pair, the start times of the intervals whose fp64 lower bound of g is within `rel` (on the distance) of the
    pair's smallest attained value: the only ones that can hold the infimum (exact_cross_clearance's `candidates`)."""
    st = {}
    fp64_cross_clearance(coef_a, dur_a, t0_a, coef_b, dur_b, t0_b, pairs, stats=st)
    out = [set() for _ in range(len(pairs))]
    keep = st["lane_low"] <= st["pair_best"][st["lane_pair"]] * (1 + rel) ** 2 + 1e-12
    for p, t0 in zip(st["lane_pair"][keep], st["lane_start"][keep]):
        out[int(p)].add(float(t0))
    return out


def fp64_clearance(coef, dur, pairs, stats=None):
    """The pairwise form: coef [N, M, 4, nc], dur [N, M], pairs [P, 2] (valid, finite) -> (min_dist [P], t_min [P],
    lower [P]): one set against itself on one clock."""
    return fp64_cross_clearance(coef, dur, None, coef, dur, None, pairs, stats)


def candidate_intervals(coef, dur, pairs, rel=1e-6):
    """cross_candidate_intervals of one set against itself on one clock (exact_clearance's `candidates`)."""
    return cross_candidate_intervals(coef, dur, None, coef, dur, None, pairs, rel)


# ------------------------------------------------------------------------------------------------ shared test helper
def check_contract(ctx, coef, dur, pairs, with_R=False, exact=None, closed=True, restated=True, crossing=False):
    """msnap_pair_clearance through `ctx` (a Context) on `pairs`: no status raised, the header's inequalities against
    exact_clearance (on the candidate intervals), t_min inside the window, msnap_eval_flat at t_min giving min_dist
    back.  with_R: the allowance with its coordinate term c 2^-52 R (without it the check is stricter: inputs near the
    origin).  exact: per pair (D, window) known already.  restated: the kernel also within rtol 1e-9 of fp64_clearance.
    Returns (min_dist, t_min, lower, worst round_ratio or None)."""
    pairs = np.asarray(pairs, dtype=np.int32)
    md, tm, lower, status = ctx.pair_clearance(coef, dur, pairs)
    assert (status == 0).all()
    cands = candidate_intervals(coef, dur, pairs) if exact is None else None
    worst = None
    Rs = np.zeros(len(pairs))
    for k, (a, b) in enumerate(pairs):
        if exact is None:
            D, _, W = exact_clearance(coef[a], dur[a], coef[b], dur[b], cands[k])
        else:
            D, W = exact[k]
        R = pair_R(coef[a], dur[a], coef[b], dur[b]) if with_R else 0.0
        Rs[k] = R
        line = f"pair ({a}, {b}): lower {lower[k]!r} D {float(D)!r} min_dist {md[k]!r} t_min {tm[k]!r}"
        if with_R:
            ratio = round_ratio(md[k], lower[k], D, R, exact_distance_at(coef[a], dur[a], coef[b], dur[b], tm[k]))
            worst = ratio if worst is None else max(worst, ratio)
            line += f" R {R:.4g} rounding / (2^-52 R) {ratio:.3f}"
        print(line)
        assert not contract_violations(md[k], lower[k], D, closed=closed, R=R), (a, b)
        assert 0.0 <= tm[k] <= float(W)
        # attained: eval_flat of the two drones at t_min gives min_dist back
        out = ctx.eval_flat(coef[[a, b]], dur[[a, b]], tm[k:k + 1])
        d = float(np.linalg.norm(out[0, 0, :3] - out[1, 0, :3]))
        assert abs(d - md[k]) <= 1e-12 * md[k] + round_terms(R), (a, b, d, md[k])
    if with_R:
        print(f"worst rounding / (2^-52 R): {worst:.3f} (C_ROUND {C_ROUND})")
        assert worst < C_ROUND
    if restated:
        # test_large_list_against_the_fp64_restatement's tolerances, with the coordinate term on min_dist where the
        # allowance has it.  crossing: D is (next to) zero, so both walks stop inside the absolute closing slack A and
        # their attained values are any two numbers in [D, D + A] -- there, and only there, min_dist gets A as well.
        rmd, rtm, rlower = fp64_clearance(coef, dur, pairs)
        print("kernel - restatement: min_dist", np.abs(md - rmd).max(), "lower", np.abs(lower - rlower).max())
        slack = ABS_CLOSE if crossing else 0.0
        assert (np.abs(md - rmd) <= 1e-9 * np.abs(rmd) + ABS_ROUND + C_ROUND * EPS * Rs + slack).all(), (md, rmd)
        assert (np.abs(lower - rlower) <= 1e-9 * np.abs(rlower) + ABS_CLOSE).all(), (lower, rlower)
    return md, tm, lower, worst


class RestatedContext:
    """fp64_clearance and the restated msnap_eval_flat positions behind Context's two methods that check_contract
    uses: the CPU twins of the GPU tests run the same checks on the restatement.  (eval_flat here is the routine
    fp64_clearance forms min_dist with, so the twins' "eval_flat at t_min gives min_dist back" holds by construction;
    that check says something only on the GPU, where msnap_eval_flat is a kernel of its own.)"""

    def __init__(self, order, max_segments=4096):
        self.order, self.ncoef, self.max_segments = order, order + 1, max_segments

    def pair_clearance(self, coef, dur, pairs):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        md, tm, lower = fp64_clearance(coef, dur, pairs)
        return md, tm, lower, np.zeros(len(pairs), dtype=np.int32)

    def eval_flat(self, coef, dur, ts):
        coef, dur, ts = np.asarray(coef, dtype=np.float64), np.asarray(dur, dtype=np.float64), np.asarray(ts, dtype=np.float64)
        out = np.zeros((coef.shape[0], len(ts), 13))
        for d in range(coef.shape[0]):
            out[d, :, :3] = _positions(coef, dur, np.full(len(ts), d), ts)
        return out
