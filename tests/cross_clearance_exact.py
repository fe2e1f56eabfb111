"""References for the cross clearance (include/msnap.h, "cross clearance"), test side only.

exact_cross_clearance: clearance_exact's pieces on two drones with their own segment counts and start times.  The
coefficients, the fp64 running sums of the durations and the offsets t0 are taken as exact Fractions; a drone's knots on
the common clock are the EXACT sums t0 + running sum.  The window is the header's: S = max of the two t0, W = min of the
two fp64 sums fl(t0 + total).  On every interval between consecutive knots inside the window g = |p_a - p_b|^2 is an
exact rational polynomial; clearance_exact.exact_interval_min gives its minimum at 60 digits.
fp64_cross_clearance, candidate_intervals: clearance_exact's (one NumPy restatement of the kernel serves both entries).
pair_R, pair_Rprime, T_c, contract_violations, the two measured ratios, and RestatedContext: the stand-in through
which tests/test_cross_clearance_cpu.py runs the test bodies of tests/test_cross_clearance_gpu.py on the restatement."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

import clearance_exact as CE
import dyadic_walk as DW
from clearance_exact import DPS, MAX_DEPTH, MAX_NODES, PRUNE_ABS, PRUNE_REL, _mpf, _shift, _t0, exact_interval_min, knots  # noqa: F401
from clearance_exact import cross_candidate_intervals as candidate_intervals, fp64_cross_clearance  # noqa: F401
from dyadic_walk import ABS_CLOSE, ABS_ROUND, EPS, REL_CLOSE, REL_ROUND, _bernstein_weights, _positions, _taylor  # noqa: F401

# include/msnap.h, "cross clearance": r = ABS_ROUND + C_ROUND_CROSS 2^-52 R + C_CLOCK 2^-52 T_c R'.  Ten times the worst
# measured ratio, rounded up (tools/cross_clearance_rounding.py)
C_ROUND_CROSS = 7.0          # worst measured 0.686 (one set against itself at +1e5 m, order 7: K9's own worst case)
C_CLOCK = 1.0                # worst measured 0.0007 (continued paths against the paths they left)


def window(dur_a, t0a, dur_b, t0b):
    """(S, W) of the header as floats: the later start, the earlier of the two fp64 ends fl(t0 + total)."""
    t0a, t0b = float(t0a), float(t0b)
    return max(t0a, t0b), min(t0a + knots(dur_a)[-1], t0b + knots(dur_b)[-1])


def _segment(kn, t):
    """Index of the segment that holds t (first i with t <= kn[i]; the last beyond all)."""
    return next((i for i, x in enumerate(kn) if t <= x), len(kn) - 1)


def exact_cross_clearance(coef_a, dur_a, t0a, coef_b, dur_b, t0b, candidates=None):
    """coef [M, 4, nc], dur [M], t0 of two drones -> (D, t, S, W) as mpf, or None when W < S.  D: the infimum of
    |P_a(t - t0a) - P_b(t - t0b)| over [S, W], t a common-clock time at which it is attained.  `candidates`: start
    times (floats) of the intervals that can hold the infimum -- an exact interval is kept when its start is within
    1e-9 (1 + |t|) of one of them (the fp64 knots differ from the exact ones by an ulp)."""
    S, W = window(dur_a, t0a, dur_b, t0b)
    if W < S:
        return None
    S, W = Fraction(S), Fraction(W)
    ta, tb = Fraction(float(t0a)), Fraction(float(t0b))
    ka = [ta + Fraction(x) for x in knots(dur_a)]
    kb = [tb + Fraction(x) for x in knots(dur_b)]
    sa, sb = [ta] + ka[:-1], [tb] + kb[:-1]
    cuts = sorted({S, W} | {x for x in ka + kb if S < x < W})
    ca = np.asarray(coef_a, dtype=np.float64)
    cb = np.asarray(coef_b, dtype=np.float64)

    def g_at(t0, t1):
        ia, ib = _segment(ka, t1), _segment(kb, t1)
        g = [Fraction(0)]
        for ax in range(3):
            pa = _shift([Fraction(float(x)) for x in ca[ia, ax]], t0 - sa[ia])
            pb = _shift([Fraction(float(x)) for x in cb[ib, ax]], t0 - sb[ib])
            d = [x - y for x, y in zip(pa, pb)]
            sq = [Fraction(0)] * (2 * len(d) - 1)
            for i, x in enumerate(d):
                if x:
                    for j, y in enumerate(d):
                        sq[i + j] += x * y
            g = [(g[i] if i < len(g) else 0) + sq[i] for i in range(len(sq))]
        return g

    with mpmath.workdps(DPS):
        if len(cuts) == 1:                                   # W == S: the one instant
            v = _mpf(g_at(S, S)[0])
            return mpmath.sqrt(v), _mpf(S), _mpf(S), _mpf(W)
        best, bt = None, None
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            if candidates is not None and not any(abs(float(t0) - c) <= 1e-9 * (1 + abs(c)) for c in candidates):
                continue
            v, tau = exact_interval_min(g_at(t0, t1), t0, t1)
            if best is None or v < best:
                best, bt = v, _mpf(t0) + tau
        assert best is not None
        return mpmath.sqrt(max(best, mpmath.mpf(0))), bt, _mpf(S), _mpf(W)


def exact_cross_distance_at(coef_a, dur_a, t0a, coef_b, dur_b, t0b, t):
    """|P_a(t - t0a) - P_b(t - t0b)| as mpf at a common-clock time t (a float or an mpf), local times exact and
    clamped to each path."""
    with mpmath.workdps(DPS):
        t = mpmath.mpf(t)
        pos = []
        for coef, dur, t0 in ((coef_a, dur_a, t0a), (coef_b, dur_b, t0b)):
            k = knots(dur)
            tau = min(max(t - mpmath.mpf(float(t0)), mpmath.mpf(0)), mpmath.mpf(k[-1]))
            i = _segment(k, tau)
            tl = tau - ([0.0] + k)[i]
            pos.append([mpmath.polyval([mpmath.mpf(float(x)) for x in coef[i, ax][::-1]], tl) for ax in range(3)])
        return mpmath.sqrt(sum((x - y) ** 2 for x, y in zip(*pos)))


# ------------------------------------------------------------------------------------------------ the allowance
def _meeting_segments(dur, t0, S, W):
    """The segments of one drone that meet the window [S, W]: closed ranges of the fp64 knots fl(t0 + running sum)."""
    k = [float(t0) + x for x in knots(dur)]
    starts = [float(t0)] + k[:-1]
    return [i for i, (s, e) in enumerate(zip(starts, k)) if s <= W and e >= S]


def _size(coef_a, dur_a, t0a, coef_b, dur_b, t0b, term):
    S, W = window(dur_a, t0a, dur_b, t0b)
    out = 0.0
    for coef, dur, t0 in ((coef_a, dur_a, t0a), (coef_b, dur_b, t0b)):
        coef = np.asarray(coef, dtype=np.float64)
        for i in _meeting_segments(dur, t0, S, W):
            out = max(out, float(term(np.abs(coef[i, :3]), float(dur[i])).sum(axis=1).max()))
    return out


def pair_R(coef_a, dur_a, t0a, coef_b, dur_b, t0b):
    """R of include/msnap.h: the largest sum_k |c_k| T_i^k over x, y, z, both drones and every segment that meets the
    window."""
    return _size(coef_a, dur_a, t0a, coef_b, dur_b, t0b, lambda c, T: c * T ** np.arange(c.shape[1]))


def pair_Rprime(coef_a, dur_a, t0a, coef_b, dur_b, t0b):
    """R' of include/msnap.h: the largest sum_j j |c_j| T_i^(j-1) over the same axes, drones and segments."""
    def term(c, T):
        j = np.arange(1, c.shape[1])
        return c[:, 1:] * j * T ** (j - 1)
    return _size(coef_a, dur_a, t0a, coef_b, dur_b, t0b, term)


def T_c(dur_a, t0a, dur_b, t0b):
    S, W = window(dur_a, t0a, dur_b, t0b)
    return max(abs(S), abs(W))


def allowance(R, Tc, Rp):
    """r of include/msnap.h."""
    return ABS_ROUND + C_ROUND_CROSS * EPS * R + C_CLOCK * EPS * Tc * Rp


def contract_violations(min_dist, lower, D, closed=True, R=0.0, Tc=0.0, Rp=0.0):
    """The inequalities of include/msnap.h that (min_dist, lower) break against the exact D (an mpf): a list of text.
    R = Tc = Rp = 0: the allowance without its coordinate and clock terms, which is stricter."""
    return DW.contract_violations(min_dist, lower, D, closed, C_ROUND_CROSS * R + C_CLOCK * Tc * Rp, 1.0,
                                  lower_le_min_dist=False)


def deviation(min_dist, lower, D, attained=None):
    """What the two terms have to cover [m]: the larger of lower - D, D - min_dist and |min_dist - exact distance at
    t_min|, less the distance-relative part of the allowance (dyadic_walk.round_ratio's numerator)."""
    return DW.round_ratio(min_dist, lower, D, 1.0 / EPS, attained)


# ------------------------------------------------------------------------------------------------ shared test helper
def exact_of(A, B, pairs):
    """Per pair exact_cross_clearance on the candidate intervals.  A, B: (coef, dur, t0 or None)."""
    (ca, da, ta), (cb, db, tb) = A, B
    ta, tb = _t0(ta, len(da)), _t0(tb, len(db))
    cands = candidate_intervals(ca, da, ta, cb, db, tb, pairs)
    return [exact_cross_clearance(ca[a], da[a], ta[a], cb[b], db[b], tb[b], cands[k]) for k, (a, b) in enumerate(pairs)]


def fma_distance(pa, pb):
    """sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) of the header, each operation rounded once (through Fractions)."""
    dx, dy, dz = (Fraction(float(x) - float(y)) for x, y in zip(pa, pb))
    s = Fraction(float(dx * dx))
    s = Fraction(float(dy * dy + s))
    return float(np.sqrt(np.float64(float(dz * dz + s))))


def check_contract(ctx, A, B, pairs, full=False, exact=None, closed=True, attained_bits=False):
    """msnap_cross_clearance through `ctx` (a Context or RestatedContext) on `pairs`, A and B as (coef, dur, t0 or None):
    no status raised, the header's inequalities against exact_cross_clearance, S <= t_min <= W, msnap_eval_flat at the
    clamped local times giving min_dist back.  full: the allowance with its R and clock terms (without them the check
    is stricter: inputs near the origin, t < 20 s).  attained_bits: min_dist is that distance bit for bit (the library;
    the restatement has no fused multiply-add).  Prints per pair and returns (min_dist, t_min, lower, the worst
    deviation / (2^-52 R), the worst deviation / (2^-52 T_c R'))."""
    (ca, da, t0a), (cb, db, t0b) = A, B
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    md, tm, lower, status = ctx.cross_clearance(ca, da, cb, db, pairs, t0_a=t0a, t0_b=t0b)
    assert (status == 0).all(), status
    ta, tb = _t0(t0a, len(da)), _t0(t0b, len(db))
    if exact is None:
        exact = exact_of((ca, da, ta), (cb, db, tb), pairs)
    worst_round = worst_clock = -np.inf
    for k, (a, b) in enumerate(pairs):
        if exact[k] is None:            # the drones never fly at the same time
            print(f"pair ({a}, {b}): disjoint windows")
            assert md[k] == np.inf and lower[k] == np.inf and np.isnan(tm[k]), (a, b)
            continue
        D, _, S, W = exact[k]
        args = (ca[a], da[a], ta[a], cb[b], db[b], tb[b])
        R, Rp, Tc = pair_R(*args), pair_Rprime(*args), T_c(da[a], ta[a], db[b], tb[b])
        dev = deviation(md[k], lower[k], D, exact_cross_distance_at(*args, tm[k]))
        worst_round, worst_clock = max(worst_round, dev / (EPS * R)), max(worst_clock, dev / (EPS * Tc * Rp))
        print(f"pair ({a}, {b}): lower {lower[k]!r} D {float(D)!r} min_dist {md[k]!r} t_min {tm[k]!r} window "
              f"[{float(S)!r}, {float(W)!r}] R {R:.4g} T_c R' {Tc * Rp:.4g} deviation {dev:.3g} m = "
              f"{dev / (EPS * R):.3f} 2^-52 R = {dev / (EPS * Tc * Rp):.5f} 2^-52 T_c R'")
        terms = dict(R=R, Tc=Tc, Rp=Rp) if full else {}
        assert not contract_violations(md[k], lower[k], D, closed=closed, **terms), (a, b)
        assert float(S) <= tm[k] <= float(W)
        # attained: eval_flat of the two drones at the clamped local times gives min_dist back
        tau_a = min(max(tm[k] - ta[a], 0.0), knots(da[a])[-1])
        tau_b = min(max(tm[k] - tb[b], 0.0), knots(db[b])[-1])
        pa = ctx.eval_flat(ca[a:a + 1], da[a:a + 1], np.array([tau_a]))[0, 0, :3]
        pb = ctx.eval_flat(cb[b:b + 1], db[b:b + 1], np.array([tau_b]))[0, 0, :3]
        d = float(np.linalg.norm(pa - pb))
        assert abs(d - md[k]) <= 1e-12 * md[k] + ABS_ROUND + C_ROUND_CROSS * EPS * R, (a, b, d, md[k])
        if attained_bits:
            assert fma_distance(pa, pb) == md[k], (a, b, fma_distance(pa, pb), md[k])
    print(f"worst deviation / (2^-52 R): {worst_round:.3f} (C_ROUND_CROSS {C_ROUND_CROSS}); "
          f"/ (2^-52 T_c R'): {worst_clock:.5f} (C_CLOCK {C_CLOCK})")
    return md, tm, lower, worst_round, worst_clock


class RestatedContext:
    """fp64_cross_clearance, clearance_exact.fp64_clearance and the restated msnap_eval_flat positions behind the
    Context methods the test bodies use: the CPU twins run the same checks on the restatement."""

    def __init__(self, order, max_segments=4096):
        self.order, self.ncoef, self.max_segments = order, order + 1, max_segments
        self._k9 = CE.RestatedContext(order, max_segments)

    def cross_clearance(self, coef_a, dur_a, coef_b, dur_b, pairs, t0_a=None, t0_b=None):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        md, tm, lower = fp64_cross_clearance(coef_a, dur_a, t0_a, coef_b, dur_b, t0_b, pairs)
        return md, tm, lower, np.zeros(len(pairs), dtype=np.int32)

    def pair_clearance(self, coef, dur, pairs):
        return self._k9.pair_clearance(coef, dur, pairs)

    def eval_flat(self, coef, dur, ts):
        return self._k9.eval_flat(coef, dur, ts)
