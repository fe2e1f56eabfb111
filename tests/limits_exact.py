"""References for the dynamic-limit peaks (include/msnap.h, "dynamic limits"), test side only.

exact_peaks: the coefficients taken as exact Fractions, g = |p^(r)|^2 and g' formed exactly, the real roots of g' in
[0, T] from mpmath.polyroots at 50 digits, g evaluated there and at both ends; max, then sqrt.
fp64_peaks: a vectorised fp64 reference for large batches -- the roots of g' as eigenvalues of its companion matrix
(what numpy.roots does, batched), polished by Newton steps, g at those and at the ends.
fp64_walk_peaks: the kernel's own method restated in NumPy fp64 (csrc/msnap_limits.hip on tests/dyadic_walk.walk), the
counterpart of clearance_exact.fp64_clearance: what the rounding of the method is measured on without a GPU
(tools/limits_rounding.py), and what tools/limits_nodes.py counts nodes with.
peaks_R, in_contract, exact_value_at: the contract's coordinate term r_q = C_ROUND_PEAKS 2^-52 R_q; peaks_R1, time_term:
the term of the value at t_peak for the rounding of t_peak itself."""
from __future__ import annotations

import os
import sys
from fractions import Fraction
from typing import NamedTuple

import mpmath
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyadic_walk as DW  # noqa: E402
from dyadic_walk import EPS, _bernstein_weights, _taylor  # noqa: E402

DPS = 50
# csrc/msnap_limits.hip, csrc/msnap_walk.h
PRUNE_REL, PRUNE_ABS, MAX_DEPTH, MAX_NODES = 1e-9, 1e-26, 40, 4096
# include/msnap.h, "dynamic limits": r_q = C_ROUND_PEAKS 2^-52 R_q, the rounding of the Horner that recomputes the peak.
# Ten times the worst |peak - exact value at the lane's own local time T u| / (2^-52 R_q) that tools/limits_rounding.py
# prints over its families (1.637, on the mixed batch of 67 x 3 at order 9), rounded up -- the rule of clearance_exact.C_ROUND and
# mesh_clearance_exact.C_ROUND.  The rounding of t_peak = acc + T u is NOT in it: the header gives that its own, proven
# term (time_term below), which grows with the absolute time where r_q does not.  DESIGN.md §5 K7.
C_ROUND_PEAKS = 17
ORDERS = ((1, (0, 1, 2)), (2, (0, 1, 2)), (3, (0, 1, 2)), (1, (3,)))   # quantity q: (derivative, axes)


def _deriv(c, r):
    """Exact coefficients (ascending) of the r-th derivative."""
    c = list(c)
    for _ in range(r):
        c = [(i + 1) * c[i + 1] for i in range(len(c) - 1)]
    return c


def _mul(a, b):
    out = [Fraction(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return out


def _add(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0) for i in range(n)]


def exact_segment_max(polys, T):
    """max over t in [0, T] of sum_k h_k(t)^2, h_k given by exact ascending coefficients: (sqrt of it, t) as mpf."""
    g = [Fraction(0)]
    for h in polys:
        g = _add(g, _mul(h, h))
    gp = [(i + 1) * g[i + 1] for i in range(len(g) - 1)]
    while gp and gp[-1] == 0:
        gp.pop()
    T = Fraction(T)
    cands = [mpmath.mpf(0), mpmath.mpf(T.numerator) / T.denominator]
    with mpmath.workdps(DPS):
        if len(gp) >= 2:
            coeffs = [mpmath.mpf(x.numerator) / x.denominator for x in reversed(gp)]
            try:
                roots = mpmath.polyroots(coeffs, maxsteps=200, extraprec=2 * DPS)
            except mpmath.libmp.NoConvergence:        # (clustered roots: more steps and digits)
                roots = mpmath.polyroots(coeffs, maxsteps=4000, extraprec=20 * DPS)
            Tm = cands[1]
            for z in roots:
                z = mpmath.mpc(z)
                if abs(z.imag) <= mpmath.mpf(10) ** (-DPS // 2) * (1 + abs(z.real)):
                    cands.append(min(max(z.real, mpmath.mpf(0)), Tm))      # (a real point of the range: attained)
        gm = [mpmath.mpf(x.numerator) / x.denominator for x in g]
        best, bt = mpmath.mpf(-1), mpmath.mpf(0)
        for t in cands:
            v = mpmath.polyval(list(reversed(gm)), t)
            if v > best:
                best, bt = v, t
        return mpmath.sqrt(max(best, mpmath.mpf(0))), bt


def exact_peaks(coef, dur, candidates=None):
    """coef [M, 4, nc], dur [M] of one drone -> (peaks [4] as mpf, their absolute times [4] as mpf).
    `candidates[q]`: the segments that can hold quantity q's supremum (default: all) -- e.g. those whose fp64 maximum
    is within a percent of the drone's, which fp64_peaks tells far more precisely than that."""
    M = len(dur)
    peaks = [mpmath.mpf(-1)] * 4
    times = [mpmath.mpf(0)] * 4
    acc = mpmath.mpf(0)
    with mpmath.workdps(DPS):
        for i in range(M):
            fr = [[Fraction(float(x)) for x in coef[i, a]] for a in range(4)]
            for q, (r, axes) in enumerate(ORDERS):
                if candidates is not None and i not in candidates[q]:
                    continue
                v, t = exact_segment_max([_deriv(fr[a], r) for a in axes], float(dur[i]))
                if v > peaks[q]:
                    peaks[q], times[q] = v, acc + t
            acc += mpmath.mpf(float(dur[i]))
    return peaks, times


def round_term(R):
    """r_q of include/msnap.h: C_ROUND_PEAKS 2^-52 R_q."""
    return C_ROUND_PEAKS * EPS * R


def in_contract(peak, S, R=0.0):
    """include/msnap.h: S (1 - 1e-9) - 1e-12 - r <= peak <= S (1 + 1e-12) + 1e-12 + r, r = C_ROUND_PEAKS 2^-52 R
    (peak a float, S an mpf).  R: the quantity's peaks_R (0: the allowance without its coordinate term, which is
    stricter -- what held before the term was stated, and still does for paths whose coefficients do not cancel)."""
    S = float(S)
    r = round_term(R)
    return S * (1 - 1e-9) - 1e-12 - r <= peak <= S * (1 + 1e-12) + 1e-12 + r


def _deriv_fp64(c, r):
    """derivative()'s operation order in fp64: (i + 1) * previous[i + 1], one rounding each; [..., n] -> [..., n - r]."""
    c = np.asarray(c, dtype=np.float64)
    for _ in range(r):
        c = np.arange(1, c.shape[-1], dtype=np.float64) * c[..., 1:]
    return c


def peaks_R(coef_d, dur_d):
    """R_q of include/msnap.h for one drone (coef_d [M, 4, nc], dur_d [M]) -> [4]: the largest value, over the
    quantity's axes and the drone's segments i, of sum_j |d_j| T_i^j, d the t-domain coefficients of the r-th
    derivative of that axis -- the size of what the attained value is summed from."""
    coef_d = np.asarray(coef_d, dtype=np.float64)
    dur_d = np.asarray(dur_d, dtype=np.float64)
    out = np.zeros(4)
    for q, (r, axes) in enumerate(ORDERS):
        d = np.abs(_deriv_fp64(coef_d[:, list(axes), :], r))                      # [M, A, nc - r]
        out[q] = float((d * dur_d[:, None, None] ** np.arange(d.shape[-1])).sum(axis=-1).max())
    return out


def peaks_R1(coef_d, dur_d):
    """R'_q of include/msnap.h for one drone -> [4]: the largest value, over the quantity's axes and the drone's
    segments i, of sum_j j |d_j| T_i^(j-1) -- the size of the NEXT derivative, what a change of the time moves the
    value by."""
    coef_d = np.asarray(coef_d, dtype=np.float64)
    dur_d = np.asarray(dur_d, dtype=np.float64)
    out = np.zeros(4)
    for q, (r, axes) in enumerate(ORDERS):
        d = np.abs(_deriv_fp64(coef_d[:, list(axes), :], r))[..., 1:]              # [M, A, nc - r - 1]
        j = np.arange(1, d.shape[-1] + 1)
        out[q] = float((d * j * dur_d[:, None, None] ** (j - 1)).sum(axis=-1).max())
    return out


def time_term(t_peak, R1):
    """include/msnap.h: 2^-52 t_peak R'_q, what the rounding of t_peak = acc + T u to fp64 can move the exact value at
    t_peak by.  Proven, not measured: the sum is rounded by at most ulp(t_peak) / 2 <= 2^-53 t_peak, each axis's
    derivative changes by at most that times sum_j j |d_j| T^(j-1), and the norm of up to three axes by at most
    sqrt(3) times the largest of them; sqrt(3) / 2 < 1."""
    return EPS * t_peak * R1


def lookup_segment(dur_d, t):
    """msnap_eval_flat's lookup on its running fp64 sums: (the first segment i with t <= acc_i + T_i, acc_i)."""
    acc = 0.0
    for i, T in enumerate(dur_d):
        if t <= acc + float(T):
            return i, acc
        acc = acc + float(T)
    raise ValueError(f"t = {t!r} is beyond the path's end {acc!r}")


def exact_value_local(coef_d, i, q, tl):
    """|p^(r)(tl)| of quantity q as mpf at the local time tl (a float or an mpf) of segment i."""
    with mpmath.workdps(DPS):
        tl = mpmath.mpf(tl)
        r, axes = ORDERS[q]
        s = mpmath.mpf(0)
        for a in axes:
            d = _deriv([Fraction(float(x)) for x in coef_d[i, a]], r)
            s += mpmath.polyval([mpmath.mpf(x.numerator) / x.denominator for x in reversed(d)], tl) ** 2
        return mpmath.sqrt(s)


def exact_value_at(coef_d, dur_d, q, t, later=False):
    """|p^(r)(t)| of quantity q as mpf at the absolute time t (a float), on the segment msnap_eval_flat's lookup
    selects.  later: if t is that segment's end and another one follows, on the one that starts there (local time 0)
    -- the two differ where the coefficients jump at the knot."""
    i, acc = lookup_segment(dur_d, t)
    with mpmath.workdps(DPS):
        tl = mpmath.mpf(t) - mpmath.mpf(acc)
        if later and t == acc + float(dur_d[i]) and i + 1 < len(dur_d):
            i, tl = i + 1, mpmath.mpf(0)
        return exact_value_local(coef_d, i, q, tl)


# ------------------------------------------------------------------------------------------------ fp64 restatement
def lane_polynomials(coef, dur):
    """coef [N, M, 4, nc], dur [N, M] -> (d [L, 3, nc - 1], e [L, 3, nc - 1], T [L]) of the L = 4 N M lanes (drone,
    segment, quantity) of peaks_lane_kernel: the t-domain coefficients of the quantity's derivative per slot (x, y, z, or
    the yaw axis in slot 0), zero beyond its degree, and e_j = d_j T^j by repeated multiplication."""
    N, M, _, nc = coef.shape
    L = N * M * 4
    d = np.zeros((L, 3, nc - 1))
    lanes = d.reshape(N * M, 4, 3, nc - 1)
    c = coef.reshape(N * M, 4, nc)
    for q, (r, axes) in enumerate(ORDERS):
        for s, a in enumerate(axes):
            lanes[:, q, s, :nc - r] = _deriv_fp64(c[:, a, :], r)
    T = np.repeat(dur.reshape(-1), 4)
    e = np.empty_like(d)
    tp = np.ones(L)
    for j in range(nc - 1):
        e[:, :, j] = d[:, :, j] * tp[:, None]
        tp = tp * T
    return d, e, T


class WalkPeaks(NamedTuple):
    """walk_peaks' result.  The first four are fp64_walk_peaks' tuple."""
    peak: np.ndarray         # [N, 4]; NaN for a drone with a status
    t_peak: np.ndarray       # [N, 4]
    nodes: np.ndarray        # [N, M, 4] nodes each lane visited (0: a lane that did not walk)
    capped: np.ndarray       # [N, M, 4] lanes that met the depth cap with an open node, or the node guard
    status: np.ndarray       # [N] msnap_status
    seg: np.ndarray          # [N, 4] the segment whose lane the fold took
    t_local: np.ndarray      # [N, 4] that lane's local time T u: t_peak = (the segment's start) + t_local, rounded


def fp64_walk_peaks(coef, dur):
    """(peak [N, 4], t_peak [N, 4], nodes [N, M, 4], capped [N, M, 4]) of walk_peaks."""
    return tuple(walk_peaks(coef, dur)[:4])


def walk_peaks(coef, dur):
    """coef [N, M, 4, nc], dur [N, M] -> WalkPeaks by the
    kernel's method in NumPy fp64: derivative()'s operation order, e_j = d_j T^j, per node the Taylor shift and the exact
    scaling, the largest Bernstein coefficient of the sum of squares, the attained values at the node's ends and middle
    (dyadic_walk.walk on -g, so that its minimum and its tie rule serve a maximum), the prune rule bound > best (1 +
    1e-9) + 1e-26 and the caps; then msnap_eval_flat's unfused Horner at t = T best_u and the fold of each drone's
    segments on eval_flat's running sums: larger value, then earlier absolute time.  The walk itself uses no fma where
    the kernel does; the final Horner and the fold are the kernel's operations one for one.  peak and t_peak are NaN
    for a drone with a non-finite input or a duration <= 0."""
    coef = np.asarray(coef, dtype=np.float64)
    dur = np.asarray(dur, dtype=np.float64)
    N, M, _, nc = coef.shape
    D, n = nc - 2, 2 * (nc - 2)
    Wt = _bernstein_weights(n)
    with np.errstate(invalid="ignore", over="ignore"):
        d_all, e_all, T_all = lane_polynomials(coef, dur)
    used = np.zeros((4, 4), dtype=bool)                    # [q, axis]: a lane reads (and tests) only its own axes
    for q, (_, axes) in enumerate(ORDERS):
        used[q, list(axes)] = True
    fin_axis = np.isfinite(coef).all(axis=3)               # [N, M, 4 axes]
    finite = (fin_axis[:, :, None, :] | ~used[None, None]).all(axis=3) & np.isfinite(dur)[:, :, None]      # [N, M, 4]
    ok = (finite & (dur > 0.0)[:, :, None]).reshape(-1)
    lanes = np.nonzero(ok)[0]
    e, T = e_all[lanes], T_all[lanes]

    def node(act, a, hh, best, best_u):
        A = len(act)
        G = np.zeros((A, n + 1))
        g0, gm, g1 = np.zeros(A), np.zeros(A), np.zeros(A)
        scale = hh[:, None] ** np.arange(D + 1)
        for s in range(3):
            f = _taylor(e[act, s, :], a) * scale
            for i in range(D + 1):
                G[:, i:i + D + 1] += f[:, i:i + 1] * f
            vm = np.zeros(A)
            for j in range(D, -1, -1):
                vm = vm * 0.5 + f[:, j]
            v1 = f[:, ::-1].cumsum(axis=1)[:, -1]
            g0 += f[:, 0] ** 2
            gm += vm ** 2
            g1 += v1 ** 2
        bound = (G @ Wt.T).max(axis=1)
        nb, nu = DW.take_attained(((-g0, a), (-gm, a + 0.5 * hh), (-g1, a + hh)), best, best_u)
        return -bound, nb, nu, bound > (-nb) * (1 + PRUNE_REL) + PRUNE_ABS

    _, best_u, _, lane_nodes, lane_capped = DW.walk(len(lanes), node, MAX_DEPTH, MAX_NODES)

    # the attained value again in the t domain: msnap_eval_flat's derivative Horner, unfused
    tl = T * best_u
    gv = np.zeros(len(lanes))
    for s in range(3):
        v = np.zeros(len(lanes))
        for j in range(nc - 2, -1, -1):
            v = v * tl + d_all[lanes, s, j]
        gv = gv + v * v
    g_lane = np.where(finite.reshape(-1), -1.0, np.nan)
    t_lane = np.full(N * M * 4, np.nan)
    g_lane[lanes], t_lane[lanes] = gv, tl
    g_lane, t_lane = g_lane.reshape(N, M, 4), t_lane.reshape(N, M, 4)

    # peaks_fold_kernel
    best = np.full((N, 4), -1.0)
    bt = np.zeros((N, 4))
    seg = np.zeros((N, 4), dtype=np.int64)
    t_local = np.zeros((N, 4))
    acc = np.zeros(N)
    with np.errstate(invalid="ignore"):
        for i in range(M):
            g, t = g_lane[:, i, :], acc[:, None] + t_lane[:, i, :]
            take = (g > best) | ((g == best) & (t < bt))
            best, bt = np.where(take, g, best), np.where(take, t, bt)
            seg, t_local = np.where(take, i, seg), np.where(take, t_lane[:, i, :], t_local)
            acc = acc + dur[:, i]
        nonfinite = np.isnan(g_lane).any(axis=(1, 2))
        times = (g_lane < 0.0).any(axis=(1, 2))
        status = np.where(nonfinite, 3, np.where(times, 2, 0)).astype(np.int32)
        peak = np.where(status[:, None] != 0, np.nan, np.sqrt(np.maximum(best, 0.0)))
    t_peak = np.where(status[:, None] != 0, np.nan, bt)
    nodes = np.zeros(N * M * 4, dtype=np.int64)
    capped = np.zeros(N * M * 4, dtype=bool)
    nodes[lanes], capped[lanes] = lane_nodes, lane_capped
    return WalkPeaks(peak, t_peak, nodes.reshape(N, M, 4), capped.reshape(N, M, 4), status, seg, t_local)


# ---------------------------------------------------------------------------------------------------- fp64 reference
def _deriv_u(coef, dur, r):
    """[..., nc] t-domain coefficients -> coefficients in u of p^(r)(T u) ([..., nc - r])."""
    nc = coef.shape[-1]
    c = coef.copy()
    for _ in range(r):
        c = c[..., 1:] * np.arange(1, c.shape[-1])
    return c * dur[..., None] ** np.arange(nc - r)


def _g(hs):
    """sum of squares of the component polynomials [K, A, D+1] -> [K, 2D+1] (ascending)."""
    K, A, D1 = hs.shape
    g = np.zeros((K, 2 * D1 - 1))
    for i in range(D1):
        g[:, i:i + D1] += (hs[:, :, i:i + 1] * hs).sum(axis=1)
    return g


def _polyval(c, u):
    """ascending coefficients [K, n], points [K, P] -> [K, P]"""
    v = np.zeros(u.shape)
    for j in range(c.shape[1] - 1, -1, -1):
        v = v * u + c[:, j:j + 1]
    return v


def fp64_peaks(coef, dur, per_segment=False):
    """coef [N, M, 4, nc], dur [N, M] -> peaks [N, 4] (SI units; [N, M, 4] per segment) by roots of g' plus Newton,
    vectorised."""
    N, M, _, nc = coef.shape
    out = np.zeros((N, M, 4))
    for q, (r, axes) in enumerate(ORDERS):
        hs = _deriv_u(coef[:, :, list(axes), :].reshape(N * M, len(axes), nc), dur.reshape(-1)[:, None], r)
        g = _g(hs)                                        # [K, n + 1]
        gp = g[:, 1:] * np.arange(1, g.shape[1])          # g' [K, n]
        gpp = gp[:, 1:] * np.arange(1, gp.shape[1])
        K, n = gp.shape
        scale = np.abs(gp).max(axis=1)
        lead = gp[:, -1]
        ok = np.abs(lead) > 1e-13 * np.where(scale > 0, scale, 1.0)
        cands = [np.zeros((K, 1)), np.ones((K, 1))]
        if n >= 2:
            comp = np.zeros((K, n - 1, n - 1))
            comp[:, 1:, :-1] = np.eye(n - 2)
            safe_lead = np.where(ok, lead, 1.0)
            comp[:, :, -1] = -gp[:, :-1] / safe_lead[:, None]
            ev = np.linalg.eigvals(np.where(ok[:, None, None], comp, 0.0))
            real = np.where(np.abs(ev.imag) < 1e-6, ev.real, 0.0)
            for k in np.nonzero(~ok)[0]:                 # (degenerate leading coefficient: numpy.roots one by one)
                rts = np.roots(gp[k, ::-1]) if scale[k] > 0 else np.zeros(0)
                rr = [z.real for z in rts if abs(z.imag) < 1e-6][:n - 1]
                real[k] = 0.0
                real[k, :len(rr)] = rr
            u = np.clip(real, 0.0, 1.0)
            for _ in range(4):                           # Newton on g'
                d1, d2 = _polyval(gp, u), _polyval(gpp, u)
                step = np.where(np.abs(d2) > 0, d1 / np.where(d2 != 0, d2, 1.0), 0.0)
                u = np.clip(u - step, 0.0, 1.0)
            cands.append(u)
        u = np.concatenate(cands, axis=1)
        gv = _polyval(g, u).max(axis=1)
        out[:, :, q] = np.sqrt(np.maximum(gv, 0.0)).reshape(N, M)
    return out if per_segment else out.max(axis=1)


def candidate_segments(coef, dur, rel=1e-2):
    """Per quantity, the segments of one drone whose fp64 maximum is within `rel` of the drone's (exact_peaks)."""
    seg = fp64_peaks(coef[None], dur[None], per_segment=True)[0]      # [M, 4]
    return [set(np.nonzero(seg[:, q] >= seg[:, q].max() * (1 - rel))[0].tolist()) for q in range(4)]
