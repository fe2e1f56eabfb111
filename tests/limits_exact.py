"""References for the dynamic-limit peaks (include/msnap.h, "dynamic limits"), test side only.

exact_peaks: the coefficients taken as exact Fractions, g = |p^(r)|^2 and g' formed exactly, the real roots of g' in
[0, T] from mpmath.polyroots at 50 digits, g evaluated there and at both ends; max, then sqrt.
fp64_peaks: a vectorised fp64 reference for large batches -- the roots of g' as eigenvalues of its companion matrix
(what numpy.roots does, batched), polished by Newton steps, g at those and at the ends."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

DPS = 50
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


def in_contract(peak, S):
    """include/msnap.h: S (1 - 1e-9) - 1e-12 <= peak <= S (1 + 1e-12) + 1e-12 (peak a float, S an mpf)."""
    S = float(S)
    return S * (1 - 1e-9) - 1e-12 <= peak <= S * (1 + 1e-12) + 1e-12


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
