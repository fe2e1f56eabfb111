"""Exact and high-precision references for the auxiliary kernels.  TEST INFRASTRUCTURE ONLY.

msnap_oracle.py and msnap_oracle.c restate the kernels operation by operation, so they agree with
them even where both are wrong.  The functions here compute the same quantities from their
definitions instead: every input double is taken as its exact rational value, rational quantities
are computed with fractions.Fraction, and mpmath (50 digits) comes in only where a square root or a
trigonometric function does.  Nothing here follows a kernel's order of operations.

  pt_tri_d2_exact          squared distance from a point to a closed triangle (any triangle:
                           one of zero area is its segment or its point)
  tri_tri_intersect_exact  do two closed triangles meet (degenerate ones included)
  tri_tri_dist2_exact      squared distance between two closed triangles
  snap_cost_exact          sum over segments of the integral of (p^(k))^2, k = ncoef / 2
  flat_eval_hp             the 13 differential-flatness outputs of Trajectory.eval
  formation_exact          R(q) p + t of the formation transform
"""
from __future__ import annotations

import math
from fractions import Fraction as Fr

import mpmath
import numpy as np

DPS = 50


def _fr(x) -> Fr:
    return Fr(float(x))


def _vec(v):
    return tuple(_fr(x) for x in v)


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _zero(v) -> bool:
    return v[0] == 0 and v[1] == 0 and v[2] == 0


# ---- points, segments, triangles (exact rationals) --------------------------------------------
def _pt_seg_d2(p, a, b) -> Fr:
    """closed segment ab; a point when a == b"""
    u = _sub(b, a)
    w = _sub(p, a)
    l2 = _dot(u, u)
    if l2 == 0:
        return _dot(w, w)
    s = _dot(w, u) / l2
    s = min(max(s, Fr(0)), Fr(1))
    e = (w[0] - s * u[0], w[1] - s * u[1], w[2] - s * u[2])
    return _dot(e, e)


def _in_triangle(x, a, b, c, n) -> bool:
    """x in the plane of the triangle abc of nonzero normal n: inside or on its boundary"""
    return (_dot(_cross(_sub(b, a), _sub(x, a)), n) >= 0 and _dot(_cross(_sub(c, b), _sub(x, b)), n) >= 0
            and _dot(_cross(_sub(a, c), _sub(x, c)), n) >= 0)


def _pt_tri_d2(p, a, b, c) -> Fr:
    n = _cross(_sub(b, a), _sub(c, a))
    if not _zero(n):
        h = _dot(_sub(p, a), n)
        nn = _dot(n, n)
        proj = (p[0] - h * n[0] / nn, p[1] - h * n[1] / nn, p[2] - h * n[2] / nn)
        if _in_triangle(proj, a, b, c, n):
            return h * h / nn
    # outside the face, or a triangle of zero area: the nearest point is on one of the closed edges
    return min(_pt_seg_d2(p, a, b), _pt_seg_d2(p, b, c), _pt_seg_d2(p, c, a))


def pt_tri_d2_exact(p, tri) -> Fr:
    """Squared distance from the point p [3] to the triangle tri [3, 3] as a closed point set."""
    a, b, c = (_vec(v) for v in tri)
    return _pt_tri_d2(_vec(p), a, b, c)


def _seg_seg_d2(p0, p1, q0, q1) -> Fr:
    """squared distance between two closed segments (either may be a point)"""
    best = min(_pt_seg_d2(p0, q0, q1), _pt_seg_d2(p1, q0, q1), _pt_seg_d2(q0, p0, p1), _pt_seg_d2(q1, p0, p1))
    u, v, w = _sub(p1, p0), _sub(q1, q0), _sub(p0, q0)
    a, b, c, d, e = _dot(u, u), _dot(u, v), _dot(v, v), _dot(u, w), _dot(v, w)
    den = a * c - b * b
    if den != 0:                       # the lines are not parallel: their closest points, if inside both
        s = (b * e - c * d) / den
        t = (a * e - b * d) / den
        if 0 < s < 1 and 0 < t < 1:
            x = (w[0] + s * u[0] - t * v[0], w[1] + s * u[1] - t * v[1], w[2] + s * u[2] - t * v[2])
            best = min(best, _dot(x, x))
    return best


def _seg_meets_tri(s0, s1, a, b, c) -> bool:
    n = _cross(_sub(b, a), _sub(c, a))
    if _zero(n):                       # the triangle is its edges
        return any(_seg_seg_d2(s0, s1, x, y) == 0 for x, y in ((a, b), (b, c), (c, a)))
    o0, o1 = _dot(_sub(s0, a), n), _dot(_sub(s1, a), n)
    if (o0 > 0 and o1 > 0) or (o0 < 0 and o1 < 0):
        return False
    if o0 == 0 and o1 == 0:            # in the plane: an end inside, or a crossing with an edge
        return (_in_triangle(s0, a, b, c, n) or _in_triangle(s1, a, b, c, n)
                or any(_seg_seg_d2(s0, s1, x, y) == 0 for x, y in ((a, b), (b, c), (c, a))))
    r = o0 / (o0 - o1)                 # the one point where the segment meets the plane
    x = (s0[0] + r * (s1[0] - s0[0]), s0[1] + r * (s1[1] - s0[1]), s0[2] + r * (s1[2] - s0[2]))
    return _in_triangle(x, a, b, c, n)


def tri_tri_intersect_exact(P, Q) -> bool:
    """Do the closed triangles P [3, 3] and Q [3, 3] meet?  Two convex sets of this kind meet iff an edge of one
    meets the other (the intersection, a point, segment or polygon, has its extreme points on edges), so every edge
    of each is tested against the other triangle; a triangle of zero area is the union of its edges."""
    P = [_vec(v) for v in P]
    Q = [_vec(v) for v in Q]
    for A, B in ((P, Q), (Q, P)):
        for i in range(3):
            if _seg_meets_tri(A[i], A[(i + 1) % 3], *B):
                return True
    return False


def tri_tri_dist2_exact(P, Q) -> Fr:
    """Squared distance between the closed triangles P and Q: 0 when they meet, else the minimum over the vertex-to-
    triangle and edge-to-edge distances (where the closest pair of points of two disjoint triangles lies)."""
    if tri_tri_intersect_exact(P, Q):
        return Fr(0)
    Pv = [_vec(v) for v in P]
    Qv = [_vec(v) for v in Q]
    best = min(min(_pt_tri_d2(v, *Qv) for v in Pv), min(_pt_tri_d2(v, *Pv) for v in Qv))
    for i in range(3):
        for j in range(3):
            best = min(best, _seg_seg_d2(Pv[i], Pv[(i + 1) % 3], Qv[j], Qv[(j + 1) % 3]))
    return best


# ---- polynomials ---------------------------------------------------------------------------------
def _deriv(c, k):
    """coefficients (ascending) of the k-th derivative"""
    c = list(c)
    for _ in range(k):
        c = [i * c[i] for i in range(1, len(c))]
    return c


def snap_cost_exact(coef, dur) -> list:
    """coef [M, 4, ncoef], dur [M] -> [4] Fractions: sum over segments of int_0^T (p^(k))^2 dt, k = ncoef // 2."""
    coef = np.asarray(coef, dtype=np.float64)
    M, A, nc = coef.shape
    k = nc // 2
    out = [Fr(0)] * A
    for i in range(M):
        T = _fr(dur[i])
        for a in range(A):
            q = _deriv([_fr(x) for x in coef[i, a]], k)
            sq = [Fr(0)] * (2 * len(q) - 1)
            for m, x in enumerate(q):
                for n, y in enumerate(q):
                    sq[m + n] += x * y
            Tp, acc = T, Fr(0)
            for e, s in enumerate(sq):
                acc += s * Tp / (e + 1)
                Tp *= T
            out[a] += acc
    return out


def snap_cost_terms(coef, dur) -> np.ndarray:
    """[4]: sum over segments of sum_{p,q} |f_p f_q T^(p+q+1) / (p+q+1)|, the scale of the rounding error of J."""
    coef = np.asarray(coef, dtype=np.float64)
    M, A, nc = coef.shape
    k = nc // 2
    fac = np.array([math.factorial(k + q) / math.factorial(q) for q in range(nc - k)])
    e = np.add.outer(np.arange(nc - k), np.arange(nc - k)) + 1.0
    out = np.zeros(A)
    for i in range(M):
        for a in range(A):
            f = np.abs(fac * coef[i, a, k:])
            out[a] += float((np.outer(f, f) * float(dur[i]) ** e / e).sum())
    return out


def _horner(c, t):
    x = Fr(0)
    for v in reversed(c):
        x = x * t + v
    return x


def piece_lookup(dur, t):
    """Trajectory.eval's piece lookup in fp64 (uav_trajectory.py:119-127): the first piece with
    t <= cur + T_i against the running fp64 sum cur; -> (piece, fl(t - cur)), or None outside [0, duration]."""
    t = float(t)
    if not t >= 0.0:
        return None
    cur = 0.0
    for i, T in enumerate(dur):
        if t <= cur + float(T):
            return i, t - cur
        cur = cur + float(T)
    return None


def flat_eval_hp(coef, dur, t) -> np.ndarray:
    """coef [M, 4, nc], dur [M], t -> [13] = pos3 vel3 acc3 omega3 yaw (NaN outside [0, duration]).  The piece and the
    local time are found in fp64 as Trajectory.eval does; the outputs are then evaluated at 50 digits from those
    doubles: the polynomials exactly, the body axes and omega in mpmath."""
    hit = piece_lookup(dur, t)
    if hit is None:
        return np.full(13, np.nan)
    seg, tl = hit
    tl = _fr(tl)
    c = np.asarray(coef, dtype=np.float64)[seg]
    P = [[_fr(x) for x in c[a]] for a in range(4)]
    val = [[_horner(_deriv(P[a], k), tl) for k in range(4)] for a in range(4)]
    with mpmath.workdps(DPS):
        mp = [[mpmath.mpf(v.numerator) / v.denominator for v in row] for row in val]
        acc = [mp[a][2] for a in range(3)]
        jerk = [mp[a][3] for a in range(3)]
        yaw, dyaw = mp[3][0], mp[3][1]
        th = [acc[0], acc[1], acc[2] + mpmath.mpf(9.81)]       # g as the reference has it: the double 9.81
        nt = mpmath.sqrt(th[0] ** 2 + th[1] ** 2 + th[2] ** 2)
        zb = [x / nt for x in th]
        xw = [mpmath.cos(yaw), mpmath.sin(yaw), mpmath.mpf(0)]
        yb = [zb[1] * xw[2] - zb[2] * xw[1], zb[2] * xw[0] - zb[0] * xw[2], zb[0] * xw[1] - zb[1] * xw[0]]
        yn = mpmath.sqrt(yb[0] ** 2 + yb[1] ** 2 + yb[2] ** 2)
        yb = [x / yn for x in yb]
        xb = [yb[1] * zb[2] - yb[2] * zb[1], yb[2] * zb[0] - yb[0] * zb[2], yb[0] * zb[1] - yb[1] * zb[0]]
        jd = jerk[0] * zb[0] + jerk[1] * zb[1] + jerk[2] * zb[2]
        h = [(jerk[i] - jd * zb[i]) / nt for i in range(3)]
        om = [-(h[0] * yb[0] + h[1] * yb[1] + h[2] * yb[2]), h[0] * xb[0] + h[1] * xb[1] + h[2] * xb[2], zb[2] * dyaw]
        out = [mp[a][0] for a in range(3)] + [mp[a][1] for a in range(3)] + acc + om + [yaw]
        return np.array([float(x) for x in out])


# ---- formation transform -------------------------------------------------------------------------
def formation_exact(rb, off) -> list:
    """rb [7] (t, q = x y z w), off [3] -> [3] Fractions: R(q) off + t with KDL's Rotation::Quaternion matrix (no
    normalisation of q), exactly."""
    tx, ty, tz, x, y, z, w = (_fr(v) for v in rb)
    o = _vec(off)
    R = [[w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y],
         [2 * x * y + 2 * w * z, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x],
         [2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, w * w - x * x - y * y + z * z]]
    return [R[r][0] * o[0] + R[r][1] * o[1] + R[r][2] * o[2] + t for r, t in enumerate((tx, ty, tz))]
