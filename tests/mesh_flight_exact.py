"""A second, fast exact reference for the mesh clearance (include/msnap.h, "mesh clearance"), for straight flights only.

A straight rest-to-rest segment is p(t) = a + s(t / T) (q - a), s the step polynomial of the order: 35 x^4 - 84 x^5 +
70 x^6 - 20 x^7 at order 7, 126 x^5 - 420 x^6 + 540 x^7 - 315 x^8 + 70 x^9 at order 9.  s rises monotonically from 0
to 1 (s' = 140 x^3 (1 - x)^3, 630 x^4 (1 - x)^4), so the path is exactly the line segment [a, q].  With a and q on a
dyadic lattice and T a power of two every fp64 coefficient is exact (flight asserts it), and the D of the header is
the distance between a polyline and a set of triangles: per (segment, triangle) the smallest of the two end points
against the triangle, the segment against the three edges (the clamped closed form, no iteration), and 0 when the
segment pierces the face.  All of it in Fractions, one mpmath square root at the end.  The triangle semantics are
tests/mesh_clearance_exact.py's: a degenerate triangle (tri_degenerate) is the union of its edges, a non-finite one is
skipped.  Written without reading exact_mesh_clearance's candidates (roots of feature polynomials): the two agree to
1e-50 where both run (tests/test_mesh_clearance_edges_cpu.py)."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

import mesh_clearance_exact as ME
from clearance_exact import DPS

STEP = {8: (4, (35, -84, 70, -20)), 10: (5, (126, -420, 540, -315, 70))}      # nc -> (first power, coefficients)


def _exact3(v):
    return [Fraction(float(x)) for x in v]


def flight(p, q, T, nc):
    """coef [4, nc] of the straight rest-to-rest segment from p to q (3 floats each) in T seconds; yaw zero.  Every
    coefficient is asserted exact: c_0 = p, c_k T^k = (q - p) step_k."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    T = float(T)
    k0, step = STEP[nc]
    coef = np.zeros((4, nc))
    u = q - p
    for ax in range(3):
        assert Fraction(float(u[ax])) == Fraction(float(q[ax])) - Fraction(float(p[ax])), (p, q)
        coef[ax, 0] = p[ax]
        for i, s in enumerate(step):
            k = k0 + i
            c = u[ax] * s / T ** k
            assert Fraction(float(c)) * Fraction(T) ** k == Fraction(float(u[ax])) * s, (p, q, T, k)
            coef[ax, k] = c
    return coef


def path(points, durs, nc):
    """points [M + 1, 3], durs [M] -> (coef [M, 4, nc], dur [M]): the polyline through the points, at rest at each."""
    points = np.asarray(points, dtype=np.float64)
    durs = np.asarray(durs, dtype=np.float64)
    assert points.shape == (len(durs) + 1, 3)
    return np.stack([flight(points[i], points[i + 1], durs[i], nc) for i in range(len(durs))]), durs.copy()


# ------------------------------------------------------------------------------------------------ exact distances
def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _clamp(x):
    return min(max(x, 0), 1)


def _end_feature(t):
    return "vertex" if t == 0 or t == 1 else "edge"


def seg_seg(p1, q1, p2, q2):
    """Squared distance of the closed segments [p1, q1] and [p2, q2] (Fractions) and the parameters (s, t) of one
    pair of closest points: the clamped closed form -- the unconstrained minimum of the lines clamped on the first
    segment, the second segment's parameter from it, and where that leaves [0, 1] the first one again."""
    d1, d2, r = _sub(q1, p1), _sub(q2, p2), _sub(p1, p2)
    a, e, f = _dot(d1, d1), _dot(d2, d2), _dot(d2, r)
    if a == 0 and e == 0:
        s = t = Fraction(0)
    elif a == 0:
        s, t = Fraction(0), _clamp(f / e)
    else:
        c = _dot(d1, r)
        if e == 0:
            s, t = _clamp(-c / a), Fraction(0)
        else:
            b = _dot(d1, d2)
            den = a * e - b * b
            s = _clamp((b * f - c * e) / den) if den != 0 else Fraction(0)
            t = (b * s + f) / e
            if t < 0:
                s, t = _clamp(-c / a), Fraction(0)
            elif t > 1:
                s, t = _clamp((b - c) / a), Fraction(1)
    w = [r[k] + s * d1[k] - t * d2[k] for k in range(3)]
    return _dot(w, w), s, t


def point_tri(p, tri, degenerate):
    """Squared distance of the point p to the triangle tri (Fractions) and the feature the closest point lies on: a
    vertex or an open edge (the three closed edges), or the open face when the foot of the perpendicular falls strictly
    nearer than every edge."""
    best, feat = None, None
    for e in range(3):
        a, b = tri[e], tri[(e + 1) % 3]
        u, w = _sub(b, a), _sub(p, a)
        l2 = _dot(u, u)
        t = _clamp(_dot(w, u) / l2) if l2 > 0 else Fraction(0)
        c = [a[k] + t * u[k] - p[k] for k in range(3)]
        d = _dot(c, c)
        if best is None or d < best or (d == best and feat == "edge" and _end_feature(t) == "vertex"):
            best, feat = d, _end_feature(t) if l2 > 0 else "vertex"
    if not degenerate:
        n = _cross(_sub(tri[1], tri[0]), _sub(tri[2], tri[0]))
        nn = _dot(n, n)
        if nn > 0:
            h = _dot(_sub(p, tri[0]), n)
            foot = [p[k] - h * n[k] / nn for k in range(3)]
            if all(_dot(_cross(_sub(tri[(e + 1) % 3], tri[e]), _sub(foot, tri[e])), n) >= 0 for e in range(3)):
                if h * h / nn < best:
                    best, feat = h * h / nn, "face"
    return best, feat


def _pierces(p, q, tri):
    """The parameter s in [0, 1] at which the segment [p, q] meets the closed triangle's plane inside the triangle, or
    None (a segment inside the plane is left to the edges and the end points)."""
    n = _cross(_sub(tri[1], tri[0]), _sub(tri[2], tri[0]))
    hp, hq = _dot(_sub(p, tri[0]), n), _dot(_sub(q, tri[0]), n)
    if hp == hq or (hp > 0 and hq > 0) or (hp < 0 and hq < 0):
        return None
    s = hp / (hp - hq)
    x = [p[k] + s * (q[k] - p[k]) for k in range(3)]
    if all(_dot(_cross(_sub(tri[(e + 1) % 3], tri[e]), _sub(x, tri[e])), n) >= 0 for e in range(3)):
        return s
    return None


def segment_triangle(p, q, tri, degenerate):
    """(squared distance, feature, s) of the segment [p, q] against the triangle tri, all Fractions: s is the segment's
    parameter at one closest approach, feature the part of the triangle the closest point lies on -- "crossing" whenever
    the distance is zero.  End points first, then the edges: of several closest pairs the end point's is reported."""
    if not degenerate:
        s = _pierces(p, q, tri)
        if s is not None:
            return Fraction(0), "crossing", s
    best, feat, bs = None, None, None
    for s, x in ((Fraction(0), p), (Fraction(1), q)):
        d, f = point_tri(x, tri, degenerate)
        if best is None or d < best:
            best, feat, bs = d, f, s
    for e in range(3):
        a, b = tri[e], tri[(e + 1) % 3]
        if a == b:
            continue
        d, s, t = seg_seg(p, q, a, b)
        if d < best:
            best, feat, bs = d, _end_feature(t), s
    return best, ("crossing" if best == 0 else feat), bs


def _box_gap2(lo1, hi1, lo2, hi2):
    g = Fraction(0)
    for k in range(3):
        d = max(lo1[k] - hi2[k], lo2[k] - hi1[k], 0)
        g += d * d
    return g


def polyline_closest(points, tris):
    """points [M + 1, 3] against tris [T, 3, 3] -> (squared distance as a Fraction or None without a finite triangle,
    feature, segment, s, triangle) of the first closest approach found (segments, then triangles, in index order;
    strictly smaller wins).  A (segment, triangle) whose boxes lie farther apart than a value already attained is
    skipped."""
    points = np.asarray(points, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    ok, degen = ME.finite_tris(tris), ME.tri_degenerate(tris)
    P = [_exact3(x) for x in points]
    ftris = {t: [_exact3(v) for v in tris[t]] for t in range(len(tris)) if ok[t]}
    tbox = {t: ([min(v[k] for v in tr) for k in range(3)], [max(v[k] for v in tr) for k in range(3)])
            for t, tr in ftris.items()}
    best = (None, None, None, None, None)
    for i in range(len(P) - 1):
        p, q = P[i], P[i + 1]
        lo, hi = [min(p[k], q[k]) for k in range(3)], [max(p[k], q[k]) for k in range(3)]
        for t, tr in ftris.items():
            if best[0] is not None and _box_gap2(lo, hi, *tbox[t]) > best[0]:
                continue
            d, f, s = segment_triangle(p, q, tr, bool(degen[t]))
            if best[0] is None or d < best[0]:
                best = (d, f, i, s, t)
                if d == 0:
                    return best
    return best


def exact_polyline_clearance(points, tris):
    """(D as mpf, feature) of the polyline through points [M + 1, 3] against tris [T, 3, 3]: feature is "vertex", "edge"
    or "face" -- where on the winning triangle the closest point lies -- or "crossing" (D = 0); (inf, None) without a
    finite triangle."""
    d2, feat = polyline_closest(points, tris)[:2]
    with mpmath.workdps(DPS):
        if d2 is None:
            return mpmath.inf, None
        return mpmath.sqrt(mpmath.mpf(d2.numerator) / mpmath.mpf(d2.denominator)), feat
