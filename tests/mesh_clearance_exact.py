"""References for the mesh clearance (include/msnap.h, "mesh clearance"), test side only.

exact_mesh_clearance: the coefficients and the fp64 knot times taken as exact; per (segment, triangle) the candidates
are the segment's ends and the real roots in [0, T] of the derivative of each of the seven feature polynomials (squared
distance to the plane, to the three edge lines, to the three vertices; mpmath.polyroots at 60 digits); the true
point-triangle distance at each candidate, the minimum of all.  A (segment piece, triangle) whose exact box distance
exceeds a value already attained is skipped.
fp64_mesh_clearance: a plain NumPy fp64 restatement of the kernel's walk (csrc/msnap_mesh_clearance.hip), vectorised
over the (drone, segment) lanes and the triangles -- for the node counts and for measuring the rounding of the fp64
method against the exact reference.  Not bit-exact with the kernel (no fused multiply-add, and the
distances come from edge and face projections, not from the sweep's region walk)."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

import clearance_exact as CE  # noqa: F401 (ME.CE: the pairwise module, for the tests that use both)
import dyadic_walk as DW
from clearance_exact import DPS, _mpf, _shift, _squarefree, knots
from dyadic_walk import ABS_CLOSE, ABS_ROUND, EPS, REL_CLOSE, REL_ROUND  # noqa: F401 (re-exported)

# include/msnap.h, "mesh clearance": lower <= D (1 + REL_ROUND) + r, D <= min_dist (1 + REL_ROUND) + r, lower <= min_dist,
# and lower >= min_dist (1 - REL_CLOSE) - ABS_CLOSE - r when the walk closes; r = ABS_ROUND + C_ROUND_MESH 2^-52 R
C_ROUND_MESH = 3.0      # ten times the worst measured, 0.271 (tools/mesh_clearance_rounding.py), rounded up
# csrc/msnap_mesh_clearance.hip
MAX_DEPTH = 40
MAX_NODES = 4096
PRUNE_REL = 1e-9
PRUNE_ABS = 1e-9
TRI_DEGENERATE = 1e-10  # csrc/msnap_tri.h


# ------------------------------------------------------------------------------------------------ triangles, fp64
def finite_tris(tris):
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    return np.isfinite(tris).all(axis=(1, 2))


def tri_degenerate(tris):
    """csrc/msnap_tri.h::tri_degenerate, operation for operation (nothing fused there): [T] bool."""
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        ab, ac = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
        nn = nx * nx + ny * ny + nz * nz
        ab2 = ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1] + ab[:, 2] * ab[:, 2]
        ac2 = ac[:, 0] * ac[:, 0] + ac[:, 1] * ac[:, 1] + ac[:, 2] * ac[:, 2]
        return nn <= TRI_DEGENERATE * (ab2 * ac2)


def unit_normals(tris):
    ab, ac = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    n = np.cross(ab, ac)
    ln = np.sqrt((n * n).sum(axis=1))
    return n * np.where(ln > 0, 1.0 / np.where(ln > 0, ln, 1.0), 0.0)[:, None]


def closest_np(P, tris, degen, normals):
    """P [..., 3] against tris [T, 3, 3] -> (q [..., T, 3], d2 [..., T]): the closest point of each triangle (the union
    of its edges when degenerate) by edge and face projection."""
    P = P[..., None, :]                                        # [..., 1, 3]
    best, q = None, None
    for e in range(3):
        a, b = tris[:, e], tris[:, (e + 1) % 3]
        u = b - a
        l2 = (u * u).sum(axis=1)
        w = P - a
        s = (w * u).sum(axis=-1) / np.where(l2 > 0, l2, 1.0)
        s = np.where(l2 > 0, np.clip(s, 0.0, 1.0), 0.0)
        c = a + s[..., None] * u
        d = ((P - c) ** 2).sum(axis=-1)
        if best is None:
            best, q = d, c
        else:
            take = d < best
            best = np.where(take, d, best)
            q = np.where(take[..., None], c, q)
    h = ((P - tris[:, 0]) * normals).sum(axis=-1)
    foot = P - h[..., None] * normals
    inside = ~degen
    for e in range(3):
        a, b = tris[:, e], tris[:, (e + 1) % 3]
        inside = inside & ((np.cross(b - a, foot - a) * normals).sum(axis=-1) >= 0.0)
    take = inside & (h * h < best)
    best = np.where(take, h * h, best)
    q = np.where(take[..., None], foot, q)
    return q, best


def mesh_R(coef_d, dur_d, tris):
    """R of include/msnap.h: the largest sum_k |c_k| T_i^k over x, y, z and the drone's segments, plus the largest
    |vertex coordinate| of the mesh's finite triangles."""
    coef_d = np.asarray(coef_d, dtype=np.float64)
    dur_d = np.asarray(dur_d, dtype=np.float64)
    pw = dur_d[:, None] ** np.arange(coef_d.shape[2])[None, :]
    R = float((np.abs(coef_d[:, :3, :]) * pw[:, None, :]).sum(axis=2).max())
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    ok = finite_tris(tris)
    return R + (float(np.abs(tris[ok]).max()) if ok.any() else 0.0)


def round_terms(R):
    return DW.round_terms(R, C_ROUND_MESH)


def contract_violations(min_dist, lower, D, closed=True, R=0.0):
    """The inequalities of include/msnap.h that (min_dist, lower) break against the exact D: a list of text.  `R`:
    mesh_R (0: the allowance without its coordinate term, which is stricter)."""
    return DW.contract_violations(min_dist, lower, D, closed, R, C_ROUND_MESH, lower_le_min_dist=True)


def round_ratio(min_dist, lower, D, R, attained=None):
    """What C_ROUND_MESH has to cover, in units of 2^-52 R: dyadic_walk.round_ratio."""
    return DW.round_ratio(min_dist, lower, D, R, attained)


# ------------------------------------------------------------------------------------------------ exact reference
def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def exact_point_tri_dist2(p, tri, degenerate):
    """Squared distance of the point p (3 mpf or Fractions) to the triangle tri (3 x 3 mpf or Fractions): the three
    closed edges, and the face where the foot of the perpendicular falls inside it (not for a degenerate triangle)."""
    best = None
    for e in range(3):
        a, b = tri[e], tri[(e + 1) % 3]
        u, w = _sub(b, a), _sub(p, a)
        l2 = _dot(u, u)
        s = 0
        if l2 > 0:
            s = min(max(_dot(w, u) / l2, 0), 1)
        c = [a[k] + s * u[k] for k in range(3)]
        d = _dot(_sub(p, c), _sub(p, c))
        best = d if best is None or d < best else best
    if not degenerate:
        n = _cross(_sub(tri[1], tri[0]), _sub(tri[2], tri[0]))
        nn = _dot(n, n)
        if nn > 0:
            h = _dot(_sub(p, tri[0]), n)                          # times |n|
            foot = [p[k] - h * n[k] / nn for k in range(3)]
            if all(_dot(_cross(_sub(tri[(e + 1) % 3], tri[e]), _sub(foot, tri[e])), n) >= 0 for e in range(3)):
                best = min(best, h * h / nn)
    return best


def _critical_points(g, h):
    """Real roots in [0, h] of g' (g ascending Fractions), as mpf."""
    gp = [(i + 1) * g[i + 1] for i in range(len(g) - 1)]
    while gp and gp[-1] == 0:
        gp.pop()
    while gp and gp[0] == 0:
        gp.pop(0)
    if len(gp) < 2:
        return []
    coeffs = [_mpf(x) for x in reversed(gp)]
    try:
        roots = mpmath.polyroots(coeffs, maxsteps=200, extraprec=DPS)
    except mpmath.libmp.NoConvergence:
        coeffs = [_mpf(x) for x in reversed(_squarefree([Fraction(x) for x in gp]))]
        roots = mpmath.polyroots(coeffs, maxsteps=4000, extraprec=20 * DPS) if len(coeffs) >= 2 else []
    out = []
    tol = mpmath.mpf(10) ** (-DPS // 2)
    for z in roots:
        z = mpmath.mpc(z)
        if abs(z.imag) <= tol * (1 + abs(z.real)) and -tol <= z.real <= h + tol:
            out.append(min(max(z.real, mpmath.mpf(0)), h))
    return out


def _pmul(a, b):
    out = [Fraction(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return out


def _padd(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0) for i in range(n)]


def _feature_polys(p, tri):
    """The seven squared-distance polynomials of the path p (3 lists of ascending Fractions) against the plane, the
    edge lines and the vertices of tri (3 x 3 Fractions); the ones that vanish identically are left out."""
    out = []
    rel = [[_padd(p[k], [-v[k]]) for k in range(3)] for v in tri]           # p - v_j
    n = _cross(_sub(tri[1], tri[0]), _sub(tri[2], tri[0]))
    if any(n):
        s = [Fraction(0)]
        for k in range(3):
            s = _padd(s, [n[k] * c for c in rel[0][k]])
        out.append(_pmul(s, s))
    for e in range(3):
        u = _sub(tri[(e + 1) % 3], tri[e])
        if any(u):
            w = rel[e]
            cr = [_padd([u[2] * c for c in w[1]], [-u[1] * c for c in w[2]]),
                  _padd([u[0] * c for c in w[2]], [-u[2] * c for c in w[0]]),
                  _padd([u[1] * c for c in w[0]], [-u[0] * c for c in w[1]])]
            g = [Fraction(0)]
            for c in cr:
                g = _padd(g, _pmul(c, c))
            out.append(g)
    for j in range(3):
        g = [Fraction(0)]
        for k in range(3):
            g = _padd(g, _pmul(rel[j][k], rel[j][k]))
        out.append(g)
    return out


def _control_points(p, t0, t1):
    """Exact Bernstein control points of p (3 ascending Fraction lists) on [t0, t1]: 3 lists."""
    from math import comb
    out = []
    for k in range(3):
        c = _shift(p[k], t0)
        h = t1 - t0
        c = [x * h ** j for j, x in enumerate(c)]
        n = len(c) - 1
        out.append([sum(Fraction(comb(i, j), comb(n, j)) * c[j] for j in range(i + 1)) for i in range(n + 1)])
    return out


def _piece_tri_gap2(b, tri, n):
    """An exact lower bound of the squared distance between the hull of the control points b and the triangle tri: the
    boxes' distance, and the separation along the face normal n (the support-plane bound of DESIGN.md §5 K11)."""
    s = Fraction(0)
    for k in range(3):
        tmin, tmax = min(v[k] for v in tri), max(v[k] for v in tri)
        gap = max(Fraction(0), min(b[k]) - tmax, tmin - max(b[k]))
        s += gap * gap
    nn = _dot(n, n)
    if nn:
        proj = [n[0] * x + n[1] * y + n[2] * z for x, y, z in zip(*b)]
        sup = [_dot(n, v) for v in tri]
        val = max(min(proj) - max(sup), min(sup) - max(proj))
        if val > 0:
            s = max(s, val * val / nn)
    return s


def exact_mesh_clearance(coef_d, dur_d, tris, hint_t=None, pieces=16):
    """coef [M, 4, nc], dur [M] of one drone against tris [T, 3, 3] -> (D, t) as mpf: the infimum over [0, sum dur] and
    all triangles of the sweep's distance function (degenerate triangles as their edges, non-finite ones skipped) and a
    time at which it is attained.  `hint_t`: absolute times (floats) whose exact distances seed the value the box test
    skips against (any attained value is valid there).  A value below 1e-30 m ends the search: a crossing, D = 0."""
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    ok, degen = finite_tris(tris), tri_degenerate(tris)
    ks = knots(dur_d)
    starts = [0.0] + ks[:-1]
    best, bt = None, None
    with mpmath.workdps(DPS):
        mtris = {t: [[mpmath.mpf(float(x)) for x in v] for v in tris[t]] for t in range(len(tris)) if ok[t]}
        ftris = {t: [[Fraction(float(x)) for x in v] for v in tris[t]] for t in mtris}
        fnorm = {t: _cross(_sub(ftris[t][1], ftris[t][0]), _sub(ftris[t][2], ftris[t][0])) for t in mtris}
        crossing = mpmath.mpf(10) ** -60

        def dist2_at(i, tau, only=None):
            pt = [mpmath.polyval([mpmath.mpf(float(x)) for x in coef_d[i, ax][::-1]], tau) for ax in range(3)]
            vals = [(exact_point_tri_dist2(pt, mtris[t], bool(degen[t])), t) for t in (mtris if only is None else only)]
            return min(vals)[0] if vals else None

        def offer(v, t):
            nonlocal best, bt
            if v is not None and (best is None or v < best or (v == best and t < bt)):
                best, bt = v, t

        for ht in ([] if hint_t is None else hint_t):
            i = next((i for i, x in enumerate(ks) if ht <= x), len(ks) - 1)
            offer(dist2_at(i, mpmath.mpf(float(ht)) - mpmath.mpf(starts[i])), mpmath.mpf(float(ht)))
        for i in range(len(ks)):
            T = Fraction(float(dur_d[i]))
            p = [[Fraction(float(x)) for x in coef_d[i, ax]] for ax in range(3)]
            h = _mpf(T)
            for tau in (mpmath.mpf(0), h):
                offer(dist2_at(i, tau), mpmath.mpf(starts[i]) + tau)
            hulls = [_control_points(p, T * j / pieces, T * (j + 1) / pieces) for j in range(pieces)]
            for t in mtris:
                if best is not None and best < crossing:
                    return mpmath.mpf(0), bt
                if best is not None:
                    bq = Fraction(float(best)) * (1 + Fraction(1, 10 ** 12))       # (the mpf rounded to fp64, with slack)
                    if all(_piece_tri_gap2(b, ftris[t], fnorm[t]) > bq for b in hulls):
                        continue
                for g in _feature_polys(p, ftris[t]):
                    for tau in _critical_points(g, h):
                        offer(dist2_at(i, tau, only=[t]), mpmath.mpf(starts[i]) + tau)
        if best is None:
            return mpmath.inf, mpmath.mpf(0)
        return mpmath.sqrt(max(best, mpmath.mpf(0))), bt


def exact_distance_at(coef_d, dur_d, tris, t):
    """The sweep's distance function of the drone at absolute time t (a float), exactly (mpf)."""
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    ok, degen = finite_tris(tris), tri_degenerate(tris)
    ks = knots(dur_d)
    with mpmath.workdps(DPS):
        i = next((i for i, x in enumerate(ks) if t <= x), len(ks) - 1)
        tl = mpmath.mpf(float(t)) - mpmath.mpf(([0.0] + ks)[i])
        pt = [mpmath.polyval([mpmath.mpf(float(x)) for x in coef_d[i, ax][::-1]], tl) for ax in range(3)]
        vals = [exact_point_tri_dist2(pt, [[mpmath.mpf(float(x)) for x in v] for v in tris[t_]], bool(degen[t_]))
                for t_ in range(len(tris)) if ok[t_]]
        return mpmath.sqrt(min(vals)) if vals else mpmath.inf


# ------------------------------------------------------------------------------------------------ fp64 restatement
def fp64_mesh_clearance(coef, dur, tris, stats=None):
    """coef [N, M, 4, nc], dur [N, M] (valid, finite), tris [T, 3, 3] -> (min_dist [N], t_min [N], tri_min [N],
    lower [N]) by the kernel's method in NumPy fp64.  `stats` (a dict) receives the nodes per lane ("nodes") and the
    lanes that met the depth cap or the node guard ("capped")."""
    coef = np.asarray(coef, dtype=np.float64)
    dur = np.asarray(dur, dtype=np.float64)
    all_tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    keep = np.nonzero(finite_tris(all_tris))[0]
    tris = all_tris[keep]
    Tn = len(tris)
    degen, normals = tri_degenerate(tris), unit_normals(tris)
    N, M, nc = dur.shape[0], dur.shape[1], coef.shape[3]
    D = nc - 1
    Wt = DW._bernstein_weights(D)
    K = np.add.accumulate(dur, axis=1)
    start = np.concatenate([np.zeros((N, 1)), K[:, :-1]], axis=1).reshape(-1)
    T = dur.reshape(-1)
    E = start + T
    L = N * M
    e = coef[:, :, :3, :].reshape(L, 3, nc) * (T[:, None] ** np.arange(nc))[:, None, :]
    tmin_box, tmax_box = tris.min(axis=1), tris.max(axis=1)               # [T, 3]

    def node(act, a, hh, best, best_u):
        A = len(act)
        scale = hh[:, None] ** np.arange(nc)
        B = np.zeros((A, 3, nc))
        P = np.zeros((A, 3, 3))                                       # [lane, point, axis]
        for s in range(3):
            f = DW._taylor(e[act, s, :], a) * scale
            vm = np.zeros(A)
            for j in range(D, -1, -1):
                vm = vm * 0.5 + f[:, j]
            P[:, 0, s], P[:, 1, s], P[:, 2, s] = f[:, 0], vm, f[:, ::-1].cumsum(axis=1)[:, -1]
            B[:, s, :] = f @ Wt.T
        lo, hi = B.min(axis=2), B.max(axis=2)                         # [A, 3]
        sb0 = np.sqrt(best)
        thr0 = sb0 - PRUNE_REL * sb0 - PRUNE_ABS
        nb, nu = best, best_u
        bound = np.full(A, np.inf)
        if Tn:
            gap = np.maximum(0.0, np.maximum(lo[:, None, :] - tmax_box[None], tmin_box[None] - hi[:, None, :]))
            lb2 = (gap * gap).sum(axis=2)                             # [A, T]
            need = ~((thr0 > 0.0)[:, None] & (lb2 >= (thr0 * thr0)[:, None]))
            q, d2 = closest_np(P, tris, degen, normals)               # [A, 3, T, 3], [A, 3, T]
            d2n = np.where(need[:, None, :], d2, np.inf).min(axis=2)
            nb, nu = DW.take_attained(((d2n[:, 0], a), (d2n[:, 1], a + 0.5 * hh), (d2n[:, 2], a + hh)), best, best_u)
            fi = np.where(d2[:, 1] > d2[:, 0], np.where(d2[:, 2] > d2[:, 1], 2, 1), np.where(d2[:, 2] > d2[:, 0], 2, 0))
            ai, ti = np.arange(A)[:, None], np.arange(Tn)[None, :]
            dirv = P[ai, fi, :] - q[ai, fi, ti, :]                    # [A, T, 3]
            ln = np.sqrt((dirv * dirv).sum(axis=2))
            dirv = dirv * np.where(ln > 0, 1.0 / np.where(ln > 0, ln, 1.0), 0.0)[..., None]
            pn = np.einsum("tk,akd->atd", normals, B)
            pa = np.einsum("atk,akd->atd", dirv, B)
            sn = np.einsum("tk,tjk->tj", normals, tris)               # [T, 3]
            sa = np.einsum("atk,tjk->atj", dirv, tris)
            tb = np.fmax(np.fmax(pn.min(axis=2) - sn.max(axis=1)[None], sn.min(axis=1)[None] - pn.max(axis=2)),
                         pa.min(axis=2) - sa.max(axis=2))
            bound = np.where(need, tb, np.inf).min(axis=1)
            skipped = np.where(need, np.inf, lb2).min(axis=1)
            bound = np.fmin(bound, np.fmax(np.sqrt(skipped), thr0))
        sb = np.sqrt(nb)
        return bound, nb, nu, bound < sb - PRUNE_REL * sb - PRUNE_ABS

    with np.errstate(all="ignore"):
        best, best_u, low, nodes, capped = DW.walk(L, node, MAX_DEPTH, MAX_NODES)

        tm = np.minimum(T * best_u + start, E)
        best, tm, low = best.reshape(N, M), tm.reshape(N, M), low.reshape(N, M)
        g = best.min(axis=1)
        t_d = np.where(best == g[:, None], tm, np.inf).min(axis=1)
        t_d = np.where(np.isfinite(t_d), t_d, 0.0)
        low_d = low.min(axis=1)
        pos = DW._positions(coef, dur, np.arange(N), t_d)
        if Tn:
            _, d2 = closest_np(pos, tris, degen, normals)                 # [N, T]
            tri = d2.argmin(axis=1)
            md = np.sqrt(d2[np.arange(N), tri])
            tri = keep[tri].astype(np.int32)
        else:
            md, tri = np.full(N, np.inf), np.full(N, -1, dtype=np.int32)
        lower = np.minimum(np.maximum(low_d, 0.0), md)
    if stats is not None:
        stats["nodes"], stats["capped"] = nodes.reshape(N, M), capped.reshape(N, M)
    return md, t_d, tri, lower


# ------------------------------------------------------------------------------------------------ shared test helper
def check_contract(clearance, coef, dur, tris, with_R=False, closed=True, drones=None, exact=None):
    """`clearance(coef, dur, tris)` -> (min_dist, t_min, tri_min, lower, status) checked per drone (at most 12: the
    exact reference is slow) against exact_mesh_clearance: no status raised, the header's inequalities, t_min inside
    the flight.  with_R: the allowance with its coordinate term (without it the check is stricter).  Prints each
    drone's figures; returns (min_dist, t_min, tri_min, lower, worst round_ratio)."""
    md, tm, tri, lower, status = clearance(coef, dur, tris)
    assert (np.asarray(status) == 0).all()
    drones = range(len(md)) if drones is None else drones
    assert len(drones) <= 12
    worst = -np.inf
    for d in drones:
        D, _ = exact_mesh_clearance(coef[d], dur[d], tris, hint_t=[float(tm[d])]) if exact is None else (exact[d], None)
        R = mesh_R(coef[d], dur[d], tris)
        ratio = round_ratio(md[d], lower[d], D, R, exact_distance_at(coef[d], dur[d], tris, float(tm[d])))
        worst = max(worst, ratio)
        print(f"drone {d}: lower {lower[d]!r} D {float(D)!r} min_dist {md[d]!r} t_min {tm[d]!r} tri {tri[d]} "
              f"R {R:.4g} rounding / (2^-52 R) {ratio:.3f}")
        assert not contract_violations(md[d], lower[d], D, closed=closed, R=R if with_R else 0.0), d
        assert 0.0 <= tm[d] <= knots(dur[d])[-1]
    print(f"worst rounding / (2^-52 R): {worst:.3f} (C_ROUND_MESH {C_ROUND_MESH})")
    assert worst < C_ROUND_MESH
    return md, tm, tri, lower, worst
