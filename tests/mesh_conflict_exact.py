"""References for the mesh conflict windows (include/msnap.h, "mesh conflict windows"), test side only.

Exact, for straight flights (tests/mesh_flight_exact.py).  A straight flight is p(t) = a + s(t / T) (q - a) with s
monotone, and the distance of a point of a line to one triangle is convex in the line parameter: each (segment, triangle)
has one open sub-level interval {distance < threshold}.  Its ends are found by bisection on the exact rational
point-triangle distance (mesh_clearance_exact.exact_point_tri_dist2) to 2^-70 and mapped to time through the step
polynomial with mpmath at DPS digits.  From those:
  StraightExact.ranges     the maximal ranges on which the drone is in conflict (joined across triangles and knots),
  StraightExact.speeds     the crossing speed |d/dt distance| [m/s] at every entry and exit that is a root,
  StraightExact.touches    the (segment, triangle) whose smallest distance equals the threshold exactly,
  StraightExact.infimum    the exact infimum of the distance over any sub-range [t0, t1]: the truncated polyline has
                           exact rational end points (s of a rational is rational), which segment_triangle takes.
CurvedExact: the infimum over a sub-range for any path, from mesh_clearance_exact's candidates (ends and critical points
of the feature polynomials) restricted to the range; no ranges, so no closing checks.
fp64_mesh_conflict_window: a plain NumPy fp64 restatement of the lane and fold rules of csrc/msnap_mesh_conflict.hip,
vectorised over the (drone, segment) lanes and the triangles.  Not bit-exact with the kernel (no fused multiply-add, and
the distances come from edge and face projections, not from the sweep's region walk).
check_mesh_windows: the per-drone checks against the exact reference, shared by the CPU and the GPU tests."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

import dyadic_walk as DW
import mesh_clearance_exact as ME
import mesh_flight_exact as MF
from clearance_exact import DPS, _mpf, knots
from dyadic_walk import ABS_ROUND, EPS, trailing_ones
from mesh_clearance_exact import MAX_DEPTH, MAX_NODES

OUTPUTS = ("t_clear_until", "t_first", "d_first", "tri_first", "t_last", "d_last", "tri_last", "t_clear_from")
TIMES = (0, 1, 4, 7)                # the four times among them
CLEAR = (np.inf, np.inf, np.inf, -1, -np.inf, np.inf, -1, -np.inf)
# include/msnap.h, "mesh conflict windows": r = ABS_ROUND + C_ROUND_MESH_WINDOW 2^-52 R.  Ten times the worst deviation
# measured, 0.732 on the restatement and 0.609 on the kernel (tools/mesh_conflict_window_rounding.py),
# rounded up: more than msnap_mesh_clearance's C_ROUND_MESH = 3, so the header states a constant of its own
C_ROUND_MESH_WINDOW = 8.0
BISECT_BITS = 70


def allowance(coef_d, dur_d, tris):
    return ABS_ROUND + C_ROUND_MESH_WINDOW * EPS * ME.mesh_R(coef_d, dur_d, tris)


def ulp(x):
    return float(np.spacing(abs(float(x))))


# ------------------------------------------------------------------------------------------------ exact, straight
def step(nc, x):
    """s(x) of mesh_flight_exact.STEP, in the arithmetic of x (a Fraction stays one)."""
    k0, c = MF.STEP[nc]
    return sum(ck * x ** (k0 + i) for i, ck in enumerate(c))


def step_rate(nc, x):
    k0, c = MF.STEP[nc]
    return sum((k0 + i) * ck * x ** (k0 + i - 1) for i, ck in enumerate(c))


def step_inverse(nc, lam):
    """x in [0, 1] with s(x) = lam (a Fraction in [0, 1]) as mpf: fp64 bisection, then Newton at DPS digits."""
    if lam <= 0:
        return mpmath.mpf(0)
    if lam >= 1:
        return mpmath.mpf(1)
    lo, hi, fl = 0.0, 1.0, float(lam)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if step(nc, mid) < fl else (lo, mid)
    x, target = mpmath.mpf(0.5 * (lo + hi)), _mpf(lam)
    for _ in range(8):
        x = x - (step(nc, x) - target) / step_rate(nc, x)
    assert abs(step(nc, x) - target) < mpmath.mpf(10) ** (-DPS + 8)
    return x


class StraightExact:
    """One polyline flight (points [M + 1, 3] on the lattice, durs [M] powers of two, nc) against tris at `threshold`."""

    def __init__(self, points, durs, nc, tris, threshold):
        self.nc, self.threshold = nc, float(threshold)
        self.P = [[Fraction(float(x)) for x in p] for p in np.asarray(points, dtype=np.float64)]
        self.T = [Fraction(float(x)) for x in durs]
        ks = knots(durs)
        self.K = [Fraction(0)] + [Fraction(x) for x in ks]
        assert all(self.K[i] + self.T[i] == self.K[i + 1] for i in range(len(self.T)))      # exact running sums
        self.W = self.K[-1]
        tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
        ok, degen = ME.finite_tris(tris), ME.tri_degenerate(tris)
        self.tris = [([[Fraction(float(x)) for x in v] for v in tris[t]], bool(degen[t])) for t in range(len(tris)) if ok[t]]
        self.L = Fraction(self.threshold) ** 2
        self._ranges = None

    # -- geometry in the line parameter
    def _at(self, i, lam):
        p, q = self.P[i], self.P[i + 1]
        return [p[k] + lam * (q[k] - p[k]) for k in range(3)]

    def _dist2(self, i, lam, only=None):
        x = self._at(i, lam)
        return min(ME.exact_point_tri_dist2(x, tr, dg) for tr, dg in (self.tris if only is None else [only]))

    def _root(self, i, tri, inside, outside):
        """The line parameter between `inside` (distance < threshold) and `outside` (>=) at which the distance to the
        one triangle crosses the threshold, to 2^-BISECT_BITS."""
        while abs(outside - inside) > Fraction(1, 2 ** BISECT_BITS):
            mid = (inside + outside) / 2
            if self._dist2(i, mid, tri) < self.L:
                inside = mid
            else:
                outside = mid
        return (inside + outside) / 2

    def _segment_intervals(self, i):
        """[(lam_in, lam_out, in_is_root, out_is_root)] of segment i, joined over the triangles; and the touches."""
        p, q = self.P[i], self.P[i + 1]
        lo, hi = [min(p[k], q[k]) for k in range(3)], [max(p[k], q[k]) for k in range(3)]
        raw, touches = [], []
        for tr, dg in self.tris:
            tb = ([min(v[k] for v in tr) for k in range(3)], [max(v[k] for v in tr) for k in range(3)])
            if MF._box_gap2(lo, hi, *tb) > self.L:
                continue
            d2, _, s = MF.segment_triangle(p, q, tr, dg)
            if d2 == self.L and p != q:
                touches.append(i)
            if not d2 < self.L:
                continue
            if p == q:
                raw.append((Fraction(0), Fraction(1), False, False))
                continue
            a_in = self._dist2(i, Fraction(0), (tr, dg)) < self.L
            b_in = self._dist2(i, Fraction(1), (tr, dg)) < self.L
            raw.append((Fraction(0) if a_in else self._root(i, (tr, dg), s, Fraction(0)),
                        Fraction(1) if b_in else self._root(i, (tr, dg), s, Fraction(1)), not a_in, not b_in))
        raw.sort(key=lambda r: r[0])
        out = []
        for r in raw:
            if out and r[0] <= out[-1][1]:
                if r[1] > out[-1][1]:
                    out[-1] = (out[-1][0], r[1], out[-1][2], r[3])
            else:
                out.append(r)
        return out, touches

    def _time(self, i, lam):
        return _mpf(self.K[i]) + _mpf(self.T[i]) * step_inverse(self.nc, lam)

    def _speed(self, i, lam):
        h = Fraction(1, 2 ** 30)
        with mpmath.workdps(DPS):
            d = [mpmath.sqrt(_mpf(self._dist2(i, lam + s * h))) for s in (-1, 1)]
            x = step_inverse(self.nc, lam)
            return abs(d[1] - d[0]) / (2 * _mpf(h)) * step_rate(self.nc, x) / _mpf(self.T[i])

    def _build(self):
        if self._ranges is not None:
            return
        ranges, speeds, touches = [], [], []
        with mpmath.workdps(DPS):
            for i in range(len(self.T)):
                ivs, tch = self._segment_intervals(i)
                touches += tch
                for lam_in, lam_out, rin, rout in ivs:
                    t_in, t_out = self._time(i, lam_in), self._time(i, lam_out)
                    for lam, is_root in ((lam_in, rin), (lam_out, rout)):
                        if is_root:
                            speeds.append(self._speed(i, lam))
                    if ranges and ranges[-1][1] == t_in and not rin:      # continues across a knot
                        ranges[-1] = (ranges[-1][0], t_out)
                    else:
                        ranges.append((t_in, t_out))
        self._ranges, self._speeds, self._touches = ranges, speeds, touches

    @property
    def ranges(self):
        self._build()
        return self._ranges

    @property
    def speeds(self):
        self._build()
        return self._speeds

    @property
    def touches(self):
        self._build()
        return self._touches

    # -- sub-ranges
    def _locate(self, t):
        """(segment, line parameter) of the absolute time t (a float or Fraction in [0, W]): msnap_eval_flat's lookup."""
        t = Fraction(t)
        i = next((i for i in range(len(self.T)) if t <= self.K[i + 1]), len(self.T) - 1)
        return i, step(self.nc, (t - self.K[i]) / self.T[i])

    def infimum(self, t0, t1):
        """The exact infimum of the distance over [t0, t1] as mpf (+inf: no finite triangle)."""
        (i0, l0), (i1, l1) = self._locate(t0), self._locate(t1)
        best = None
        for i in range(i0, i1 + 1):
            p = self._at(i, l0) if i == i0 else self.P[i]
            q = self._at(i, l1) if i == i1 else self.P[i + 1]
            lo, hi = [min(p[k], q[k]) for k in range(3)], [max(p[k], q[k]) for k in range(3)]
            for tr, dg in self.tris:
                tb = ([min(v[k] for v in tr) for k in range(3)], [max(v[k] for v in tr) for k in range(3)])
                if best is not None and MF._box_gap2(lo, hi, *tb) > best:
                    continue
                d2 = MF.segment_triangle(p, q, tr, dg)[0]
                best = d2 if best is None or d2 < best else best
        with mpmath.workdps(DPS):
            return mpmath.inf if best is None else mpmath.sqrt(_mpf(best))

    def distance_at(self, t):
        i, lam = self._locate(t)
        with mpmath.workdps(DPS):
            return mpmath.sqrt(_mpf(self._dist2(i, lam))) if self.tris else mpmath.inf

    def assert_transversal(self, min_speed=1e-3, min_gap=1e-6):
        """Every entry and exit at >= min_speed m/s, no touch, and the infimum over the whole flight not within min_gap
        of the threshold: the flight is no graze."""
        assert not self.touches, self.touches
        assert all(s >= min_speed for s in self.speeds), [float(s) for s in self.speeds]
        assert abs(float(self.infimum(0, self.W)) - self.threshold) > min_gap


# ------------------------------------------------------------------------------------------------ exact, any path
class CurvedExact:
    """One drone (coef [M, 4, nc], dur [M]) against tris: the infimum over a sub-range from mesh_clearance_exact's
    candidates -- the range's ends and, per (segment, triangle), the critical points of the seven feature polynomials
    inside it.  A (segment, triangle) whose exact hull distance exceeds a value already attained, or the threshold, is
    skipped: the value returned is the infimum wherever that lies below the threshold, and at least the threshold
    otherwise, which is all the checks ask."""
    ranges = None

    def __init__(self, coef_d, dur_d, tris, threshold, pieces=16):
        self.L = Fraction(float(threshold)) ** 2
        self.coef, self.dur, self.threshold, self.pieces = np.asarray(coef_d), np.asarray(dur_d), float(threshold), pieces
        self.all_tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
        ok, degen = ME.finite_tris(self.all_tris), ME.tri_degenerate(self.all_tris)
        self.K = [0.0] + knots(dur_d)
        self.W = Fraction(self.K[-1])
        self.ftris = {t: [[Fraction(float(x)) for x in v] for v in self.all_tris[t]] for t in range(len(ok)) if ok[t]}
        self.degen = degen

    def distance_at(self, t):
        return ME.exact_distance_at(self.coef, self.dur, self.all_tris, float(t))

    def infimum(self, t0, t1):
        t0, t1 = Fraction(t0), Fraction(t1)
        with mpmath.workdps(DPS):
            mtris = {t: [[_mpf(x) for x in v] for v in tr] for t, tr in self.ftris.items()}
            if not mtris:
                return mpmath.inf
            best = None

            def dist2(i, tau, only=None):
                pt = [mpmath.polyval([mpmath.mpf(float(x)) for x in self.coef[i, ax][::-1]], tau) for ax in range(3)]
                return min(ME.exact_point_tri_dist2(pt, mtris[t], bool(self.degen[t])) for t in (mtris if only is None else only))

            for i in range(len(self.dur)):
                a, b = max(t0, Fraction(self.K[i])), min(t1, Fraction(self.K[i + 1]))
                if a > b:
                    continue
                la, lb = a - Fraction(self.K[i]), b - Fraction(self.K[i])
                for tau in (la, lb):
                    v = dist2(i, _mpf(tau))
                    best = v if best is None or v < best else best
                if lb == la:
                    continue
                p = [[Fraction(float(x)) for x in self.coef[i, ax]] for ax in range(3)]
                ps = [ME._shift(c, la) for c in p]                        # in the time since la
                h = lb - la
                hulls = [ME._control_points(ps, h * j / self.pieces, h * (j + 1) / self.pieces) for j in range(self.pieces)]
                for t, tr in self.ftris.items():
                    n = ME._cross(ME._sub(tr[1], tr[0]), ME._sub(tr[2], tr[0]))
                    bq = min(Fraction(float(best)), self.L) * (1 + Fraction(1, 10 ** 12))
                    if all(ME._piece_tri_gap2(hb, tr, n) > bq for hb in hulls):
                        continue
                    for g in ME._feature_polys(ps, tr):
                        for tau in ME._critical_points(g, _mpf(h)):
                            v = dist2(i, _mpf(la) + tau, only=[t])
                            best = v if v < best else best
            return mpmath.sqrt(max(best, mpmath.mpf(0)))


# ------------------------------------------------------------------------------------------------ fp64 restatement
def _first_crossing(e, h, threshold, t_res, tris, degen, normals, Wt):
    """csrc/msnap_mesh_conflict.hip, first_crossing, for the lanes e [n, 3, D + 1] of lengths h [n]:
    (hit_u, clear_u, nodes)."""
    n, D = len(h), e.shape[2] - 1
    L = threshold * threshold
    Tn = len(tris)
    tmin_box, tmax_box = (tris.min(axis=1), tris.max(axis=1)) if Tn else (None, None)
    hit, clear = np.full(n, np.inf), np.full(n, np.inf)
    idx, lvl, nodes = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    act = np.arange(n)
    while len(act):
        A = len(act)
        hh = np.ldexp(1.0, -lvl[act])
        a = idx[act].astype(np.float64) * hh
        scale = hh[:, None] ** np.arange(D + 1)
        B, P = np.zeros((A, 3, D + 1)), np.zeros((A, 3, 3))
        for s in range(3):
            f = DW._taylor(e[act, s, :], a) * scale
            vm = np.zeros(A)
            for j in range(D, -1, -1):
                vm = vm * 0.5 + f[:, j]
            P[:, 0, s], P[:, 1, s], P[:, 2, s] = f[:, 0], vm, f[:, ::-1].cumsum(axis=1)[:, -1]
            B[:, s, :] = f @ Wt.T
        bound, g = np.full(A, np.inf), np.full((A, 3), np.inf)
        if Tn:
            lo, hi = B.min(axis=2), B.max(axis=2)
            gap = np.maximum(0.0, np.maximum(lo[:, None, :] - tmax_box[None], tmin_box[None] - hi[:, None, :]))
            need = ~((gap * gap).sum(axis=2) >= L)                        # [A, T]
            q, d2 = ME.closest_np(P, tris, degen, normals)                # [A, 3, T, 3], [A, 3, T]
            g = np.where(need[:, None, :], d2, np.inf).min(axis=2)
            fi = np.where(d2[:, 1] > d2[:, 0], np.where(d2[:, 2] > d2[:, 1], 2, 1), np.where(d2[:, 2] > d2[:, 0], 2, 0))
            ai, ti = np.arange(A)[:, None], np.arange(Tn)[None, :]
            dirv = P[ai, fi, :] - q[ai, fi, ti, :]
            ln = np.sqrt((dirv * dirv).sum(axis=2))
            dirv = dirv * np.where(ln > 0, 1.0 / np.where(ln > 0, ln, 1.0), 0.0)[..., None]
            pn = np.einsum("tk,akd->atd", normals, B)
            pa = np.einsum("atk,akd->atd", dirv, B)
            sn = np.einsum("tk,tjk->tj", normals, tris)
            sa = np.einsum("atk,tjk->atj", dirv, tris)
            tb = np.fmax(np.fmax(pn.min(axis=2) - sn.max(axis=1)[None], sn.min(axis=1)[None] - pn.max(axis=2)),
                         pa.min(axis=2) - sa.max(axis=2))
            bound = np.where(need, tb, np.inf).min(axis=1)
        open_ = ~(bound >= threshold)
        at_start = open_ & (g[:, 0] < L)
        leaf = (h[act] * hh <= t_res) | (lvl[act] >= MAX_DEPTH)
        in_mid, at_end = g[:, 1] < L, g[:, 2] < L
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


def mesh_distance_np(pos, all_tris):
    """pos [P, 3] against the whole mesh -> (distance [P], lowest triangle index attaining it [P] int32; +inf, -1
    without a finite triangle), by closest_np."""
    all_tris = np.asarray(all_tris, dtype=np.float64).reshape(-1, 3, 3)
    keep = np.nonzero(ME.finite_tris(all_tris))[0]
    if not len(keep):
        return np.full(len(pos), np.inf), np.full(len(pos), -1, dtype=np.int32)
    tris = all_tris[keep]
    with np.errstate(all="ignore"):
        _, d2 = ME.closest_np(pos, tris, ME.tri_degenerate(tris), ME.unit_normals(tris))
    tri = d2.argmin(axis=1)
    return np.sqrt(d2[np.arange(len(pos)), tri]), keep[tri].astype(np.int32)


def fp64_mesh_conflict_window(coef, dur, tris, threshold, t_res=1e-6, stats=None):
    """coef [N, M, 4, nc], dur [N, M] (valid, finite), tris [T, 3, 3] -> the eight arrays of OUTPUTS by the kernel's
    method in NumPy fp64.  `stats` receives the nodes per lane and direction ("nodes" [N M, 2])."""
    coef, dur = np.asarray(coef, dtype=np.float64), np.asarray(dur, dtype=np.float64)
    all_tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    ftris = all_tris[ME.finite_tris(all_tris)]
    degen, normals = ME.tri_degenerate(ftris), ME.unit_normals(ftris)
    N, M, nc = dur.shape[0], dur.shape[1], coef.shape[3]
    D = nc - 1
    Wt = DW._bernstein_weights(D)
    K = np.add.accumulate(dur, axis=1)
    start = np.concatenate([np.zeros((N, 1)), K[:, :-1]], axis=1).reshape(-1)
    T = dur.reshape(-1)
    E = start + T
    e = coef[:, :, :3, :].reshape(N * M, 3, nc) * (T[:, None] ** np.arange(nc))[:, None, :]
    threshold = float(threshold)
    with np.errstate(all="ignore"):
        hit_f, clear_f, nodes_f = _first_crossing(e, T, threshold, t_res, ftris, degen, normals, Wt)
        back = np.stack([DW._taylor(e[:, s, :], np.ones(N * M)) for s in range(3)], axis=1)      # e_s(1 - u)
        back[:, :, 1::2] *= -1.0
        hit_b, clear_b, nodes_b = _first_crossing(back, T, threshold, t_res, ftris, degen, normals, Wt)
        fwd = lambda u: np.where(np.isfinite(u), np.minimum(T * np.where(np.isfinite(u), u, 0.0) + start, E), np.inf)     # noqa: E731
        bwd = lambda u: np.where(np.isfinite(u), np.maximum(E - T * np.where(np.isfinite(u), u, 0.0), start), -np.inf)    # noqa: E731
        tf, cu = fwd(hit_f).reshape(N, M).min(axis=1), fwd(clear_f).reshape(N, M).min(axis=1)
        tl, cf = bwd(hit_b).reshape(N, M).max(axis=1), bwd(clear_b).reshape(N, M).max(axis=1)
        lo = np.minimum(tf, np.where(tl > -np.inf, tl, np.inf))
        hi = np.maximum(tl, np.where(tf < np.inf, tf, -np.inf))
        tf, tl = lo, hi
        cu, cf = np.minimum(cu, tf), np.maximum(cf, tl)
        found = np.isfinite(tf)
        out = []
        for t in (tf, tl):
            d, tri = mesh_distance_np(DW._positions(coef, dur, np.arange(N), np.where(found, t, 0.0)), all_tris)
            out.append((np.where(found, d, np.inf), np.where(found, tri, -1).astype(np.int32)))
    if stats is not None:
        stats["nodes"] = np.stack([nodes_f, nodes_b], axis=1)
    return cu, tf, out[0][0], out[0][1], tl, out[1][0], out[1][1], cf


class RestatedContext:
    """fp64_mesh_conflict_window, the restated msnap_eval_flat positions and a restated msnap_mesh_sweep of single
    positions behind the Context methods the test bodies use: the CPU tests run the GPU tests' checks on them."""

    def __init__(self, order, max_segments=4096):
        self.order, self.ncoef, self.max_segments = order, order + 1, max_segments

    def mesh_conflict_window(self, coef, dur, tris, threshold, t_res=1e-6):
        out = fp64_mesh_conflict_window(coef, dur, tris, threshold, t_res)
        return out + (np.zeros(len(out[0]), dtype=np.int32),)

    def eval_flat(self, coef, dur, ts):
        coef, dur, ts = np.asarray(coef, dtype=np.float64), np.asarray(dur, dtype=np.float64), np.asarray(ts, dtype=np.float64)
        out = np.zeros((coef.shape[0], len(ts), 13))
        for d in range(coef.shape[0]):
            out[d, :, :3] = DW._positions(coef, dur, np.full(len(ts), d), ts)
        return out

    def mesh_sweep(self, pos, tris, radius):
        pos = np.asarray(pos, dtype=np.float64)
        d = np.stack([mesh_distance_np(pos[:, s, :], tris)[0] for s in range(pos.shape[1])], axis=1).min(axis=1)
        return d, d < radius


# ------------------------------------------------------------------------------------------------ shared test helper
def _attained(ctx, coef, dur, tris, d, t):
    """(msnap_mesh_sweep of the single position msnap_eval_flat gives drone d at t over the whole mesh, the lowest
    triangle index whose own sweep gives the smallest value) -- mesh_clearance_cases.check_attained's rule."""
    out = ctx.eval_flat(coef[d:d + 1], dur[d:d + 1], np.array([t]))
    pos = np.ascontiguousarray(out[:, :, :3])
    whole = ctx.mesh_sweep(pos, tris, 0.1)[0][0]
    each = np.array([ctx.mesh_sweep(pos, tris[k:k + 1], 0.1)[0][0] for k in range(len(tris))])
    each = np.where(np.isfinite(each), each, np.inf)                      # (a non-finite triangle alone: nothing)
    return whole, int(np.argmin(each)), each


def check_mesh_windows(ctx, coef, dur, tris, threshold, exact, t_res=1e-6, closing=True, verdict=None, restated=None):
    """msnap_mesh_conflict_window through `ctx` (a Context or RestatedContext) against the exact reference `exact` (per
    drone a StraightExact or CurvedExact), per drone:
      1. the exact infimum over [0, t_clear_until] and over [t_clear_from, W] is >= threshold - r;
      2. the exact distance at t_first and at t_last is < threshold + r;
      3. mesh_sweep of eval_flat at those times equals d_first / d_last bit for bit, and tri_* is the lowest index
         attaining it;
      4. closing: t_first - t_clear_until <= t_res + 2 ulp(W), t_clear_from - t_last likewise; a conflict is found
         exactly when the reference has one; t_first and t_last lie within t_res + 2 ulp(W) + 2 r / speed of the exact
         first entry and last exit;
      5. 0 <= t_clear_until <= t_first <= t_last <= t_clear_from <= W where finite.
    verdict: per drone "clear", "conflict" or None.  restated: the restatement's eight arrays -- the four times of
    `ctx` lie within t_res + 2 ulp(W) of them.  Prints each drone's figures; returns the outputs."""
    tris = np.ascontiguousarray(tris, dtype=np.float64)
    out = ctx.mesh_conflict_window(coef, dur, tris, threshold, t_res)
    cu, tf, df, wf, tl, dl, wl, cf, status = out
    assert (status == 0).all(), status
    for d in range(len(cu)):
        ex = exact[d]
        W = knots(dur[d])[-1]
        r = allowance(coef[d], dur[d], tris)
        tol = t_res + 2 * ulp(W)
        print(f"drone {d} W {W!r}: clear until {cu[d]!r} first {tf[d]!r} ({df[d]!r} m, tri {wf[d]}) last {tl[d]!r} "
              f"({dl[d]!r} m, tri {wl[d]}) clear from {cf[d]!r} r {r:.3g}"
              + ("" if ex.ranges is None else f" exact ranges {[(float(x), float(y)) for x, y in ex.ranges]}"))
        # 5. order
        chain = [0.0] + [x for x in (cu[d], tf[d], tl[d], cf[d]) if np.isfinite(x)] + [W]
        assert all(x <= y for x, y in zip(chain[:-1], chain[1:])), (d, chain)
        assert np.isfinite(tf[d]) == np.isfinite(tl[d]) == np.isfinite(df[d]) == np.isfinite(dl[d]) == (wf[d] >= 0) == (wl[d] >= 0)
        if np.isfinite(tf[d]):
            assert np.isfinite(cu[d]) and np.isfinite(cf[d])
        # 1. the proven ranges (half open: in conflict at 0, [0, t_clear_until) is empty; likewise at W)
        if not np.isfinite(cu[d]):
            assert float(ex.infimum(0, Fraction(W))) >= threshold - r, (d, "certified clear")
            assert tuple(x[d] for x in out[:8]) == CLEAR, d
        elif not (cu[d] == tf[d] == 0.0):
            assert float(ex.infimum(0, Fraction(float(cu[d])))) >= threshold - r, (d, "clear until")
        if np.isfinite(cf[d]) and not (cf[d] == tl[d] == W):
            assert float(ex.infimum(Fraction(float(cf[d])), Fraction(W))) >= threshold - r, (d, "clear from")
        # 2., 3. the conflicts found
        for t, dist, tri in ((tf[d], df[d], wf[d]), (tl[d], dl[d], wl[d])):
            if not np.isfinite(t):
                continue
            assert float(ex.distance_at(float(t))) < threshold + r, (d, t)
            whole, lowest, each = _attained(ctx, coef, dur, tris, d, float(t))
            assert whole == dist, (d, t, whole, dist)
            assert tri == lowest and each[tri] == dist, (d, t, tri, lowest)
        # 4. the search closes on a transversal fixture
        if closing:
            ranges, speeds = ex.ranges, ex.speeds
            assert bool(ranges) == bool(np.isfinite(tf[d])), (d, ranges, tf[d])
            if ranges:
                assert tf[d] - cu[d] <= tol and cf[d] - tl[d] <= tol, (d, tf[d] - cu[d], cf[d] - tl[d])
                slack = tol + (2 * r / float(min(speeds)) if speeds else 0.0)
                assert abs(tf[d] - float(ranges[0][0])) <= slack and abs(float(ranges[-1][1]) - tl[d]) <= slack, d
            else:
                assert cu[d] == np.inf and cf[d] == -np.inf, (d, "not certified clear")
        if verdict is not None and verdict[d] == "clear":
            assert tuple(x[d] for x in out[:8]) == CLEAR, d
        if verdict is not None and verdict[d] == "conflict":
            assert np.isfinite(tf[d]) and np.isfinite(tl[d]), d
        if restated is not None:
            for k in TIMES:
                assert out[k][d] == restated[k][d] or abs(out[k][d] - restated[k][d]) <= tol, (d, OUTPUTS[k], out[k][d], restated[k][d])
    return out
