"""Inputs and test bodies of the mesh conflict-window tests (tests/test_mesh_conflict_window_cpu.py on the NumPy
restatement, tests/test_mesh_conflict_window_gpu.py on the kernel).  A fixture of the closing checks is a list of groups
(nc, points [N, M + 1, 3], durs [N, M], tris, threshold): straight polyline flights on a dyadic lattice with durations
that are powers of two (tests/mesh_flight_exact.py), one entry call per group; tests/test_mesh_conflict_window_cpu.py
proves every one of them transversal."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import mesh_clearance_cases as MC
import mesh_conflict_exact as MX
import mesh_flight_exact as MF

WALL = MC.ONE_TRI                   # the plane x = 0.25
WALL_THRESHOLD = 0.1
HOLE_THRESHOLD = MC.CERTIFY_RADIUS
MARGINS = (2.0 ** -2, 2.0 ** -3, 2.0 ** -4, 2.0 ** -6, 2.0 ** -8, 2.0 ** -10)      # the dyadic margins tried on top of a flight's exact D
FEATURE_LINES = ("o7_tri0", "o7_tri1", "o7_tri2", "o7_tri3", "o7_fan", "o7_ridge", "o9_tri0", "o9_fan")


def _group(nc, points, durs, tris, threshold):
    points = np.asarray(points, dtype=np.float64)
    points = points[None] if points.ndim == 2 else points
    durs = np.asarray(durs, dtype=np.float64).reshape(len(points), -1)
    return nc, points, durs, np.asarray(tris, dtype=np.float64), float(threshold)


def wall(nc):
    """The issue's trial: the straight flight through the wall x = 0.25, entry at the root of s(x) = 0.575."""
    return [_group(nc, [(-1, .25, .25), (1, .25, .25)], [1.0], WALL, WALL_THRESHOLD)]


def hole_scene():
    """Through the wall of env-scene-hole.stl at x = 2.5 (the wall is hollow: 0.5 m between its faces, so the flight
    is in conflict twice), and two flights that stay clear: through the hole's centre and past the wall."""
    pts = [[(x, -2.25, .25), (x, 2.25, .25)] for x in (2.5, 0.0, 5.0)]
    return [_group(8, pts, np.ones((3, 1)), MC.scene("hole"), HOLE_THRESHOLD)]


def _feature_threshold(nc, points, tris):
    """(threshold, StraightExact) for one feature flight: its exact D rounded to fp64 plus the first dyadic margin with
    which the first entry falls at a line parameter in [0.1, 0.9], the flight is transversal, and no entry or exit falls
    on a boundary of the walk's dyadic subdivision (s(1/2) = 1/2, and these flights come from a lattice: an exit at
    exactly t = 1/2 has the distance EQUAL to the threshold at a node's end, which a last-bit comparison decides)."""
    D = float(MF.exact_polyline_clearance(points, tris)[0])
    for m in MARGINS:
        ex = MX.StraightExact(points, [1.0], nc, tris, D + m)
        ivs, touches = ex._segment_intervals(0)
        if ivs and not touches and Fraction(1, 10) <= ivs[0][0] <= Fraction(9, 10):
            ends = [float(t) * 2.0 ** 32 for r in ex.ranges for t in r if 0 < t < 1]
            if all(abs(y - round(y)) > 1e-6 for y in ends):
                return D + m, ex
    raise AssertionError(("no margin fits", points))


def features(name):
    """Every flight of mesh_clearance_cases.features_line(name) -- the closest feature a vertex, an edge, the face, a
    crossing -- each with a threshold of its own: the entry is a root of a different feature polynomial."""
    line = MC.features_line(name)
    out, exact = [], []
    for p in line["points"]:
        thr, ex = _feature_threshold(line["nc"], p, line["tris"])
        out.append(_group(line["nc"], p, [1.0], line["tris"], thr))
        exact.append([ex])
    return out, exact


def knot():
    """Three segments, in conflict across a knot: one polyline comes to rest 0.0625 m in front of the wall and leaves
    along it, one comes to rest on the wall itself."""
    pts = [[(-.5, .25, .25), (.1875, .25, .25), (.1875, .5, .25), (-1, .5, .5)],
           [(-1, .25, .25), (.25, .25, .25), (1, .5, .25), (1, 1, 1)]]
    return [_group(8, pts, [[1.0, 0.5, 1.0], [1.0, 1.0, 0.5]], WALL, WALL_THRESHOLD)]


def both_ends():
    """The path starts and ends inside the margin: the whole flight in conflict, and out of the margin and back."""
    return [_group(8, [(.1875, .25, .25), (.3125, .5, .25)], [1.0], WALL, WALL_THRESHOLD),
            _group(8, [(.1875, .25, .25), (-.5, .25, .25), (.1875, .5, .5)], [1.0, 0.5], WALL, WALL_THRESHOLD)]


def two_conflicts():
    """Out through the wall and back: t_first comes from the first conflict, t_last from the second."""
    return [_group(8, [(-1, .25, .25), (1, .25, .25), (-1, .5, .5)], [1.0, 2.0], WALL, WALL_THRESHOLD)]


def far():
    """The wall flight with path and mesh moved by mesh_clearance_cases' FAR offsets, +1e5 m among them."""
    out = []
    for off in sorted({o for _, o in MC.FAR.values()}):
        base = dict(points=np.array([[(-1, .25, .25), (1, .25, .25)]]), tris=WALL)
        moved = MC._moved(base, "far", off)
        out.append(_group(8, moved["points"], [1.0], moved["tris"], WALL_THRESHOLD))
    return out


def odd_mesh():
    """A NaN triangle, the wall twice, and a zero-area triangle far away in one mesh: the lowest index of the duplicate
    is reported, the NaN one is ignored."""
    tris = np.concatenate([np.full((1, 3, 3), np.nan), WALL, WALL, [[[3, 3, 3], [4, 4, 4], [5, 5, 5]]]])
    return [_group(8, [(-1, .25, .25), (1, .25, .25)], [1.0], tris, WALL_THRESHOLD)]


CLOSING = {"wall_o7": lambda: wall(8), "wall_o9": lambda: wall(10), "hole": hole_scene, "knot": knot,
           "both_ends": both_ends, "two_conflicts": two_conflicts, "far": far, "odd_mesh": odd_mesh}
CLOSING.update({f"features_{n}": (lambda n=n: features(n)) for n in FEATURE_LINES})
_MEMO = {}


def fixture(name):
    """(groups, exact): exact[g][d] the StraightExact of drone d of group g -- built once per session."""
    if name not in _MEMO:
        made = CLOSING[name]()
        groups, exact = made if isinstance(made, tuple) else (made, None)
        if exact is None:
            exact = [[MX.StraightExact(p, t, nc, tris, thr) for p, t in zip(points, durs)]
                     for nc, points, durs, tris, thr in groups]
        _MEMO[name] = (groups, exact)
    return _MEMO[name]


def paths(group):
    nc, points, durs, tris, thr = group
    both = [MF.path(p, t, nc) for p, t in zip(points, durs)]
    return np.stack([c for c, _ in both]), np.stack([t for _, t in both])


def run(ctx, name, t_res=1e-6, restated=False, **kw):
    """The fixture's groups through check_mesh_windows; restated: also the agreement of the four times with the
    restatement.  `ctx` must be of the fixture's order.  Returns [(group, outputs)]."""
    groups, exact = fixture(name)
    res = []
    for g, ex in zip(groups, exact):
        assert g[0] == ctx.ncoef, (name, g[0])
        coef, dur = paths(g)
        ref = MX.fp64_mesh_conflict_window(coef, dur, g[3], g[4], t_res) if restated else None
        res.append((g, MX.check_mesh_windows(ctx, coef, dur, g[3], g[4], ex, t_res, restated=ref, **kw)))
    return res


# ---------------------------------------------------------------------------------------------------- test bodies
def check_wall(ctx, nc, **kw):
    (_, out), = run(ctx, f"wall_o{nc - 1}", verdict=["conflict"], **kw)
    if nc == 8:            # the root of s(x) = 0.575
        assert abs(out[1][0] - 0.534448773) <= 1e-6 and out[3][0] == 0 and out[6][0] == 0


def check_hole(ctx, **kw):
    (_, out), = run(ctx, "hole", verdict=["conflict", "clear", "clear"], **kw)
    assert out[1][0] < 0.5 < out[4][0]                 # the first conflict in the front face, the last in the back face


def check_features(ctx, name, **kw):
    for _, out in run(ctx, f"features_{name}", **kw):
        assert np.isfinite(out[1]).all()


def check_knot(ctx, **kw):
    (g, out), = run(ctx, "knot", verdict=["conflict"] * 2, **kw)
    K = np.add.accumulate(g[2], axis=1)
    assert (out[1] < K[:, 0]).all() and (out[4] > K[:, 0]).all()      # one conflict, entered before the knot, left after
    assert out[4][0] > K[0, 1]                                          # (the first polyline stays inside over a whole segment)


def check_both_ends(ctx, **kw):
    for g, out in run(ctx, "both_ends", verdict=["conflict"], **kw):
        W = float(g[2].sum())
        assert (out[0][0], out[1][0], out[4][0], out[7][0]) == (0.0, 0.0, W, W)


def check_two_conflicts(ctx, **kw):
    (g, out), = run(ctx, "two_conflicts", verdict=["conflict"], **kw)
    ranges = fixture("two_conflicts")[1][0][0].ranges
    assert len(ranges) == 2 and out[1][0] < 1.0 < out[4][0]
    assert float(ranges[0][0]) - 2e-6 <= out[1][0] <= float(ranges[0][1])      # t_first from the first conflict,
    assert float(ranges[1][0]) <= out[4][0] <= float(ranges[1][1]) + 2e-6      # t_last from the second


def check_far(ctx, **kw):
    for _, out in run(ctx, "far", verdict=["conflict"], **kw):
        assert abs(out[1][0] - 0.534448773) <= 1e-6 + 1e-8


def check_odd_mesh(ctx, **kw):
    (_, out), = run(ctx, "odd_mesh", verdict=["conflict"], **kw)
    assert out[3][0] == 1 and out[6][0] == 1


def check_t_res(ctx, **kw):
    """The closing gap follows t_res."""
    for t_res in (1e-3, 1e-6, 1e-9):
        (g, out), = run(ctx, "wall_o7", t_res=t_res, **kw)
        assert out[1][0] - out[0][0] <= t_res + 2 * MX.ulp(1.0) and out[7][0] - out[4][0] <= t_res + 2 * MX.ulp(1.0)
        assert abs(out[1][0] - 0.534448773) <= t_res + 1e-9


# -- verdict cases without closing checks
def never_close():
    pts = [[(-1, 4.0, .25), (1, 4.5, .25), (1, 5.0, 1.0)], [(2, .25, .25), (3, .25, .5), (2, 1.0, .25)]]
    return _group(8, pts, [[1.0, 0.5], [0.5, 1.0]], WALL, WALL_THRESHOLD)


def check_never_close(ctx):
    g = never_close()
    coef, dur = paths(g)
    out = ctx.mesh_conflict_window(coef, dur, g[3], g[4])
    assert all(tuple(x[d] for x in out[:8]) == MX.CLEAR for d in range(2)) and (out[8] == 0).all()
    stats = {}
    MX.fp64_mesh_conflict_window(coef, dur, g[3], g[4], stats=stats)
    assert (stats["nodes"] == 1).all()                                  # certified clear in one node per lane


def check_tangent(ctx):
    """Drone 11 of certify_case flies at exactly CERTIFY_RADIUS from triangle 2: no conflict is found."""
    coef, dur, tris = MC.certify_case()
    out = ctx.mesh_conflict_window(coef[11:12], dur[11:12], tris, MC.CERTIFY_RADIUS)
    assert out[1][0] == np.inf and out[4][0] == -np.inf and out[3][0] == -1 and out[6][0] == -1 and out[8][0] == 0
    assert out[2][0] == np.inf and out[5][0] == np.inf
    if np.isfinite(out[0][0]):                                          # undecided: the proven ranges are in order
        assert 0.0 <= out[0][0] <= out[7][0] <= float(dur[11].sum())


def check_threshold_zero(ctx):
    g = wall(8)[0]
    coef, dur = paths(g)
    out = ctx.mesh_conflict_window(coef, dur, g[3], 0.0)
    assert tuple(x[0] for x in out[:8]) == MX.CLEAR and out[8][0] == 0


def check_no_triangles(ctx):
    g = wall(8)[0]
    coef, dur = paths(g)
    for tris in (np.zeros((0, 3, 3)), np.full((2, 3, 3), np.nan)):
        out = ctx.mesh_conflict_window(coef, dur, tris, 0.5)
        assert tuple(x[0] for x in out[:8]) == MX.CLEAR and out[8][0] == 0


# -- curved paths: name -> (mesh_clearance_cases.CURVED's case, drones, threshold)
CURVED = {"m1": ("o9_m1", (0, 5), 1.0), "m3": ("o7_m3", (0, 1), 0.5), "m10": ("o9_m10", (0, 1), 0.5)}


def curved(name):
    case, drones, thr = CURVED[name]
    if ("curved", name) not in _MEMO:
        coef, dur, tris = MC.curved_case(case)
        coef, dur = np.ascontiguousarray(coef[list(drones)]), np.ascontiguousarray(dur[list(drones)])
        _MEMO["curved", name] = (coef, dur, tris, thr, [MX.CurvedExact(c, t, tris, thr) for c, t in zip(coef, dur)])
    return _MEMO["curved", name]


def check_curved(ctx, name, restated=False):
    """Checks 1 to 3 and 5 on solved paths against the closed box."""
    coef, dur, tris, thr, exact = curved(name)
    assert coef.shape[3] == ctx.ncoef
    ref = MX.fp64_mesh_conflict_window(coef, dur, tris, thr) if restated else None
    out = MX.check_mesh_windows(ctx, coef, dur, tris, thr, exact, closing=False, restated=ref)
    assert np.isfinite(out[1]).any()
    return out


# -- bit identity: 87 drones x 3 segments = 261 lanes, more than one 256-thread block
def identity_batch():
    if "identity" not in _MEMO:
        line = MC.random_flights(8, 87, 3, 23001)
        coef, dur, tris = MC.line_paths(line)
        _MEMO["identity"] = (coef, dur, tris, 0.5)
    return _MEMO["identity"]


def same(x, y):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y))


def check_identities(ctx):
    """Whole batch, each drone alone, a permuted batch, an empty batch: the same bits.  Returns the whole batch's
    outputs."""
    coef, dur, tris, thr = identity_batch()
    ref = ctx.mesh_conflict_window(coef, dur, tris, thr)
    assert (ref[8] == 0).all() and np.isfinite(ref[1]).any() and not np.isfinite(ref[1]).all()
    for d in range(0, len(dur), 7):
        one = ctx.mesh_conflict_window(coef[d:d + 1], dur[d:d + 1], tris, thr)
        assert same(one, [x[d:d + 1] for x in ref]), d
    perm = np.random.default_rng(9).permutation(len(dur))
    got = ctx.mesh_conflict_window(coef[perm], dur[perm], tris, thr)
    assert same(got, [x[perm] for x in ref])
    empty = ctx.mesh_conflict_window(coef[:0], dur[:0], tris, thr)
    assert all(x.shape == (0,) for x in empty)
    return ref


# -- swarm.mesh_conflict_windows / latest_replan_time on certify_case
TUNNELLING = (5, 6, 7, 8)            # certify_case's drones at x = 2.5, -2.5, 3.0, 1.8: through the wall, away from the hole


def check_swarm_windows(res, t_replan, coef, dur, margin):
    """A MeshConflictWindowResult of certify_case: the tunnelling drones get finite windows inside the wall's exact
    range -- |y| < 0.25 + radius, y the flight's own fp64 polynomial -- and the others no conflict."""
    n = lambda x: np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x)      # noqa: E731
    cu, tf, tl, cf, first, t_r = (n(x) for x in (res.t_clear_until, res.t_first, res.t_last, res.t_clear_from,
                                                  res.first_conflict, t_replan))
    assert set(TUNNELLING) <= set(n(res.idx).tolist())
    reach = 0.25 + MC.CERTIFY_RADIUS

    def y_at(d, t):
        return float(np.polyval(coef[d, 0, 1, ::-1], t))

    for d in range(len(dur)):
        if d in TUNNELLING:
            assert np.isfinite([cu[d], tf[d], tl[d], cf[d]]).all() and first[d] == cu[d], d
            assert cu[d] <= tf[d] <= cu[d] + 2e-6 and tl[d] <= cf[d] <= tl[d] + 2e-6, d
            # inside the wall's range, and its ends within the resolution (the flight moves at about 8 m/s there)
            assert -reach <= y_at(d, tf[d]) < -reach + 1e-4 and reach - 1e-4 < y_at(d, tl[d]) <= reach, d
            assert y_at(d, cu[d]) <= -reach + 1e-9 and y_at(d, cf[d]) >= reach - 1e-9, d
            assert t_r[d] == max(cu[d] - margin, 0.0), d
        else:
            assert tf[d] == np.inf and tl[d] == -np.inf and (first[d] == np.inf or first[d] == cu[d]), d
            assert t_r[d] == (np.inf if first[d] == np.inf else max(first[d] - margin, 0.0)), d
