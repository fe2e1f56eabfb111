"""Inputs and shared checks of the half-space window tests (tests/test_halfspace_window_cpu.py on the restatement,
tests/test_halfspace_window_gpu.py on the kernel) and of tools/halfspace_window_rounding.py: hand-built polynomials whose
exits and re-entries are known, the overshoot of the reference planner's workspace, solved swarms near and far from the
origin with 1, 3, 10 and 49 segments, the three-box corridor, and the list of the bit identities."""
from __future__ import annotations

import functools

import numpy as np

import extent_cases as EC
import extent_exact as XE
import halfspace_exact as HE

T_RES = (1e-3, 1e-6, 1e-9)
X_LE = lambda b: np.array([[1.0, 0.0, 0.0, b]])      # noqa: E731


def parabola(order):
    """one segment x = 4 t (1 - t) on T = 1 (y = x / 2, z = 1): x > 3/4 exactly on (1/4, 3/4), x = 1 at t = 1/2"""
    return EC._poly(order, [[0.0, 4.0, -4.0]]), np.array([[1.0]])


def two_humps(order):
    """two such segments: x > 3/4 on (1/4, 3/4) and on (5/4, 7/4)"""
    return EC._poly(order, [[0.0, 4.0, -4.0], [0.0, 4.0, -4.0]]), np.array([[1.0, 1.0]])


def valley(order):
    """x = 1 - 4 t (1 - t): x > 3/4 on [0, (1 - sqrt(3)/2) / 2) and on ((1 + sqrt(3)/2) / 2, 1] -- outside at both ends"""
    return EC._poly(order, [[1.0, -4.0, 4.0]]), np.array([[1.0]])


def run(ctx, coef, dur, planes, queries, t_res=1e-6, restated=False, **kw):
    ref = None
    if restated:
        ref = HE.fp64_halfspace_window(coef, dur, planes, queries, t_res, kw.get("t_from"), kw.get("t_to"))
    return HE.check_windows(ctx, coef, dur, planes, queries, t_res, restated=ref, **kw)


Q00 = np.array([[0, 0]], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ hand-built cases
def check_parabola(ctx, order, **kw):
    coef, dur = parabola(order)
    iu, tf, vf, tl, vl, ifr, _ = run(ctx, coef, dur, X_LE(0.75), Q00, verdict=["outside"], **kw)
    for got, want in ((iu[0], 0.25), (tf[0], 0.25), (tl[0], 0.75), (ifr[0], 0.75)):
        assert abs(got - want) <= 1e-6, (got, want)
    assert vf[0] > 0.75 and vl[0] > 0.75


def check_tangency(ctx, **kw):
    """x <= 1 is touched at t = 1/2 and never crossed: nothing is found outside; undecided or certified"""
    coef, dur = parabola(7)
    iu, tf, vf, tl, vl, ifr, _ = run(ctx, coef, dur, X_LE(1.0), Q00, closing=False, **kw)
    assert tf[0] == np.inf and tl[0] == -np.inf and vf[0] == -np.inf and vl[0] == -np.inf
    assert (iu[0] == np.inf and ifr[0] == -np.inf) or abs(iu[0] - 0.5) <= 2e-6


@functools.lru_cache(maxsize=None)
def overshoot(order):
    coef, dur = EC.solve(*EC.overshoot_waypoints(), order + 1)
    return coef, dur


def overshoot_swarm(scales, order=7):
    """the overshoot waypoints drawn towards (0, 3.9, 1.5) by each scale: the larger ones leave the workspace"""
    wp, t = EC.overshoot_waypoints()
    centre = np.array([0.0, 3.9, 1.5, 0.0])
    wps = np.concatenate([centre + s * (wp - centre) for s in scales])
    return EC.solve(wps, np.tile(t, (len(scales), 1)), order + 1)


def check_overshoot(ctx, order, **kw):
    """the reference planner's four waypoints inside the workspace: the fit leaves x <= 2.2 around t = 3.0"""
    coef, dur = overshoot(order)
    iu, tf, vf, tl, vl, ifr, _ = run(ctx, coef, dur, X_LE(EC.BOX_HI[0]), Q00, verdict=["outside"], **kw)
    assert iu[0] <= tf[0] < 3.0 < tl[0] <= ifr[0]
    return tf[0], tl[0]


def check_two_conflicts(ctx, **kw):
    coef, dur = two_humps(7)
    iu, tf, vf, tl, vl, ifr, _ = run(ctx, coef, dur, X_LE(0.75), Q00, verdict=["outside"], **kw)
    assert abs(tf[0] - 0.25) <= 1e-6 and abs(tl[0] - 1.75) <= 1e-6      # the first and the last


def check_ends(ctx, **kw):
    coef, dur = valley(7)
    iu, tf, vf, tl, vl, ifr, _ = run(ctx, coef, dur, X_LE(0.75), Q00, verdict=["outside"], **kw)
    assert iu[0] == tf[0] == 0.0 and tl[0] == ifr[0] == 1.0 and vf[0] == 1.0 and vl[0] == 1.0


def check_ranges(ctx, **kw):
    coef, dur = parabola(7)
    q4 = np.zeros((4, 2), dtype=np.int32)
    #                 begins inside the violation, W < S, W == S inside, W == S outside
    t_from, t_to = np.array([0.5, 0.8, 0.1, 0.5]), np.array([1.0, 0.3, 0.1, 0.5])
    iu, tf, vf, tl, vl, ifr, _ = run(ctx, coef, dur, X_LE(0.75), q4, t_from=t_from, t_to=t_to,
                                     verdict=["outside", "inside", "inside", "outside"], **kw)
    assert iu[0] == tf[0] == 0.5 and abs(tl[0] - 0.75) <= 1e-6
    assert (iu[3], tf[3], tl[3], ifr[3]) == (0.5, 0.5, 0.5, 0.5) and vf[3] == vl[3] == 1.0
    # a range that reaches past the flight on both sides is the whole flight
    whole = ctx.halfspace_window(coef, dur, X_LE(0.75), Q00, 1e-6)
    wide = ctx.halfspace_window(coef, dur, X_LE(0.75), Q00, 1e-6, t_from=np.array([-3.0]), t_to=np.array([7.0]))
    assert same(whole, wide)


def check_partial_segments(ctx, **kw):
    coef, dur = two_humps(7)
    q2 = np.zeros((2, 2), dtype=np.int32)
    #                 strictly inside segment 1; ends on the knot
    t_from, t_to = np.array([1.1, 0.5]), np.array([1.6, 1.0])
    iu, tf, vf, tl, vl, ifr, _ = run(ctx, coef, dur, X_LE(0.75), q2, t_from=t_from, t_to=t_to,
                                     verdict=["outside", "outside"], **kw)
    assert abs(tf[0] - 1.25) <= 1e-6 and tl[0] == ifr[0] == 1.6
    assert iu[1] == tf[1] == 0.5 and abs(tl[1] - 0.75) <= 1e-6 and ifr[1] <= 1.0


def check_planes(ctx, **kw):
    coef, dur = parabola(7)
    planes = np.array([[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, -1.0], [0.0, 0.0, 0.0, 0.0], [1.0, np.nan, 0.0, 0.75],
                       [1.0, 0.0, 0.0, np.inf], [2.0, 0.0, 0.0, 1.5], [1.0, 0.0, 0.0, 0.75]])
    queries = np.stack([np.zeros(7), np.arange(7)], axis=1).astype(np.int32)
    iu, tf, vf, tl, vl, ifr, st = ctx.halfspace_window(coef, dur, planes, queries, 1e-6)
    assert (st == 0).all()
    inside = (np.inf, np.inf, -np.inf, -np.inf, -np.inf, -np.inf)
    assert (iu[0], tf[0], vf[0], tl[0], vl[0], ifr[0]) == inside             # zero normal, 0 <= b
    assert (iu[2], tf[2], vf[2], tl[2], vl[2], ifr[2]) == inside             # 0 <= 0
    assert (iu[1], tf[1], tl[1], ifr[1]) == (0.0, 0.0, 1.0, 1.0) and vf[1] == 0.0 and vl[1] == 0.0      # b < 0: outside throughout
    for k in (3, 4):
        assert all(np.isnan(x[k]) for x in (iu, tf, vf, tl, vl, ifr))
    # a non-unit normal: (2 n, 2 b) is the same half-space; doubling is exact, so the times are the same bits
    assert (iu[5], tf[5], tl[5], ifr[5]) == (iu[6], tf[6], tl[6], ifr[6]) and vf[5] == 2.0 * vf[6]
    run(ctx, coef, dur, planes[5:7], np.array([[0, 0], [0, 1]], dtype=np.int32), verdict=["outside"] * 2, **kw)


def check_t_res(ctx, **kw):
    """The closing gap follows t_res (check 4 at each), and a finer resolution moves the bracket inwards.  The limit
    0.7 puts the crossings off the dyadic grid."""
    coef, dur = parabola(7)
    gaps = []
    for t_res in T_RES:
        iu, tf, vf, tl, vl, ifr, _ = run(ctx, coef, dur, X_LE(0.7), Q00, t_res=t_res, **kw)
        gaps.append(max(tf[0] - iu[0], ifr[0] - tl[0]))
    print("closing gaps:", gaps)
    assert gaps[0] > 1e-6 >= gaps[1] > 1e-9 and gaps[2] <= 1.01e-9


# ------------------------------------------------------------------------------------------------ solved swarms
# name -> (extent_cases swarm, the drones that get a query): M of 1, 3, 10 and 49, near the origin and 1e5 m from it
SWARMS = {
    "m1": ("near_n1_m1_k1", [0]), "m3": ("near_n5_m3_k7", [0, 2, 4]), "m10": ("near_n5_m10_k6", [1, 3]),
    "m49": ("long_n2_m49_k7", [1]), "far_1e5_m3": ("far_1e5_n5_m3_k7", [0, 1, 2, 3, 4]),
    "far_1e5_m10": ("far_1e5_n1_m10_k6", [0]),
}
_MEMO = {}


def midreach_planes(coef, dur, drones, dirs):
    """(planes, queries): per listed drone and direction n of `dirs` the half-space n.x <= b with b half way between
    the path's least and largest reach in that direction, [-ext(-n), ext(n)]: the path attains both, so it crosses b"""
    ext, _, _ = XE.fp64_extent(coef, dur, np.concatenate([dirs, -dirs]))
    planes, queries = [], []
    for d in drones:
        for k, n in enumerate(dirs):
            planes.append([*n, 0.5 * (ext[d, k] - ext[d, k + len(dirs)])])
            queries.append((d, len(planes) - 1))
    return np.array(planes), np.array(queries, dtype=np.int32)


def swarm_fixture(name, order):
    """(coef, dur, planes, queries, exact_of): per listed drone two half-spaces, +x and -y, whose limit lies half way
    between the path's least and largest reach in that direction -- the path attains both, so it crosses the limit; that
    every crossing is transversal the CPU test asserts."""
    key = (name, order)
    if key not in _MEMO:
        base, drones = SWARMS[name]
        coef, dur, _ = EC.swarm_case(base, order)
        planes, queries = midreach_planes(coef, dur, drones, np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]))
        _MEMO[key] = (coef, dur, planes, queries, HE.exact_of(coef, dur, planes, queries))
    return _MEMO[key]


def check_swarm(ctx, name, order, **kw):
    coef, dur, planes, queries, exact = swarm_fixture(name, order)
    return run(ctx, coef, dur, planes, queries, exact=exact, **kw)


# ------------------------------------------------------------------------------------------------ identities
def same(x, y):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y))


@functools.lru_cache(maxsize=None)
def identity_case():
    """65 drones x 10 segments against 7 planes (lane counts 63, 64, 65 queries x 10 around whole waves; 455 queries):
    the six axes at each coordinate's median reach over the swarm, and one oblique plane."""
    coef, dur, dirs = EC.swarm_case("near_n65_m10_k7", 7)
    ext, _, _ = XE.fp64_extent(coef, dur, dirs)
    planes = np.concatenate([dirs, np.median(ext, axis=0)[:, None]], axis=1)
    queries = np.stack(np.meshgrid(np.arange(65), np.arange(7), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32)
    return coef, dur, planes, queries


def check_identities(ctx):
    """Place in the list and the list's length; the planes permuted; the drone alone in a batch of 1; NULL against
    explicit t_from / t_to.  Returns the reference outputs."""
    coef, dur, planes, queries = identity_case()
    ref = ctx.halfspace_window(coef, dur, planes, queries, 1e-6)
    assert (ref[6] == 0).all() and np.isfinite(ref[1]).any() and not np.isfinite(ref[1]).all()
    rng = np.random.default_rng(20)
    perm = rng.permutation(len(queries))
    assert same([x[perm] for x in ref], ctx.halfspace_window(coef, dur, planes, queries[perm], 1e-6))
    for cnt in (63 * 1, 64, 65, 1):      # (x 10 segments: lanes 630, 640, 650 around whole waves)
        assert same([x[perm[:cnt]] for x in ref], ctx.halfspace_window(coef, dur, planes, queries[perm[:cnt]], 1e-6))
    pp = rng.permutation(7)              # planes[pp][k] = planes[pp[k]]: plane j now sits at inv[j]
    inv = np.argsort(pp)
    moved = np.stack([queries[:, 0], inv[queries[:, 1]]], axis=1).astype(np.int32)
    assert same(ref, ctx.halfspace_window(coef, dur, planes[pp], moved, 1e-6))
    more = np.concatenate([np.full((3, 4), 0.5), planes])      # n_planes and the plane's place
    shifted = queries + np.array([0, 3], dtype=np.int32)
    assert same(ref, ctx.halfspace_window(coef, dur, more, shifted, 1e-6))
    for d in (0, 31, 64):                # alone in a batch of 1
        take = queries[:, 0] == d
        alone = np.stack([np.zeros(7), queries[take, 1]], axis=1).astype(np.int32)
        assert same([x[take] for x in ref], ctx.halfspace_window(coef[d:d + 1], dur[d:d + 1], planes, alone, 1e-6))
    total = np.add.accumulate(dur, axis=1)[:, -1]
    assert same(ref, ctx.halfspace_window(coef, dur, planes, queries, 1e-6, t_from=np.zeros(len(queries)),
                                          t_to=total[queries[:, 0]]))
    assert same(ref, ctx.halfspace_window(coef, dur, planes, queries, 1e-6, t_from=np.zeros(len(queries))))
    return ref


# ------------------------------------------------------------------------------------------------ three boxes, a chain
def boxes(*lo_hi):
    """planes [6 B, 4] and poly_offsets [B + 1] of axis-aligned boxes (lo [3], hi [3])"""
    planes = []
    for lo, hi in lo_hi:
        for a in range(3):
            e = np.zeros(3)
            e[a] = 1.0
            planes.append([*e, hi[a]])
            planes.append([*(-e), -lo[a]])
    return np.array(planes), np.arange(len(lo_hi) + 1) * 6


# three overlapping boxes along x: [0, 4], [3, 7], [6, 10], each 4 m wide and high, the middle one narrower (a door)
CHAIN_BOXES = (((0.0, -2.0, 0.0), (4.0, 2.0, 4.0)), ((3.0, -1.0, 0.0), (7.0, 1.0, 4.0)), ((6.0, -2.0, 0.0), (10.0, 2.0, 4.0)))


def rest_to_rest(p0, p1, T, order=7):
    """coef [1, 4, order + 1] of the straight flight p0 -> p1 in T seconds along s(u) = 35 u^4 - 84 u^5 + 70 u^6 - 20 u^7
    (at rest at both ends); exact in fp64 for lattice points and T a power of two"""
    coef = np.zeros((1, 4, order + 1))
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    for j, s in ((4, 35.0), (5, -84.0), (6, 70.0), (7, -20.0)):
        coef[0, :3, j] = (p1 - p0) * s / T ** j
    coef[0, :3, 0] = p0
    return coef


def chain_flights(order=7):
    """four straight flights, 8 s each: through all three boxes; leaving box 1 through its side wall (y = 1 at x = 5,
    inside box 1's x range and short of box 2); starting outside box 0; ending beyond the last box"""
    legs = [((1.0, 0.0, 2.0), (9.0, 0.0, 2.0)), ((1.0, 0.0, 2.0), (9.0, 2.0, 2.0)), ((-1.0, 0.0, 2.0), (9.0, 0.0, 2.0)),
            ((1.0, 0.0, 2.0), (12.0, 0.0, 2.0))]
    coef = np.stack([rest_to_rest(a, b, 8.0, order) for a, b in legs])
    return coef, np.full((4, 1), 8.0)


# ------------------------------------------------------------------------------------------------ the hole in the wall
HOLE_RADIUS = 0.1


def hole_corridor(tris, reach=0.5):
    """(planes, poly_offsets) of the three-box corridor through the wall of tests/golden/env-scene-hole.stl, from its
    vertices: the wall is a slab in y with one rectangular hole (the vertices off the slab's outline are the hole's).
    Box 0 is the free half-space in front of the wall, box 1 the hole extruded through the wall's thickness and `reach`
    beyond it on both sides (so that it overlaps the other two), box 2 the free half-space behind the wall."""
    v = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rim = v[(np.abs(v[:, 0]) < hi[0]) & (np.abs(v[:, 2]) < hi[2])]
    big = 1e3
    return boxes(((-big, -big, -big), (big, lo[1], big)),
                 ((rim[:, 0].min(), lo[1] - reach, rim[:, 2].min()), (rim[:, 0].max(), hi[1] + reach, rim[:, 2].max())),
                 ((-big, hi[1], -big), (big, big, big)))


def hole_flights(order=7):
    """8 straight rest-to-rest flights from y = -2 to y = 2 in 4 s: four through the hole (|x| + radius inside its
    half width 1.4112), one with a changing height, and three that meet the wall -- two before the hole's box is
    reached (stage 0) and one that leaves the hole's box sideways inside the wall (stage 1)"""
    legs = [((0.0, -2.0, 0.0), (0.0, 2.0, 0.0)), ((0.5, -2.0, 0.25), (-0.5, 2.0, 0.5)), ((1.0, -2.0, 0.0), (1.0, 2.0, 0.0)),
            ((1.25, -2.0, 0.0), (1.25, 2.0, 0.0)), ((2.5, -2.0, 0.0), (2.5, 2.0, 0.0)), ((0.0, -2.0, 1.0), (0.0, 2.0, 1.25)),
            ((-3.0, -2.0, 0.0), (0.5, 2.0, 0.0)), ((0.0, -2.0, 0.0), (3.0, 2.0, 0.0))]
    return np.stack([rest_to_rest(a, b, 4.0, order) for a, b in legs]), np.full((8, 1), 4.0)


HOLE_VERDICTS = [0, 0, 0, 0, 1, 0, 1, 1]      # CORRIDOR_INSIDE = 0, CORRIDOR_OUTSIDE = 1
HOLE_STAGES = [-1, -1, -1, -1, 0, -1, 0, 1]
