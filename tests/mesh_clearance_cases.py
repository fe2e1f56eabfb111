"""Inputs of the mesh clearance tests (tests/test_mesh_clearance_cpu.py, tests/test_mesh_clearance_gpu.py) and of
tests/golden/make_mesh_clearance_golden.py, which records the exact reference's D for them: the exact reference takes
up to a minute per drone, the tests read its results from tests/golden/mesh_clearance_golden.npz."""
from __future__ import annotations

import os

import numpy as np

from drone_path_planning_python_amd import stl, synthetic

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "mesh_clearance_golden.npz")
ONE_TRI = np.array([[[0.25, -2.0, -2.5], [0.25, 3.0, -2.0], [0.25, 0.5, 3.0]]])


def solve(wp, t, nc):
    import c_oracle
    coef, dur, info, _ = c_oracle.solve_batch(wp, t, ncoef=nc)
    assert not info.any()
    return coef, dur


def scene(name):
    hole = stl.load_stl(os.path.join(GOLDEN_DIR, "env-scene-hole.stl"))
    ltu = stl.load_stl(os.path.join(GOLDEN_DIR, "env-scene-ltu-experiment.stl"))
    return {"one": ONE_TRI, "hole": hole, "ltu": ltu, "both": np.concatenate([hole, ltu])}[name]


def tunnelling(nc=8, x0=-1.0, x1=1.0, y=0.3, z=0.2, total=1.1, offset=0.0):
    """One rest-to-rest segment from x0 to x1 (2 m in 1.1 s: about 4 m/s in the middle) at height z."""
    wp = np.zeros((1, 2, 4))
    wp[0, :, 0] = [x0 + offset, x1 + offset]
    wp[0, :, 1] = y + offset
    wp[0, :, 2] = z + offset
    return solve(wp, np.array([0.0, total]), nc)


# name -> (order, segments, drones, scene): per-drone times throughout (synthetic.swarm)
CONTRACT = {
    "o7_m1_one": (7, 1, 2, "one"), "o7_m2_one": (7, 2, 2, "one"), "o7_m10_one": (7, 10, 2, "one"),
    "o9_m4_one": (9, 4, 2, "one"), "o7_m2_hole": (7, 2, 2, "hole"), "o7_m10_ltu": (7, 10, 2, "ltu"),
    "o7_m1_both": (7, 1, 2, "both"), "o9_m4_both": (9, 4, 2, "both"),
}


def contract_case(name):
    order, m, n, sc = CONTRACT[name]
    coef, dur = solve(*synthetic.swarm(11000 + 10 * m + order, n, m), order + 1)
    return coef, dur, scene(sc)


CERTIFY_RADIUS = 0.125


def certify_case():
    """12 straight rest-to-rest flights around env-scene-hole.stl (the wall is 0.5 m thick; 4.4 m in 1.1 s: the samples
    either side of it stay 0.18 m away): through the hole, past the wall, tunnelling through it, and one that flies
    along the wall in front of triangle 2 (all of whose vertices have y = -0.25 exactly) with y = -0.375 throughout,
    exact in fp64: it touches at exactly CERTIFY_RADIUS, D = radius, no hit.  -> (coef, dur, tris)"""
    hole = scene("hole")
    wp = np.zeros((12, 2, 4))
    for d, x in enumerate([0.0, 0.1, -0.1, 5.0, -5.0, 2.5, -2.5, 3.0, 1.8, 0.05, 6.0]):
        wp[d, :, 0], wp[d, :, 1], wp[d, :, 2] = x, [-2.2, 2.2], 0.1 * (d % 3)
    assert (hole[2, :, 1] == -0.25).all()
    wp[11, :, 0], wp[11, :, 2] = [3.0, 3.5], -0.25
    coef, dur = solve(wp, np.array([0.0, 1.1]), 8)
    coef[11, :, 1, :] = 0.0
    coef[11, :, 1, 0] = -0.25 - CERTIFY_RADIUS
    return coef, dur, hole


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def sweep_at(ctx, coef, dur, tris, d, t):
    """msnap_mesh_sweep of the single position msnap_eval_flat gives drone d at time t."""
    out = ctx.eval_flat(coef[d:d + 1], dur[d:d + 1], np.array([t]))
    md, _ = ctx.mesh_sweep(np.ascontiguousarray(out[:, :, :3]), tris, 0.1)
    return md[0]


def check_attained(ctx, coef, dur, tris, md, tm, tri):
    for d in range(len(md)):
        assert sweep_at(ctx, coef, dur, tris, d, tm[d]) == md[d], d
        out = ctx.eval_flat(coef[d:d + 1], dur[d:d + 1], tm[d:d + 1])
        each = np.array([ctx.mesh_sweep(np.ascontiguousarray(out[:, :, :3]), tris[k:k + 1], 0.1)[0][0] for k in range(len(tris))])
        assert tri[d] == int(np.nanargmin(each)) and each[tri[d]] == md[d], (d, tri[d], each)


# ---------------------------------------------------------------------------------------------------------------------
# Straight flights (tests/mesh_flight_exact.py; tests/test_mesh_clearance_edges_cpu.py, _gpu.py).  A "line" is a dict:
# name, nc, points [N, M + 1, 3] and durs [N, M] (one polyline per drone, on a dyadic lattice, durations powers of two),
# tris [T, 3, 3].  Everything is drawn from the seed in the spec or built from the closed form alone; the builders cache.
# Lattice coordinates are written in eighths of a metre.
EDGES_GOLDEN = os.path.join(GOLDEN_DIR, "mesh_clearance_edges_golden.npz")
FRACTIONS = (0.375, 0.3125)      # where on the line a built closest approach sits: never 0, 1/2 or 1 (the walk's samples)

_cache = {}


def _cached(fn):
    def get(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    get.__name__ = fn.__name__
    get.__doc__ = fn.__doc__
    return get


def line_paths(line):
    """-> (coef [N, M, 4, nc], dur [N, M], tris) of a line; every coefficient asserted exact (mesh_flight_exact.flight)."""
    import mesh_flight_exact as MF
    both = [MF.path(p, t, line["nc"]) for p, t in zip(line["points"], line["durs"])]
    return np.stack([c for c, _ in both]), np.stack([t for _, t in both]), line["tris"]


@_cached
def line_closest(family, name):
    """Per drone of the line: mesh_flight_exact.polyline_closest's (d2, feature, segment, s, triangle)."""
    import mesh_flight_exact as MF
    line = get_line(family, name)
    return [MF.polyline_closest(p, line["tris"]) for p in line["points"]]


@_cached
def line_exact(family, name):
    """Per drone of the line: (D as mpf, feature) from the closed form."""
    import mesh_flight_exact as MF
    line = get_line(family, name)
    return [MF.exact_polyline_clearance(p, line["tris"]) for p in line["points"]]


def get_line(family, name):
    return {"FEATURES": features_line, "RANDOM": random_line, "FAR": far_line, "CAPS": caps_line,
            "LONGEST": longest_line}[family](name)


def _moved(line, name, offset, scale=1.0):
    """The line with swarm and mesh scaled and moved, every coordinate still exact."""
    from fractions import Fraction
    out = dict(line, name=name, points=line["points"] * scale + offset, tris=line["tris"] * scale + offset)
    for a, b in ((line["points"], out["points"]), (line["tris"], out["tris"])):
        for x, y in zip(a.reshape(-1), b.reshape(-1)):
            assert Fraction(float(x)) * Fraction(scale) + Fraction(offset) == Fraction(float(y))
    return out


def _lattice_tris(rng, n):
    """n non-degenerate triangles: a centre within 3 m of the origin, vertices within 2 m of it."""
    out = []
    while len(out) < n:
        t = (rng.integers(-24, 25, size=(1, 3)) + rng.integers(-16, 17, size=(3, 3))) / 8.0
        if np.any(np.cross(t[1] - t[0], t[2] - t[0])):
            out.append(t)
    return np.array(out)


# --- RANDOM: name -> (order, segments, log2 of the coordinate scale, log2 of the base duration, seed); 24 drones each
RANDOM_DRONES = 24
RANDOM = {
    "o7_m1": (7, 1, 0, 0, 21001), "o7_m2": (7, 2, 0, 0, 21002), "o7_m3": (7, 3, 0, 0, 21003), "o7_m10": (7, 10, 0, 0, 21004),
    "o9_m1": (9, 1, 0, 0, 21005), "o9_m2": (9, 2, 0, 0, 21006), "o9_m3": (9, 3, 0, 0, 21007), "o9_m10": (9, 10, 0, 0, 21008),
    "o9_m20": (9, 20, 0, 0, 21009), "o7_m64": (7, 64, 0, 0, 21010),
    "o7_m2_small": (7, 2, -10, 0, 21011), "o9_m3_small": (9, 3, -10, 0, 21012),
    "o7_m3_large": (7, 3, 8, 0, 21013), "o9_m2_large": (9, 2, 8, 0, 21014),
    "o7_m3_quick": (7, 3, 0, -6, 21015), "o9_m2_quick": (9, 2, 0, -6, 21016),
    "o7_m2_slow": (7, 2, 0, 6, 21017), "o9_m3_slow": (9, 3, 0, 6, 21018),
}


def _random_points(rng, n, m):
    """n polylines of m segments: up to 3 segments between points anywhere within 4 m of the origin, longer ones a walk
    in steps of up to 0.75 m per axis (a long polyline of 8 m legs crosses nearly every triangle)."""
    if m <= 3:
        return rng.integers(-32, 33, size=(n, m + 1, 3)) / 8.0
    start = rng.integers(-32, 33, size=(n, 1, 3))
    steps = rng.integers(-6, 7, size=(n, m, 3))
    return np.concatenate([start, start + np.cumsum(steps, axis=1)], axis=1) / 8.0


@_cached
def random_line(name):
    order, m, ls, lt, seed = RANDOM[name]
    rng = np.random.default_rng(seed)
    tris = _lattice_tris(rng, int(rng.integers(1, 7)))
    points = _random_points(rng, RANDOM_DRONES, m)
    durs = np.ldexp(1.0, lt + rng.integers(-1, 2, size=(RANDOM_DRONES, m)))
    base = dict(name=name, nc=order + 1, points=points, durs=durs, tris=tris)
    return _moved(base, name, 0.0, 2.0 ** ls)


def random_flights(nc, n, m, seed):
    """n more polylines of m segments drawn as RANDOM's, against 4 triangles (the lane counts of the GPU tests)."""
    rng = np.random.default_rng(seed)
    tris = _lattice_tris(rng, 4)
    return dict(name=f"n{n}_m{m}", nc=nc, points=_random_points(rng, n, m),
                durs=np.ldexp(1.0, rng.integers(-1, 2, size=(n, m))), tris=tris)


# --- FAR: RANDOM's one- and two-segment lines with swarm and mesh moved: name -> (RANDOM's name, offset [m]).
# FAR_CAPPED: name -> the drones on which the restatement's walk meets a cap (stats["capped"]); the header promises the
# closing inequality short of the caps only, so these alone are run without it.  It is one drone: at +1e5 m it passes an
# edge at 1.36 mm, where the third candidate normal (p - q) / |p - q|, from points that carry an ulp of 1e5 m each,
# is off by about 1e-8, and the support function charges that tilt with the triangle's extent: the node cannot close
# against 1e-9 m.  tests/test_mesh_clearance_edges_cpu.py asserts that the restatement marks exactly these.
FAR = {f"{base}{tag}": (base, off) for base in ("o7_m1", "o7_m2", "o9_m1", "o9_m2")
       for tag, off in (("+5000", 5000.0), ("-8000", -8000.0), ("+1e5", 1e5))}
FAR_CAPPED = {"o9_m2+1e5": (16,)}


@_cached
def far_line(name):
    base, off = FAR[name]
    return _moved(random_line(base), name, off)


def far_closed(name):
    """Per drone of the FAR line: whether the closing inequality is asserted (all but FAR_CAPPED's)."""
    closed = np.ones(RANDOM_DRONES, dtype=bool)
    closed[list(FAR_CAPPED.get(name, ()))] = False
    return closed


# --- CAPS: one triangle, one order-7 segment, so far out that an ulp of a coordinate (1.9e-9 m at 1e7 m) exceeds what
# the prune leaves open (1e-9 m), and flights that pass a vertex or an edge of it at 0.125 to 0.8 m, 15/16 of the way
# along the line: s(3/4) = 0.929 at order 7, so the closest approach lies in the last quarter of the time, the part a
# walk that the node guard ends leaves unvisited.  name -> offset [m]
CAPS = {"o7_m1+1e7": 1e7}
CAPS_DRONES = 24
CAPS_FRACTION = 0.9375


@_cached
def caps_line(name):
    tris = FEATURE_TRIS[0:1]
    t8 = np.rint(tris[0] * 8).astype(np.int64)
    n = np.cross(t8[1] - t8[0], t8[2] - t8[0])
    feet = [(t8[v], "vertex") for v in range(3)]
    feet += [(t8[e] + k * (t8[(e + 1) % 3] - t8[e]) // 4, "edge") for e in range(3) for k in (1, 2, 3)]
    points = np.array([_find_flight(tris, foot, CAPS_FRACTION, want, side, n, w2=(1, 40), skip=3 * (i % 4))
                       for i, (foot, want) in enumerate(feet) for side in (1, -1)])      # (skip: not the same flight moved)
    assert len(points) == CAPS_DRONES
    base = dict(name=name, nc=8, points=points, durs=np.ones((CAPS_DRONES, 1)), tris=tris)
    return _moved(base, name, CAPS[name])


# --- LONGEST: one order-7 drone with as many segments as a context takes, a zigzag above one triangle
LONGEST = {"o7_m4096": (7, 4096)}


@_cached
def longest_line(name):
    order, m = LONGEST[name]
    i = np.arange(m + 1)
    points = np.stack([np.where(i % 2 == 0, -16, 16), (7 * i) % 65 - 32, (3 * i) % 17 + 12], axis=1)[None] / 8.0
    durs = np.where(np.arange(m) % 2 == 0, 0.5, 0.25)[None]
    tris = np.array([[[-1.0, -1.0, 0.5], [1.5, -1.0, 0.0], [-0.5, 1.5, 1.0]]])
    return dict(name=name, nc=order + 1, points=points, durs=durs, tris=tris)


# --- FEATURES: flights built so that a chosen vertex, open edge or the face of a fixed triangle is the closest feature,
# from both sides of its plane, and crossings; on the fan of six triangles around a shared vertex and on two triangles
# that share an edge also the flights whose closest feature (or crossing) is the shared one.  name -> order; the
# geometry is the same at both orders.
FEATURE_TRIS = np.array([[[0, 0, 0], [16, 4, 0], [4, 16, 8]], [[-8, -8, 4], [12, -8, -4], [-4, 12, 12]],
                         [[0, 0, 0], [32, 0, 0], [-8, 8, 4]], [[8, 8, 8], [12, 12, 8], [8, 12, 16]]]) / 8.0
_RING = np.array([[16, 0, -8], [8, 16, -4], [-8, 16, -8], [-16, 0, -4], [-8, -16, -8], [8, -16, -4]]) / 8.0
FAN = np.array([[[0.0, 0.0, 0.0], _RING[i], _RING[(i + 1) % 6]] for i in range(6)])       # the apex is every triangle's vertex 0
RIDGE = np.array([[[-8, 0, 0], [8, 0, 4], [0, 12, -8]], [[8, 0, 4], [-8, 0, 0], [0, -12, -4]]]) / 8.0      # share the edge (-1, 0, 0)-(1, 0, 0.5)
FEATURE_MESHES = {"tri0": FEATURE_TRIS[0:1], "tri1": FEATURE_TRIS[1:2], "tri2": FEATURE_TRIS[2:3], "tri3": FEATURE_TRIS[3:4],
                  "fan": FAN, "ridge": RIDGE}
FEATURES = {f"o{order}_{mesh}": (order, mesh) for order in (7, 9) for mesh in FEATURE_MESHES}


def _small_vectors(step, reach):
    """Non-zero integer vectors with components in step * [-reach, reach], nearest first (a fixed order)."""
    r = range(-reach, reach + 1)
    v = [(x * step, y * step, z * step) for x in r for y in r for z in r if (x, y, z) != (0, 0, 0)]
    return sorted(v, key=lambda a: (a[0] * a[0] + a[1] * a[1] + a[2] * a[2], a))


def _find_flight(tris, foot, frac, want, side=None, normal=None, w2=(16, 192), skip=0):
    """The first flight p -> q (after `skip` others), in a fixed order of small lattice vectors, whose closest approach
    to the mesh is at `foot` (a lattice point of the mesh, eighths) from the point foot + w of the line, `frac` of the way along it, with
    the closed form reporting feature `want` there.  w runs over the lattice (w2[0] <= |w|^2 <= w2[1] in eighths: at
    least half a metre unless told otherwise, nearest first), the direction d over whole metres (two when frac counts
    sixteenths) with d.w = 0, so p = foot + w - frac d is on the lattice.  side: the sign of w.normal."""
    import mesh_flight_exact as MF
    from fractions import Fraction
    unit = 8 if frac == 0.375 else 16
    foot = np.asarray(foot, dtype=np.int64)
    for w in _small_vectors(1, 8):
        wn = int(np.dot(w, normal)) if normal is not None else 0
        if not w2[0] <= np.dot(w, w) <= w2[1] or (side is not None and np.sign(wn) != side):
            continue
        m = (foot + np.array(w)) / 8.0
        d2, feat = MF.polyline_closest(np.array([m, m]), tris)[:2]
        if feat != want or d2 != Fraction(int(np.dot(w, w)), 64):      # the mesh is nearer to foot + w somewhere else
            continue
        for d in _small_vectors(unit, 2):
            if np.dot(d, w) != 0:
                continue
            p = (foot + np.array(w) - np.array(d) * frac) / 8.0
            q = p + np.array(d) / 8.0
            d2, feat, _, s, _ = MF.polyline_closest(np.array([p, q]), tris)
            if feat == want and s == Fraction(frac) and d2 == Fraction(int(np.dot(w, w)), 64):
                if skip == 0:
                    return np.array([p, q])
                skip -= 1
    raise AssertionError(("no flight", foot, frac, want, side))


def _find_crossing(tris, through, frac, k):
    """The k-th direction d (whole metres, a fixed order) whose flight from through - frac d crosses the mesh at the
    lattice point `through`, frac of the way along."""
    import mesh_flight_exact as MF
    from fractions import Fraction
    unit = 8 if frac == 0.375 else 16
    found = 0
    for d in _small_vectors(unit, 2):
        p = (np.asarray(through) - np.array(d) * frac) / 8.0
        q = p + np.array(d) / 8.0
        d2, feat, _, s, _ = MF.polyline_closest(np.array([p, q]), tris)
        if feat == "crossing" and s == Fraction(frac) and min(abs(x) for x in d) > 0:
            if found == k:
                return np.array([p, q])
            found += 1
    raise AssertionError(("no crossing", through, frac, k))


def _find_landing(tris, foot, normal, side):
    """A flight that ends above (side) the face's interior point `foot` and has its closest approach there."""
    import mesh_flight_exact as MF
    g = int(np.gcd.reduce(np.abs(normal)))
    up = side * np.asarray(normal) // g
    for h in (1, 2):
        q = np.asarray(foot) + h * up
        for d in _small_vectors(8, 2):
            if np.dot(d, up) <= 0:
                continue
            pts = np.array([q + np.array(d), q]) / 8.0
            d2, feat, _, s, _ = MF.polyline_closest(pts, tris)
            if feat == "face" and s == 1:
                return pts
    raise AssertionError(("no landing", foot, side))


@_cached
def _feature_flights(mesh):
    """points [N, 2, 3] of the flights against FEATURE_MESHES[mesh] (eighths until the end), the fractions alternating."""
    tris = FEATURE_MESHES[mesh]
    t8 = np.rint(tris * 8).astype(np.int64)
    out, turn = [], [0]

    def frac():
        turn[0] += 1
        return FRACTIONS[turn[0] % 2]

    if mesh.startswith("tri"):
        a, b, c = t8[0]
        n = np.cross(b - a, c - a)
        for v in range(3):
            for side in (1, -1):
                out.append(_find_flight(tris, t8[0][v], frac(), "vertex", side, n))
        for e in range(3):
            mid = (t8[0][e] + t8[0][(e + 1) % 3]) // 2
            for side in (1, -1):
                out.append(_find_flight(tris, mid, frac(), "edge", side, n))
        inner = a + ((b - a) + (c - a)) // 4
        for side in (1, -1):
            out.append(_find_landing(tris, inner, n, side))
        for k in range(2):
            out.append(_find_crossing(tris, inner, FRACTIONS[k], k))
        e1, e2 = (b - a) // 4, (c - a) // 4
        out.append(np.array([a - e1 - e2, a + 4 * e1 - 2 * e2]) / 8.0)                              # in the plane, outside
        g = int(np.gcd.reduce(np.abs(n)))
        over = np.array([inner + n // g, inner + n // g]) / 8.0                                     # over the face, parallel to it
        d = 2 * (b - a) - 2 * (c - a)
        out.append(over + np.array([-0.375 * d, 0.625 * d]) / 8.0)
    elif mesh == "fan":
        apex = t8[0][0]
        for k in range(4):
            out.append(_find_crossing(tris, apex, FRACTIONS[k % 2], k))                            # exactly through the shared vertex
        out.append(_find_crossing(tris, (t8[0][0] + t8[0][1]) // 2, FRACTIONS[0], 0))              # through a spoke: an edge of two
        for f in FRACTIONS:
            out.append(_find_flight(tris, apex, f, "vertex"))                                      # past the apex: six copies tie
    else:
        a, b = t8[0][0], t8[0][1]
        mid = (a + b) // 2
        for k in range(4):
            out.append(_find_crossing(tris, mid, FRACTIONS[k % 2], k))                             # exactly through the shared edge
        for f in FRACTIONS:
            out.append(_find_flight(tris, mid, f, "edge"))                                         # past it: both copies tie
        out.append(_find_flight(tris, a, FRACTIONS[0], "vertex"))
    return np.array(out)


@_cached
def features_line(name):
    order, mesh = FEATURES[name]
    points = _feature_flights(mesh)
    return dict(name=name, nc=order + 1, points=points, durs=np.ones((len(points), 1)), tris=FEATURE_MESHES[mesh])


# --- CURVED: solved paths (the hull of a straight flight does not bend) against a closed box inside the swarm's volume;
# D from the slow exact reference, recorded.  name -> (order, segments, drones)
CURVED = {"o9_m10": (9, 10, 6), "o9_m1": (9, 1, 6), "o7_m3": (7, 3, 6)}
BOX = (np.array([-1.0, -0.75, -1.5]), np.array([1.0, 1.25, 0.5]))


def box_tris(lo, hi):
    """The 12 triangles of the closed box [lo, hi], two per face."""
    c = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    return np.array([[c[q[0]], c[q[i]], c[q[i + 1]]] for q in quads for i in (1, 2)])


def curved_case(name):
    order, m, n = CURVED[name]
    coef, dur = solve(*synthetic.swarm(12000 + 10 * m + order, n, m), order + 1)
    return coef, dur, box_tris(*BOX)


def inputs_sha256(coef, dur, tris):
    """SHA-256 of the inputs' bytes, as 32 uint8."""
    import hashlib
    h = hashlib.sha256()
    for x in (coef, dur, tris):
        h.update(np.ascontiguousarray(x, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def edges_golden():
    with np.load(EDGES_GOLDEN) as z:
        return {k: z[k] for k in z.files}
