"""Mesh clearance on the GPU where it is not comfortable (include/msnap.h, "mesh clearance"): every closest feature of a
triangle and every kind of crossing, shared vertices and edges, several triangles, both orders at the segment counts
they are used at, extreme scales and durations, far from the origin, at the walk's caps, the longest path, solved
(curved) paths around a closed box, a wave that mixes 60-node lanes with one-node lanes and failed drones, lane counts
around the wavefront and workgroup boundaries, and the kernel against the NumPy restatement on 258 lanes.

Straight flights are held against the closed form of tests/mesh_flight_exact.py, solved paths against the slow exact
reference's recorded D (tests/golden/mesh_clearance_edges_golden.npz); the cases are tests/mesh_clearance_cases.py's,
whose conditions tests/test_mesh_clearance_edges_cpu.py asserts from the references alone.  Every family checks the
header's inequalities with R = mesh_R and the rounding bar C_ROUND_MESH = 3, that msnap_mesh_sweep of the position at
t_min returns min_dist bit for bit against the lowest triangle attaining it, and appends its figures to
profiles/mesh_clearance_edges.jsonl."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clearance_cases as MC  # noqa: E402
import mesh_clearance_exact as ME  # noqa: E402
import mesh_flight_exact as MF  # noqa: E402
from conftest import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu

RECORD = os.path.join(ROOT, "profiles", "mesh_clearance_edges.jsonl")
_started = []


def _record(line):
    """the first line of a process starts the file anew; a tree that cannot be written to loses the record only"""
    try:
        with open(RECORD, "a" if _started else "w") as f:
            f.write(json.dumps(line) + "\n")
        _started.append(1)
    except OSError:
        pass


@pytest.fixture(scope="module")
def ctxs(ctx7, ctx9):
    return {8: ctx7, 10: ctx9}


def _closes(md, lower, R):
    return bool(lower >= md * (1 - ME.REL_CLOSE) - ME.ABS_CLOSE - ME.round_terms(R))


def check_family(ctx, family, name, coef, dur, tris, exact, closed, attained=True):
    """One call of msnap_mesh_clearance held against the exact D of every drone: status, the time inside the flight,
    the header's inequalities (closed: the closing one too, one flag or one per drone), 0 <= lower <= min_dist, the
    rounding ratio against D and against the exact distance at t_min below C_ROUND_MESH, the attained value through
    the sweep (attained: of every drone, or of the listed ones); one record line."""
    md, tm, tri, lower, status = ctx.mesh_clearance(coef, dur, tris)
    assert (status == 0).all()
    closed = np.broadcast_to(closed, len(md))
    worst, over, under, n_closed = -np.inf, -np.inf, -np.inf, 0
    for d in range(len(md)):
        D = exact[d]
        R = ME.mesh_R(coef[d], dur[d], tris)
        r = ME.round_terms(R)
        ratio = ME.round_ratio(md[d], lower[d], D, R, ME.exact_distance_at(coef[d], dur[d], tris, float(tm[d])))
        worst, over, under = max(worst, ratio), max(over, md[d] - float(D)), max(under, float(D) - lower[d])
        n_closed += _closes(md[d], lower[d], R)
        print(f"{name} drone {d}: lower {lower[d]!r} D {float(D)!r} min_dist {md[d]!r} t_min {tm[d]!r} tri {tri[d]} "
              f"rounding / (2^-52 R) {ratio:.3f}")
        assert 0.0 <= tm[d] <= ME.knots(dur[d])[-1], d
        assert 0.0 <= lower[d] <= md[d], d
        assert lower[d] <= float(D) * (1 + ME.REL_ROUND) + r and float(D) <= md[d] * (1 + ME.REL_ROUND) + r, d
        assert not ME.contract_violations(md[d], lower[d], D, closed=bool(closed[d]), R=R), d
    print(f"{family} {name}: worst rounding / (2^-52 R) {worst:.3f}, closed {n_closed} of {len(md)}")
    assert worst < ME.C_ROUND_MESH
    at = np.arange(len(md)) if attained is True else np.asarray(attained)
    MC.check_attained(ctx, coef[at], dur[at], tris, md[at], tm[at], tri[at])
    _record({"family": family, "name": name, "order": coef.shape[3] - 1, "M": int(dur.shape[1]), "drones": len(md),
             "worst_round_ratio": worst, "worst_min_dist_minus_D": over, "worst_D_minus_lower": under, "closed": n_closed})
    return md, tm, tri, lower


def check_line(ctxs, family, name, closed):
    line = MC.get_line(family, name)
    coef, dur, tris = MC.line_paths(line)
    exact = [e[0] for e in MC.line_exact(family, name)]
    return check_family(ctxs[line["nc"]], family, name, coef, dur, tris, exact, closed)


# ------------------------------------------------------------------------------------------------ the contract per family
@pytest.mark.parametrize("name", list(MC.FEATURES))
def test_every_closest_feature_and_crossing(ctxs, name):
    """On the fan and the ridge the shared vertex / edge belongs to several triangles: check_attained pins the copy
    that wins (the lowest index attaining min_dist)."""
    check_line(ctxs, "FEATURES", name, closed=True)


@pytest.mark.parametrize("name", list(MC.RANDOM))
def test_random_polylines(ctxs, name):
    check_line(ctxs, "RANDOM", name, closed=True)


@pytest.mark.parametrize("name", list(MC.FAR))
def test_far_from_the_origin(ctxs, name):
    """The closing inequality on every drone but the one on which the restatement's walk meets a cap
    (mesh_clearance_cases.FAR_CAPPED, asserted in tests/test_mesh_clearance_edges_cpu.py): 287 of 288."""
    check_line(ctxs, "FAR", name, closed=MC.far_closed(name))


@pytest.mark.parametrize("name", list(MC.CAPS))
def test_at_the_caps(ctxs, name):
    """A bounded loop of 4096 nodes per lane; the restatement meets a cap on 8 of the 24 drones
    (tests/test_mesh_clearance_edges_cpu.py asserts at least a quarter).  lower stays proven: 0 <= lower <= D."""
    check_line(ctxs, "CAPS", name, closed=False)


@pytest.mark.parametrize("name", list(MC.LONGEST))
def test_the_longest_path(ctxs, name):
    assert MC.LONGEST[name][1] == ctxs[8].max_segments == 4096
    check_line(ctxs, "LONGEST", name, closed=True)


@pytest.mark.parametrize("name", list(MC.CURVED))
def test_solved_paths_around_a_closed_box(ctxs, name):
    coef, dur, tris = MC.curved_case(name)
    gold = MC.edges_golden()
    assert np.array_equal(gold[name + "_sha256"], MC.inputs_sha256(coef, dur, tris))      # D is of these inputs
    check_family(ctxs[coef.shape[3]], "CURVED", name, coef, dur, tris, gold[name], closed=True)


# ------------------------------------------------------------------------------------------------ a mixed wave
def _mixed(m):
    """65 polylines of m segments against the fan: 0, 63 and 64 cross it off the grid (through the apex, through a
    spoke), the others hover or fly short legs 30 m away.  -> (points [65, m + 1, 3], durs [65, m])"""
    crossings = [p for p, c in zip(MC.features_line("o7_fan")["points"], MC.line_closest("FEATURES", "o7_fan"))
                 if c[1] == "crossing"]
    rng = np.random.default_rng(21200 + m)
    points = np.zeros((65, m + 1, 3))
    for d in range(65):
        if d in (0, 63, 64):
            p, q = crossings[(0, 63, 64).index(d) * 2]
            lead = [q + (k + 1) * np.array([0.5, 0.25, 1.0]) for k in range(m - 1)]      # on from q, away from the cone
            points[d] = np.array([p, q] + lead)
        elif d % 2:
            points[d] = rng.integers(16, 33, size=(1, 3)) / 8.0                           # hovering, 2 to 4 m out
        else:
            points[d] = 30.0 + np.cumsum(rng.integers(-4, 5, size=(m + 1, 3)), axis=0) / 8.0
    return points, np.ldexp(1.0, rng.integers(-1, 2, size=(65, m)))


@pytest.mark.parametrize("nc", [8, 10])
def test_a_wave_of_deep_and_shallow_lanes_with_failed_drones(ctxs, nc):
    """260 lanes in one call: 65 drones of one segment, then the same of four.  A commit that is not under `if (active)`
    shows where a 60-node lane shares its wave with lanes that finished after one node."""
    ctx, tris = ctxs[nc], MC.FAN
    for m in (1, 4):
        points, durs = _mixed(m)
        both = [MF.path(p, t, nc) for p, t in zip(points, durs)]
        coef, dur = np.stack([c for c, _ in both]), np.stack([t for _, t in both])
        coef[1, 0, 3, 1] = np.nan
        dur[62, m - 1] = 0.0
        whole = ctx.mesh_clearance(coef, dur, tris)
        md, tm, tri, lower, status = whole
        assert status[1] == 3 and status[62] == 2 and (np.delete(status, [1, 62]) == 0).all()
        for d in (1, 62):
            assert np.isnan(md[d]) and np.isnan(tm[d]) and np.isnan(lower[d]) and tri[d] == -1
        flipped = ctx.mesh_clearance(coef[::-1], dur[::-1], tris)
        for f, w in zip(flipped, whole):
            assert np.array_equal(f[::-1], w, equal_nan=True)
        for d in range(65):
            alone = ctx.mesh_clearance(coef[d:d + 1], dur[d:d + 1], tris)
            for a, w in zip(alone, whole):
                assert np.array_equal(a[0], w[d], equal_nan=True), (m, d)
        good = [d for d in range(65) if d not in (1, 62)]
        exact = [MF.exact_polyline_clearance(points[d], tris)[0] for d in good]
        assert all(exact[good.index(d)] == 0 for d in (0, 63, 64))
        check_family(ctx, "MIXED", f"o{nc - 1}_m{m}", coef[good], dur[good], tris, exact, closed=True)


# ------------------------------------------------------------------------------------------------ lane counts
LANES = [(63, 1), (21, 3), (64, 1), (65, 1), (255, 1), (85, 3), (256, 1), (257, 1), (513, 1), (171, 3)]


@pytest.mark.parametrize("nc,n,m", [(8, n, m) for n, m in LANES] + [(10, 65, 1), (10, 85, 3), (10, 257, 1)])
def test_lane_counts_around_a_wavefront_and_a_workgroup(ctxs, nc, n, m):
    assert n * m in (63, 64, 65, 255, 256, 257, 513)
    line = MC.random_flights(nc, n, m, 21300 + n * m)
    coef, dur, tris = MC.line_paths(line)
    exact = [MF.exact_polyline_clearance(p, tris)[0] for p in line["points"]]
    whole = check_family(ctxs[nc], "LANES", f"o{nc - 1}_n{n}_m{m}", coef, dur, tris, exact, closed=True,
                         attained=sorted({0, 1, n // 4, n // 2, n - 2, n - 1}))      # (a sample: 2 + 4 sweeps per drone)
    alone = ctxs[nc].mesh_clearance(coef[-1:], dur[-1:], tris)
    for a, w in zip(alone, whole):
        assert np.array_equal(a[0], w[-1])
    assert alone[4][0] == 0


# ------------------------------------------------------------------------------------------------ kernel against restatement
@pytest.mark.parametrize("nc", [8, 10])
def test_the_kernel_against_the_restatement_on_258_lanes(ctxs, nc):
    from drone_path_planning_python_amd import synthetic
    coef, dur = MC.solve(*synthetic.swarm(12900 + nc - 1, 129, 2), nc)
    tris = MC.scene("both")
    md, tm, tri, lower, status = ctxs[nc].mesh_clearance(coef, dur, tris)
    rmd, rtm, rtri, rlower = ME.fp64_mesh_clearance(coef, dur, tris)
    print("largest |min_dist - restated|", np.abs(md - rmd).max(), "|lower - restated|", np.abs(lower - rlower).max())
    assert (status == 0).all() and (lower <= md).all() and (lower >= 0).all()
    assert np.allclose(md, rmd, rtol=1e-9, atol=2e-9) and np.allclose(lower, rlower, rtol=1e-9, atol=2e-9)
