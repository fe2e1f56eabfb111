"""Mesh clearance where it is not comfortable, without a GPU: the closed form for straight flights
(tests/mesh_flight_exact.py) against the slow exact reference, the conditions the families of
tests/mesh_clearance_cases.py have to meet from the references alone (which feature is closest, how many lanes of CAPS
meet a cap), and the NumPy restatement of the kernel's method (mesh_clearance_exact.fp64_mesh_clearance) held to the
header's contract on every family the GPU tests run."""
import os
import sys
from collections import Counter
from fractions import Fraction

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clearance_cases as MC  # noqa: E402
import mesh_clearance_exact as ME  # noqa: E402
import mesh_flight_exact as MF  # noqa: E402


def check_line(family, name, closed):
    """The restatement on one line against the closed form: per drone the header's inequalities (with R; closed: the
    closing one too, one flag or one per drone), the time inside the flight, the rounding ratio below C_ROUND_MESH.
    Returns (worst ratio, lanes that met a cap)."""
    line = MC.get_line(family, name)
    closed = np.broadcast_to(closed, len(line["points"]))
    coef, dur, tris = MC.line_paths(line)
    exact = MC.line_exact(family, name)
    st = {}
    md, tm, tri, lower = ME.fp64_mesh_clearance(coef, dur, tris, stats=st)
    worst = -np.inf
    for d in range(len(md)):
        D = exact[d][0]
        R = ME.mesh_R(coef[d], dur[d], tris)
        bad = ME.contract_violations(md[d], lower[d], D, closed=bool(closed[d]), R=R)
        assert not bad, (name, d, bad, exact[d][1], bool(st["capped"][d].any()))
        assert 0.0 <= lower[d] <= md[d] and 0.0 <= tm[d] <= ME.knots(dur[d])[-1]
        worst = max(worst, ME.round_ratio(md[d], lower[d], D, R, ME.exact_distance_at(coef[d], dur[d], tris, float(tm[d]))))
    print(f"{family} {name}: worst rounding / (2^-52 R) {worst:.3f}, lanes at a cap {int(st['capped'].sum())}")
    assert worst < ME.C_ROUND_MESH
    return worst, st["capped"]


# ------------------------------------------------------------------------------------------------ the two references
def test_flight_coefficients_are_exact_and_the_path_is_the_segment():
    for nc in (8, 10):
        coef, dur = MF.path([[0.125, -2.0, 1.0], [3.0, 0.5, 1.0], [3.0, 0.5, -0.25]], [0.5, 4.0], nc)
        for i, (a, b) in enumerate((([0.125, -2.0, 1.0], [3.0, 0.5, 1.0]), ([3.0, 0.5, 1.0], [3.0, 0.5, -0.25]))):
            T = Fraction(float(dur[i]))
            for x in (Fraction(0), T / 3, T / 2, T * 7 / 8, T):
                p = [sum(Fraction(float(c)) * x ** k for k, c in enumerate(coef[i, ax])) for ax in range(3)]
                s = {(p[ax] - Fraction(a[ax])) / (Fraction(b[ax]) - Fraction(a[ax])) for ax in range(3) if a[ax] != b[ax]}
                assert len(s) == 1 and 0 <= min(s) <= 1                 # one parameter for all axes: on the segment
                assert all(p[ax] == Fraction(a[ax]) for ax in range(3) if a[ax] == b[ax])
            assert (coef[i, 3] == 0).all()
    with pytest.raises(AssertionError):
        MF.flight([0.1, 0.0, 0.0], [1.0, 0.0, 0.0], 1.0, 8)              # 1.0 - 0.1 is not exact in fp64
    with pytest.raises(AssertionError):
        MF.flight([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 3.0, 8)              # 35 / 81 is not


def test_segment_segment_distance_by_hand():
    F = Fraction
    cases = [(([0, 0, 0], [2, 0, 0]), ([1, 1, 1], [1, 3, 1]), F(2)),            # interior against an end
             (([0, 0, 0], [2, 0, 0]), ([1, -1, 1], [1, 1, 1]), F(1)),           # interior against interior (skew)
             (([0, 0, 0], [2, 0, 0]), ([3, 0, 1], [5, 0, 1]), F(2)),            # parallel, apart: end against end
             (([0, 0, 0], [2, 0, 0]), ([1, 0, 1], [5, 0, 1]), F(1)),            # parallel, overlapping
             (([0, 0, 0], [2, 0, 0]), ([1, -1, 0], [1, 1, 0]), F(0)),           # crossing
             (([0, 0, 0], [0, 0, 0]), ([1, -1, 0], [1, 1, 0]), F(1)),           # a point against a segment
             (([0, 0, 0], [0, 0, 0]), ([1, 2, 2], [1, 2, 2]), F(9)),            # two points
             (([0, 0, 0], [4, 0, 0]), ([5, 1, 0], [9, 5, 0]), F(2))]            # both clamped
    for (p1, q1), (p2, q2), want in cases:
        a = [[F(x) for x in v] for v in (p1, q1, p2, q2)]
        d, s, t = MF.seg_seg(*a)
        back = MF.seg_seg(a[2], a[3], a[0], a[1])
        assert d == want == back[0] and 0 <= s <= 1 and 0 <= t <= 1, (p1, q1, p2, q2, d)
        w = [a[0][k] + s * (a[1][k] - a[0][k]) - a[2][k] - t * (a[3][k] - a[2][k]) for k in range(3)]
        assert sum(x * x for x in w) == d


def _one_of(mesh, want, nth=0):
    """(points [2, 3], tris) of the nth FEATURES flight against `mesh` whose closed-form feature is `want`."""
    name = f"o7_{mesh}"
    feats = [e[1] for e in MC.line_exact("FEATURES", name)]
    d = [i for i, f in enumerate(feats) if f == want][nth]
    return MC.features_line(name)["points"][d], MC.FEATURE_MESHES[mesh]


@pytest.mark.parametrize("mesh,want,nc", [("tri0", "vertex", 8), ("tri1", "edge", 8), ("tri2", "face", 10),
                                           ("tri3", "crossing", 8), ("fan", "crossing", 10), ("ridge", "crossing", 8)])
def test_the_closed_form_agrees_with_the_exact_reference(mesh, want, nc):
    """The two references were written independently: Fractions and a clamped closed form here, roots of the feature
    polynomials' derivatives at 60 digits there.  They agree to 1e-50 relative; at a crossing the closed form gives 0
    and the slow reference less than 1e-50 m.  One order per flight: the slow reference takes seconds on each."""
    points, tris = _one_of(mesh, want)
    coef, dur = MF.path(points, [1.0], nc)
    D, feat = MF.exact_polyline_clearance(points, tris)
    slow, _ = ME.exact_mesh_clearance(coef, dur, tris)
    assert feat == want
    with mpmath.workdps(ME.DPS):
        if want == "crossing":
            assert D == 0 and 0 <= slow < mpmath.mpf(10) ** -50
        else:
            assert D > 0 and abs(slow - D) <= mpmath.mpf(10) ** -50 * D, (D, slow)


def test_degenerate_and_non_finite_triangles_follow_the_sweep():
    p = np.array([[-1.0, 0.25, 0.5], [2.0, 0.25, 0.5]])
    needle = np.array([[[0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 1.0, 0.0]]])       # collinear: the union of its edges
    assert ME.tri_degenerate(needle)[0]
    D, feat = MF.exact_polyline_clearance(p, needle)
    assert D == 0.5 and feat == "edge"
    coef, dur = MF.path(p, [2.0], 8)
    assert abs(ME.exact_mesh_clearance(coef, dur, needle)[0] - D) < 1e-50
    nan = needle.copy()
    nan[0, 1, 1] = np.nan
    assert MF.exact_polyline_clearance(p, nan) == (mpmath.inf, None)
    both = np.concatenate([nan, needle + [[[0.0, 0.0, -1.0]]]])
    assert MF.polyline_closest(p, both)[4] == 1 and MF.exact_polyline_clearance(p, both)[0] == 1.5


# ------------------------------------------------------------------------------------------------ conditions on the cases
def test_features_hold_every_class_eight_times_per_order_off_the_walks_samples():
    for order in (7, 9):
        count, built = Counter(), 0
        for name, (o, mesh) in MC.FEATURES.items():
            if o != order:
                continue
            for d2, feat, _, s, _ in MC.line_closest("FEATURES", name):
                count[feat] += 1
                built += s in (Fraction(3, 8), Fraction(5, 16))
                assert feat != "crossing" or s in (Fraction(3, 8), Fraction(5, 16)), (name, s)      # no crossing at a sample
        print(order, dict(count), "at 3/8 or 5/16 of the line:", built)
        assert all(count[f] >= 8 for f in ("vertex", "edge", "face", "crossing")), count
        assert built >= 70
    # on the shared features every copy is equally near: the fan's six triangles at its apex, the ridge's two at its edge
    for mesh, copies in (("fan", 6), ("ridge", 2)):
        tris = MC.FEATURE_MESHES[mesh]
        hit = 0
        for p in MC.features_line(f"o7_{mesh}")["points"]:
            each = [MF.polyline_closest(p, tris[k:k + 1])[0] for k in range(len(tris))]
            hit += sum(x == min(each) for x in each) == copies
        assert hit >= 4, (mesh, hit)


def test_far_coordinates_stay_exact():
    for name, (base, off) in MC.FAR.items():
        far, near = MC.far_line(name), MC.random_line(base)
        assert len(far["points"]) == MC.RANDOM_DRONES
        assert np.array_equal(far["tris"] - off, near["tris"]) and np.array_equal(far["points"] - off, near["points"])
    assert set(MC.FAR_CAPPED) <= set(MC.FAR)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(MC.FEATURES))
def test_restatement_on_features(name):
    check_line("FEATURES", name, closed=True)


@pytest.mark.parametrize("name", list(MC.RANDOM))
def test_restatement_on_random(name):
    check_line("RANDOM", name, closed=True)


@pytest.mark.parametrize("name", list(MC.FAR))
def test_restatement_far_from_the_origin(name):
    """Every drone closes but those whose walk meets a cap, and FAR_CAPPED names exactly those: one drone in 288."""
    _, capped = check_line("FAR", name, closed=MC.far_closed(name))
    assert tuple(np.nonzero(capped.any(axis=1))[0]) == MC.FAR_CAPPED.get(name, ())
    assert sum(len(v) for v in MC.FAR_CAPPED.values()) == 1


@pytest.mark.parametrize("name", list(MC.LONGEST))
def test_restatement_on_the_longest_path(name):
    check_line("LONGEST", name, closed=True)


@pytest.mark.parametrize("name", list(MC.CAPS))
def test_restatement_at_the_caps(name):
    """At +1e7 m the restatement's walk meets a cap on 8 of the 24 drones (the condition: at least a quarter), all
    with the closest approach in the last quarter of the segment; `lower` stays proven on every one."""
    for d2, feat, _, s, _ in MC.line_closest("CAPS", name):
        assert s == Fraction(MC.CAPS_FRACTION) and d2 > 0
    _, capped = check_line("CAPS", name, closed=False)
    print("drones at a cap:", int(capped.any(axis=1).sum()), "of", len(capped))
    assert capped.any(axis=1).sum() * 4 >= len(capped)


# ------------------------------------------------------------------------------------------------ the recorded D
def test_a_curved_golden_entry_is_what_the_exact_reference_gives():
    gold = MC.edges_golden()
    for name in MC.CURVED:
        assert np.array_equal(gold[name + "_sha256"], MC.inputs_sha256(*MC.curved_case(name))), name
        assert gold[name].shape == (MC.CURVED[name][2],) and np.isfinite(gold[name]).all()
    coef, dur, tris = MC.curved_case("o7_m3")
    _, tm, _, _ = ME.fp64_mesh_clearance(coef[:1], dur[:1], tris)
    D, _ = ME.exact_mesh_clearance(coef[0], dur[0], tris, hint_t=[float(tm[0])])
    assert float(D) == gold["o7_m3"][0]
