"""tests/solve_exact.py (the 60-digit K1 reference with the start-row quirk) against everything that already pins the
solve -- states_exact, the order-9 fixture, the reference's own outputs, the dense fp64 oracle -- and
tests/solve_cases.py (the table of kernel instances) against the launcher's ranges in msnap_solve.hip.  No GPU.

The 1e-11 bars are bars on the DENSE fp64 REFERENCE (a pivoted LU of the collocation system), not on a kernel: ten
times the worst 1.0e-12 measured for it against 60 digits on the draw of tools/solve_stress.py (order 9, 10 segments;
order 7 stays below 1e-13)."""
import os
import re

import numpy as np
import pytest

import solve_cases as SC
import solve_exact as SX
import states_exact as SE
from conftest import GOLDEN_DIR, ROOT, norm_rel

ORACLE_BAR = 1e-11


# ---------------------------------------------------------------------------
# against states_exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", [7, 9])
@pytest.mark.parametrize("M", [1, 2, 10])
def test_rest_to_rest_is_states_exact_bit_for_bit(order, M):
    K = SC.khalf(order)
    wp, t = SC.inputs(order, M, "uneven", n=2)
    t = t - t[:, :1]                        # t[0] == 0 on both drones (the raised one is shifted back, bits differ)
    for d in range(2):
        want = SE.exact_solve(t[d], wp[d], [(None, None)], K)[0]
        got = SX.exact_solve_k1(t[d], wp[d], K)
        assert got.shape == (M, 4, 2 * K)
        assert got.tobytes() == want.tobytes()
    both = SX.exact_batch_k1(wp, t, K)
    assert both is SX.exact_batch_k1(wp.copy(), t.copy(), K), "the cache is keyed by the inputs' bytes"
    assert both[1].tobytes() == want.tobytes() and not both.flags.writeable


def test_raised_start_moves_segment_0_only_through_the_start_rows():
    """With t[0] = s the start rows say p_0(s) = w_0 and p_0^(j)(s) = 0: checked on the solution itself, and the
    solution differs from the t[0] == 0 one (the quirk is not a shift of the clock)."""
    import mpmath as mp
    K, M = 4, 3
    wp, t = SC.inputs(7, M, "uneven", n=1)
    t = t + 0.25 - t[:, :1]
    c = SX.exact_solve_k1(t[0], wp[0], K)
    for a in range(4):
        for j in range(K):
            v = SE.eval_state_mp(c[0, a], 0.25, j)
            want = mp.mpf(float(wp[0, 0, a])) if j == 0 else 0
            assert abs(v - want) <= 1e-13 * max(1.0, abs(wp[0, 0, a])), (a, j, v)
        assert abs(SE.eval_state_mp(c[0, a], t[0, 1] - t[0, 0], 0) - float(wp[0, 1, a])) <= 1e-13 * 5
    c0 = SX.exact_solve_k1(t[0] - 0.25, wp[0], K)
    assert norm_rel(c, c0) > 1e-3


# ---------------------------------------------------------------------------
# against the order-9 fixture: both are 60-digit solutions rounded once
# ---------------------------------------------------------------------------
ORDER9_CASES = ["m2", "m3", "m4", "m5", "m6", "m7", "m8", "m9", "m10", "m10s", "m10q", "m12", "m16", "m20", "m20s"]


@pytest.fixture(scope="module")
def gold9():
    return np.load(os.path.join(GOLDEN_DIR, "order9_golden.npz"))


@pytest.mark.parametrize("name", ORDER9_CASES)
def test_order9_fixture_within_one_ulp(gold9, name):
    """Measured: every element whose exact value is not 0 is bit for bit the fixture's, in all 15 cases.  The elements
    that differ at all (m2..m9, m10, m12, m16, m20: 10..167 per case; none in m10s, m10q, m20s) are rest-start
    coefficients with the exact value 0, where each solve keeps its own residue (at most 4e-58 of the path's largest coefficient)."""
    wp, t, ref = gold9[name + "_wp"], gold9[name + "_t"], gold9[name + "_coef"]
    got = SX.exact_batch_k1(wp, t, 5)
    # one unit in the last place of the recorded value -- or, where the exact value is 0 (the rest start's c_1..c_4)
    # and each 60-digit solve leaves its own rounding residue of some 1e-57, the floor of the 60-digit arithmetic:
    # 1e-50 of the path's largest coefficient
    floor = 1e-50 * np.abs(ref).max(axis=(1, 3), keepdims=True)
    differ = got != ref
    print(f"order9_golden {name}: {int(differ.sum())} of {ref.size} elements differ, "
          f"{int((differ & (np.abs(ref) > floor)).sum())} of them above the 60-digit floor (the others are residues of "
          f"an exact 0), norm_rel {norm_rel(got, ref):.1e}")
    ulp = np.spacing(np.abs(ref))
    assert (np.abs(got - ref) <= ulp + floor).all(), (name, float((np.abs(got - ref) / (ulp + floor)).max()))


# ---------------------------------------------------------------------------
# against the reference's own outputs (dense fp64 LU, numpy.linalg.solve)
# ---------------------------------------------------------------------------
SINGLE = ["cfg1", "testdata", "m1", "m2", "t0quirk", "path49"]
BATCH = ["cfg2", "cfg2s", "m20", "m3"]


@pytest.mark.parametrize("name", SINGLE + BATCH)
def test_reference_outputs(golden, name):
    wp, t, ref = golden[name + "_wp"], golden[name + "_t"], golden[name + "_coef"]
    if name in SINGLE:
        wp, t, ref = wp[None], t[None], ref[None]
    if name == "t0quirk":
        assert t[0, 0] != 0
    got = SX.exact_batch_k1(wp, t, 4)
    err = norm_rel(ref, got)
    print(f"ref_golden {name}: reference's dense solve vs 60 digits {err:.1e}")
    assert err <= ORACLE_BAR, (name, err)


# ---------------------------------------------------------------------------
# against the dense oracle on the grids of the GPU test
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order,M", [(7, 10), (7, 24), (9, 10), (9, 20)])
@pytest.mark.parametrize("grid", ["even", "uneven"])
def test_dense_oracle_on_the_gpu_tests_grids(order, M, grid):
    import msnap_oracle as O
    wp, t = SC.inputs(order, M, grid)
    assert wp.shape[0] == 9 and t[SC.RAISED, 0] == 0.25 and (np.delete(t[:, 0], SC.RAISED) == 0).all()
    exact = SX.exact_batch_k1(wp, t, SC.khalf(order))
    dense, _ = O.solve_batch_fast(wp, t, ncoef=order + 1)
    err, at = SX.norm_rel_at(dense, exact)
    seg, sat = SX.seg_scaled(dense, exact, np.diff(t, axis=1))
    print(f"order {order} M {M} {grid}: dense oracle vs 60 digits norm_rel {err:.1e} at {at}, segment-scaled {seg:.1e} "
          f"at {sat}")
    assert err == norm_rel(dense, exact)
    assert err <= ORACLE_BAR, (order, M, grid, err)


# ---------------------------------------------------------------------------
# the table against the launcher
# ---------------------------------------------------------------------------
def _consts():
    csrc = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("msnap_solve.hip", "msnap_sweep.h", "msnap_internal.h"))
    out = {}
    for name in ("kTwistMaxSeg", "kTwistMaxSeg9", "kTwinMaxSeg", "kTwinMaxSeg7", "kRegMaxSeg", "kRegMaxSeg2", "kTrPitch"):
        m = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert len(m) == 1, name
        out[name] = int(m[0])
    m = re.findall(r"constexpr\s+size_t\s+kMaxLdsBytes\s*=\s*(\d+)\s*\*\s*1024\s*;", text)
    assert len(m) == 1
    out["kMaxLdsBytes"] = int(m[0]) * 1024
    return out, text


def test_table_covers_exactly_the_launchers_ranges():
    k, text = _consts()
    seg = lambda fam, order: sorted(c.M for c in SC.CASES if c.family == fam and c.order == order and not c.shared)  # noqa: E731
    assert seg("twist", 7) == list(range(2, k["kTwistMaxSeg"] + 1))
    assert seg("twist", 9) == list(range(2, k["kTwistMaxSeg9"] + 1))
    assert seg("twin", 7) == list(range(4, k["kTwinMaxSeg7"] + 1))
    assert seg("twin", 9) == list(range(4, k["kTwinMaxSeg"] + 1))
    for order in (7, 9):
        assert seg("reg", order) == list(range(2, k["kRegMaxSeg2"] + 1))
        for c in SC.CASES:
            if c.family == "reg" and c.order == order:
                assert c.kernel.endswith(", %d>" % (k["kRegMaxSeg"] if c.M <= k["kRegMaxSeg"] else k["kRegMaxSeg2"]))
        assert seg("generic", order) == list(SC.GENERIC_SEG[order])
        assert seg("generic", order)[0] == 1 and seg("generic", order)[1] == k["kRegMaxSeg2"] + 1
    # the launcher's switches hold one case label per instance of the table, and no other
    assert len(re.findall(r"MSNAP_TWIST_EXACT\((\d+)\)", text)) == len(seg("twist", 7)) + len(seg("twist", 9))
    assert len(re.findall(r"MSNAP_TWIN\((\d+)\)", text)) == len(seg("twin", 7)) + len(seg("twin", 9))
    # the twin lower bound and the twist lower bound as the launcher states them
    assert re.search(r"M >= 4 && M <= \(K == 5 \? kTwinMaxSeg : kTwinMaxSeg7\)", text)
    assert re.search(r"M >= 2 && M <= \(K == 4 \? kTwistMaxSeg : kTwistMaxSeg9\)", text)
    assert re.search(r"if \(M >= 2 && M <= kRegMaxSeg2\)", text)


def test_global_scratch_threshold_is_the_tables():
    k, _ = _consts()
    for order in (7, 9):
        gs = [M for M in range(k["kRegMaxSeg2"] + 1, 200)
              if SC.scratch_bytes(order, M, k["kTrPitch"]) > k["kMaxLdsBytes"]]
        assert gs[0] == SC.GS_MIN_SEG[order] and gs == list(range(gs[0], 200))
        for c in SC.CASES:
            if c.order == order and c.family in ("generic", "generic-GS"):
                assert c.kernel == SC.generic_name(order, c.M, k["kMaxLdsBytes"])
                assert c.kernel.endswith("true>") == (c.M >= SC.GS_MIN_SEG[order])
        gsc = [c for c in SC.CASES if c.order == order and c.family == "generic-GS"]
        assert len(gsc) == 1 and gsc[0].M == SC.GS_MIN_SEG[order] and gsc[0].n == SC.N_DRONES_GS


def test_table_shape():
    ids = [SC.case_id(c) for c in SC.CASES]
    assert len(set(ids)) == len(ids)
    for c in SC.CASES:
        assert set(c.opts) <= {"no_twist", "no_twin"}
        assert c.waves == ((1, 2, 4) if c.family == "twist" else (0,))
        assert c.n == (SC.N_DRONES_GS if c.family == "generic-GS" else SC.N_DRONES)
    shared = [(c.family, c.order, c.M) for c in SC.CASES if c.shared]
    assert sorted(shared) == sorted((f, o, SC.SHARED_SEG) for f in ("twist", "twin", "reg") for o in (7, 9))
    for order, M, grid, want in [(7, 24, "uneven", 1e-9), (7, 25, "uneven", 1e-6), (9, 20, "uneven", 2e-8),
                                 (9, 21, "uneven", 1e-6), (7, 49, "even", 1e-9), (9, 40, "even", 1e-9),
                                 (9, 10, "shared", 1e-9)]:
        assert SC.bar(order, M, grid)[0] == want
