"""tests/solve_exact.py (the 60-digit K1 reference with the start-row quirk) against everything that already pins the
solve -- states_exact, the order-9 fixture, the reference's own outputs, the dense fp64 oracle -- and
tests/solve_cases.py (the table of kernel instances) against the launcher's decision, executed on the host
(csrc/msnap_solve_plan.h through tests/c_abi/solve_plan_dump.cpp).  No GPU.

The 1e-11 bars are bars on the DENSE fp64 REFERENCE (a pivoted LU of the collocation system), not on a kernel: ten
times the worst 1.0e-12 measured for it against 60 digits on the draw of tools/solve_stress.py (order 9, 10 segments;
order 7 stays below 1e-13)."""
import os
import re
import shutil
import subprocess
from collections import namedtuple

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
# the table against the launcher: its decision (csrc/msnap_solve_plan.h, plan_solve) is EXECUTED on the host by
# tests/c_abi/solve_plan_dump.cpp -- for 256 CUs, over orders x drones x segments x option sets
# ---------------------------------------------------------------------------
CSRC = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
PlanRow = namedtuple("PlanRow", "order n m opts n_cu family name instance waves tiles grid block lds slab")
PLAN_DRONES = (1, 3, 7, 8, 9, 16, 17, 255, 256, 257, 2048, 2049, 8192, 8193, 65536, 65537, 1048576)
PLAN_OPTS = ("", "no_twist", "no_twist,no_twin", "twist_waves=1", "twist_waves=2", "twist_waves=4", "twist_max_drones=1",
             "twist_max_drones=4096", "twin_max_drones=1", "twin_max_drones=1048576", "solve_grid_waves=1",
             "solve_grid_waves=3", "no_twist,solve_grid_waves=3", "no_twist,no_twin,solve_grid_waves=3")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """(order, drones, segments, option set) -> PlanRow, and the constants of the dump's first line under "consts" """
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ here")
    exe = str(tmp_path_factory.mktemp("solve_plan") / "solve_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "solve_plan_dump.cpp"), "-o", exe], check=True, capture_output=True)
    lines = subprocess.run([exe, "256"], check=True, capture_output=True, text=True).stdout.splitlines()
    head = lines[0].split("\t")
    assert head[0] == "consts"
    out = {"consts": {k: int(v) for k, v in (f.split("=") for f in head[1:])}}
    for ln in lines[1:]:
        f = ln.split("\t")
        assert len(f) == len(PlanRow._fields), ln
        r = PlanRow(int(f[0]), int(f[1]), int(f[2]), f[3], int(f[4]), f[5], f[6], f[7], *map(int, f[8:]))
        assert (r.order, r.n, r.m, r.opts) not in out
        out[(r.order, r.n, r.m, r.opts)] = r
    # the sweep the tests below rely on: every option set up to 64 segments, the default ones up to 200
    assert len(out) - 1 == 2 * len(PLAN_DRONES) * (len(PLAN_OPTS) * 64 + 136)
    assert all((o, n, 64, s) in out for o in (7, 9) for n in PLAN_DRONES for s in PLAN_OPTS)
    return out


def _labels(c):
    """the option sets of the dump under which the GPU test runs a case"""
    return ["", "twist_waves=1", "twist_waves=2", "twist_waves=4"] if c.family == "twist" else [",".join(c.opts)]


def test_table_covers_exactly_the_launchers_ranges(plan):
    seg = lambda fam, order: sorted(c.M for c in SC.CASES if c.family == fam and c.order == order and not c.shared)  # noqa: E731
    for order in (7, 9):
        for fam in ("twist", "twin", "reg"):
            cases = [c for c in SC.CASES if c.family == fam and c.order == order]
            assert len({(c.opts, c.n) for c in cases}) == 1
            for label in _labels(cases[0]):
                sent = [M for M in range(1, 65) if plan[(order, cases[0].n, M, label)].family == fam]
                assert seg(fam, order) == sent, (fam, order, label)
        assert seg("twist", order) == list(SC.TWIST_SEG[order]) and seg("twin", order) == list(SC.TWIN_SEG[order])
        assert seg("reg", order) == list(SC.REG_SEG[order])
        # the <K, 10> / <K, 20> split of the reg family falls at kRegMaxSeg
        assert SC.REG_SPLIT == plan["consts"]["kRegMaxSeg"]
        K = SC.khalf(order)
        for c in SC.CASES:
            if c.family == "reg" and c.order == order:
                want = "msnap::solve_kernel_reg<%d, %d>" % (K, SC.REG_SPLIT if c.M <= SC.REG_SPLIT else SC.REG_SEG[order][-1])
                assert plan[(order, c.n, c.M, ",".join(c.opts))].name == want == c.kernel
        # the rolled kernel: one segment, and everything behind the reg family's range
        assert seg("generic", order) == list(SC.GENERIC_SEG[order])
        rolled = [M for M in range(1, 65) if plan[(order, SC.N_DRONES, M, "no_twist,no_twin")].family == "rolled"]
        assert rolled == [1] + list(range(SC.REG_SEG[order][-1] + 1, 65))
        assert seg("generic", order)[0] == 1 and seg("generic", order)[1] == rolled[1]
        for c in SC.CASES:
            if c.order == order and c.family in ("generic", "generic-GS"):
                assert plan[(order, c.n, c.M, ",".join(c.opts))].family == "rolled"


def test_every_case_reports_the_plans_kernel_name(plan):
    for c in SC.CASES:
        for label in _labels(c):
            r = plan[(c.order, c.n, c.M, label)]
            assert r.name == c.kernel, (SC.case_id(c), label)
            assert r.family == {"generic": "rolled", "generic-GS": "rolled"}.get(c.family, c.family)
            if label.startswith("twist_waves="):      # the wave count the GPU test asks for is the instance's
                w = int(label.split("=")[1])
                assert r.waves == w and r.instance == c.kernel[len("msnap::"):-1] + ", %d>" % w
            elif c.family != "twist":
                assert r.instance == c.kernel[len("msnap::"):]


def test_global_scratch_threshold_is_the_tables(plan):
    for order in (7, 9):
        for n in PLAN_DRONES:
            gs = [M for M in range(1, 201) if plan[(order, n, M, "")].slab > 0]
            assert gs[0] == SC.GS_MIN_SEG[order] and gs == list(range(gs[0], 201)), (order, n)
        for label in PLAN_OPTS:      # no other option set moves a slab below 65 segments either
            for n in PLAN_DRONES:
                assert [M for M in range(1, 65) if plan[(order, n, M, label)].slab > 0] == \
                    list(range(SC.GS_MIN_SEG[order], 65))
        for c in SC.CASES:
            if c.order == order and c.family in ("generic", "generic-GS"):
                r = plan[(order, c.n, c.M, ",".join(c.opts))]
                assert c.kernel == SC.generic_name(order, c.M, plan["consts"]["kMaxLdsBytes"]) == r.name
                assert c.kernel.endswith("true>") == (c.M >= SC.GS_MIN_SEG[order]) == (r.slab > 0)
        gsc = [c for c in SC.CASES if c.order == order and c.family == "generic-GS"]
        assert len(gsc) == 1 and gsc[0].M == SC.GS_MIN_SEG[order] and gsc[0].n == SC.N_DRONES_GS


def test_plan_geometry_on_every_line(plan):
    c = plan["consts"]
    for key, r in plan.items():
        if key == "consts":
            continue
        assert 0 <= r.lds <= c["kMaxLdsBytes"], r
        assert 1 <= r.grid <= r.tiles, r
        assert r.block == c["kWave"] * r.waves and r.waves in (1, 2, 4), r
        assert r.tiles == -(-r.n // (8 if r.family in ("twist", "twin") else 16)), r
        assert (r.slab > 0) == r.name.endswith("true>"), r
        if r.family == "twist":
            # one workgroup per 8-drone tile under every solve_grid_waves / twist_max_drones setting: the kernel has no
            # tile loop (tests/test_twist_waves_gpu.py checks the same on the GPU)
            assert r.grid == -(-r.n // 8), r
        else:
            assert r.waves == 1, r
    twist = {r.opts for k, r in plan.items() if k != "consts" and r.family == "twist"}
    assert {"", "solve_grid_waves=1", "solve_grid_waves=3", "twist_max_drones=1", "twist_max_drones=4096"} <= twist


def test_code_object_holds_exactly_the_instances_the_plan_names(plan, tmp_path):
    """The set of solve kernels in msnap_solve.o's gfx950 code object is what the plan can name over both orders, 1..64
    segments, the dump's batch sizes and option sets (wave counts 1, 2 and 4 among them): no instance the launcher
    cannot reach, none it would miss."""
    obj = os.path.join(CSRC, "msnap_solve.o")
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(obj) or not all(os.path.exists(t) for t in tools):
        pytest.skip("no object file / ROCm LLVM tools here")
    fat, co = str(tmp_path / "fat"), str(tmp_path / "co")
    subprocess.run([tools[0], "--dump-section=.hip_fatbin=" + fat, obj, str(tmp_path / "copy.o")], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co], check=True)
    syms = subprocess.run([tools[2], "--symbols", "--demangle", co], check=True, capture_output=True, text=True).stdout
    built = set(re.findall(r"\bFUNC\b.*\bvoid msnap::(solve_kernel(?:_twist|_twin|_reg)?<[^>]*>)\(", syms))
    named = {r.instance for k, r in plan.items() if k != "consts" and r.m <= 64}
    assert built == named, (sorted(built - named), sorted(named - built))
    assert len(built) == sum(3 * len(SC.TWIST_SEG[o]) + len(SC.TWIN_SEG[o]) + 2 + 2 for o in (7, 9)) == 144


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
