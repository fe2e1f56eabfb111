"""Pairwise clearance without a GPU: the exact reference against a dense high-precision sampling, the NumPy restatement
against the exact reference, the gap and uncertain-set logic of swarm.certify_clearance with a stand-in compute object,
the argument checks of the C entries, and the build checks on the new object."""
import ctypes
import os
import re
import subprocess
import sys

import mpmath
import numpy as np
import pytest

import c_oracle
from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_cases as CC  # noqa: E402
import clearance_exact as CE  # noqa: E402

from drone_path_planning_python_amd import swarm, synthetic  # noqa: E402

OBJ = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_clearance.o")
LLVM = "/opt/rocm/lib/llvm/bin"


def crossing_pair():
    """Two rest-to-rest drones crossing at right angles, 2 m in 1.1 s each: both at the origin at t = 0.55 s."""
    wp = np.zeros((2, 2, 4))
    wp[0, :, 0] = [-1.0, 1.0]
    wp[1, :, 1] = [-1.0, 1.0]
    return wp, np.array([0.0, 1.1])


@pytest.fixture(scope="module")
def solved():
    wp, t = synthetic.swarm(7003, 4, 3)
    coef, dur, info, _ = c_oracle.solve_batch(wp, t)
    assert not info.any()
    return coef, dur


def test_exact_reference_against_dense_sampling(solved):
    coef, dur = solved
    for a, b in ((0, 1), (2, 3)):
        D, t, W = CE.exact_clearance(coef[a], dur[a], coef[b], dur[b])
        assert 0 <= t <= W and float(W) == min(CE.knots(dur[a])[-1], CE.knots(dur[b])[-1])
        assert abs(CE.exact_distance_at(coef[a], dur[a], coef[b], dur[b], t) - D) <= mpmath.mpf(10) ** -40
        n = 4000
        dense = min(CE.exact_distance_at(coef[a], dur[a], coef[b], dur[b], W * k / n) for k in range(n + 1))
        # the minimum is not above any sample, and a grid of step W / n misses it by at most (speed sum) * W / (2 n)
        assert D <= dense
        assert dense - D <= 40.0 * float(W) / (2 * n)


def test_fp64_restatement_meets_the_contract_against_the_exact_reference(solved):
    coef, dur = solved
    pairs = np.array([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)])
    md, tm, lower = CE.fp64_clearance(coef, dur, pairs)
    md2, tm2, lower2 = CE.fp64_clearance(coef, dur, pairs[:, ::-1])
    assert np.array_equal(md, md2) and np.array_equal(tm, tm2) and np.array_equal(lower, lower2)
    cands = CE.candidate_intervals(coef, dur, pairs)
    for k, (a, b) in enumerate(pairs):
        D, _, W = CE.exact_clearance(coef[a], dur[a], coef[b], dur[b], cands[k])
        assert not CE.contract_violations(md[k], lower[k], D), (a, b)
        assert 0 <= tm[k] <= float(W)


def test_the_crossing_pair_is_missed_by_the_samples_and_found_by_the_walk():
    wp, t = crossing_pair()
    coef, dur, info, _ = c_oracle.solve_batch(wp, t)
    assert not info.any()
    S = swarm.default_sample_count(1.1, synthetic.SAMPLE_DT)
    pos = c_oracle.sample_positions(coef, dur, synthetic.SAMPLE_DT, S)
    smd, _, shit = c_oracle.formation_collide(pos, 0.1)
    print("sampled minimum distance of the crossing pair:", smd)
    assert not shit.any() and (smd >= 0.25).all() and (smd <= 0.30).all()
    D, tD, _ = CE.exact_clearance(coef[0], dur[0], coef[1], dur[1])
    assert D <= 1e-12 and abs(tD - 0.55) <= 1e-9
    md, tm, lower = CE.fp64_clearance(coef, dur, np.array([[0, 1]]))
    assert md[0] < 1e-6 and not CE.contract_violations(md[0], lower[0], D)


# ---------------------------------------------------------------------------------------------- twins of the GPU edge tests
# tests/test_clearance_edges_gpu.py's families through the restatement (CE.RestatedContext) on the C oracle's
# coefficients, a dozen pairs per family: the exact reference and the restatement stay pinned without a GPU.
RESTATED = {8: CE.RestatedContext(7), 10: CE.RestatedContext(9)}


def oracle_solve(wp, t, nc):
    coef, dur, info, _ = c_oracle.solve_batch(wp, t, ncoef=nc)
    assert not info.any()
    return coef, dur


@pytest.fixture(scope="module")
def far_origin():
    return {nc: CC.far_origin(RESTATED[nc], oracle_solve, nc, n_pairs=n) for nc, n in ((8, 8), (10, 3))}


@pytest.mark.parametrize("nc", [8, 10])
def test_twin_far_from_the_origin(far_origin, nc):
    for name in ("y-1000", "all+1000", "x-5000", "all+5000", "all+1e5"):
        CC.check_far(RESTATED[nc], far_origin[nc], name)
    if nc == 8:
        CC.check_loner(RESTATED[nc], far_origin[nc])


def test_the_allowance_without_its_coordinate_term_fails_far_from_the_origin():
    """The header's earlier formula (1e-13 relative + 1e-13 m, R = 0) on the case that led to the coordinate term:
    synthetic.swarm(7003, 6, 4) moved by +1e5 m.  The rounding of the attained value alone is beyond it."""
    coef, dur = oracle_solve(*synthetic.swarm(7003, 6, 4), 8)
    coef = CC.moved(CC.quantised(coef), (1e5,) * 3)
    pairs = CC.all_pairs(6)[:6]
    md, tm, lower = CE.fp64_clearance(coef, dur, pairs)
    off = [abs(md[k] - float(CE.exact_distance_at(coef[a], dur[a], coef[b], dur[b], tm[k]))) for k, (a, b) in enumerate(pairs)]
    print("|min_dist - exact distance at t_min|:", off)
    assert max(off) > 10 * (CE.REL_ROUND * md.max() + CE.ABS_ROUND)
    R = max(CE.pair_R(coef[a], dur[a], coef[b], dur[b]) for a, b in pairs)
    assert max(off) < CE.round_terms(R)


def test_contract_violations_without_R_reports_the_far_case():
    """The far family's swarm moved by +1e5 m, order 7, pair (1, 5): with R = 0 -- the header's earlier formula --
    contract_violations reports min_dist below D (D - min_dist = 1.6e-11 m); with the pair's R it reports nothing."""
    coef, dur = CC.far_base(oracle_solve, 8)
    coef = CC.moved(coef, CC.OFFSETS["all+1e5"])
    pairs = np.array([(1, 5), (0, 4)])
    md, tm, lower = CE.fp64_clearance(coef, dur, pairs)
    cands = CE.candidate_intervals(coef, dur, pairs)
    D, _, _ = CE.exact_clearance(coef[1], dur[1], coef[5], dur[5], cands[0])
    print("min_dist", md[0], "D", float(D), "D - min_dist", float(D) - md[0])
    bad = CE.contract_violations(md[0], lower[0], D)
    assert len(bad) == 1 and "below D" in bad[0]
    assert not CE.contract_violations(md[0], lower[0], D, R=CE.pair_R(coef[1], dur[1], coef[5], dur[5]))


@pytest.mark.parametrize("scale_t,scale_w", CC.SCALES)
def test_twin_extreme_scales(scale_t, scale_w):
    coef, dur = CC.scaled(oracle_solve, 8, scale_t, scale_w)
    CE.check_contract(RESTATED[8], coef, dur, CC.all_pairs(6)[:3], with_R=True)


@pytest.mark.parametrize("nc", [8, 10])
def test_twin_crossing_of_2000_m(nc):
    for total in (11.0, 1.1):
        CC.check_crossing(RESTATED[nc], oracle_solve, nc, total)


def test_twin_long_paths():
    for unequal in (False, True):
        coef, dur = CC.long_paths(oracle_solve, 8, 49, unequal=unequal)
        CE.check_contract(RESTATED[8], coef, dur, CC.all_pairs(6)[:3], with_R=True)
    coef, dur = CC.stacked(oracle_solve, 8, 256)
    CE.check_contract(RESTATED[8], coef, dur, CC.all_pairs(3), with_R=True)
    for m in (12, 20):
        coef, dur = CC.long_paths(oracle_solve, 10, m)
        CE.check_contract(RESTATED[10], coef, dur, CC.all_pairs(6)[:2], with_R=True)


@pytest.mark.parametrize("nc", [8, 10])
def test_twin_knots_degenerate_differences_and_window_ends(nc):
    ctx = RESTATED[nc]
    for kind in ("ulp", "rel", "short") if nc == 8 else ("ulp",):
        CC.check_knots(ctx, oracle_solve, nc, kind)
    CC.check_copies(ctx, oracle_solve, nc)
    for m in (1, 3):
        CC.check_hovering(ctx, nc, m)
    CC.check_ends_by_hand(ctx, nc)
    if nc == 8:                                   # (the exact reference at degree 18 costs four times as much)
        CC.check_hover_against_moving(ctx, oracle_solve, nc)
        CC.check_ends_solved(ctx, oracle_solve, nc)


def test_twin_the_depth_cap_is_met_at_order_9_and_lower_stays_valid():
    for dz in (0.0, 1e-7):
        capped, nodes = CC.check_caps(RESTATED[10], oracle_solve, 10, dz)
        assert capped and nodes == 2 * CE.MAX_DEPTH + 1
        capped, nodes = CC.check_caps(RESTATED[8], oracle_solve, 8, dz)
        assert not capped and nodes == 2 * CE.MAX_DEPTH + 1       # closes at the last level: the most nodes found


# ---------------------------------------------------------------------------------------------- certify_clearance
def test_sample_gap():
    dt = 0.1
    assert swarm.sample_gap(dt, 100, [10.0]) == pytest.approx(0.1)           # default_sample_count stops at 9.9 s
    assert swarm.sample_gap(dt, 101, [10.0]) == pytest.approx(0.05)
    assert swarm.sample_gap(dt, 200, [10.0, 3.0]) == pytest.approx(0.05)
    assert swarm.sample_gap(dt, 200, [10.0, 3.07]) == pytest.approx(0.07)    # a sample beyond 3.07 s is extrapolated
    assert swarm.sample_gap(dt, 11, [1.1]) == pytest.approx(0.1)
    assert swarm.sample_gap(dt, 1, [0.5]) == pytest.approx(0.5)
    with pytest.raises(ValueError):
        swarm.sample_gap(0.0, 10, [1.0])


class FakeCompute:
    """Positions, peaks and exact answers handed in: what certify_clearance does with them."""

    def __init__(self, pos, speed, exact):
        import torch
        self.torch = torch
        self.pos, self.speed, self.exact = torch.from_numpy(pos), torch.from_numpy(speed), exact
        self.asked = None

    def sample(self, coef, dur, dt, n_samples):
        return self.pos

    def collide(self, pos_rows, row_offset, pos_all, radius, rows_t=None):
        torch = self.torch
        d = (pos_rows[:, None] - pos_all[None]).norm(dim=-1).amin(dim=-1)
        d.fill_diagonal_(float("inf"))
        md, partner = d.min(dim=1)
        return md, partner.to(torch.int32), (md < 2 * radius).to(torch.int32)

    def dynamic_peaks(self, coef, dur):
        torch = self.torch
        n = self.speed.shape[0]
        peak = torch.zeros((n, 4), dtype=torch.float64)
        peak[:, 0] = self.speed
        return peak, torch.zeros((n, 4), dtype=torch.float64), torch.zeros((n,), dtype=torch.int32)

    def pair_clearance(self, coef, dur, pairs):
        torch = self.torch
        self.asked = [tuple(p) for p in pairs.tolist()]
        md = torch.tensor([self.exact[p][0] for p in self.asked], dtype=torch.float64)
        lo = torch.tensor([self.exact[p][1] for p in self.asked], dtype=torch.float64)
        return md, torch.zeros_like(md), lo, torch.zeros((len(self.asked),), dtype=torch.int32)


def test_uncertain_set_and_result_of_certify_clearance():
    import torch
    S, dt, radius = 11, 0.1, 0.1
    x = np.array([0.0, 0.3, 0.55, 10.0, 10.9, 50.0])      # drones on a line, standing still in the samples
    pos = np.zeros((6, S, 3))
    pos[:, :, 0] = x[:, None]
    speed = np.array([1.0, 1.0, 0.2, 4.0, 4.0, 0.0])
    dur = torch.full((6, 2), 0.5, dtype=torch.float64)    # totals 1.0 s: 11 samples reach the end, gap = dt / 2
    coef = torch.zeros((6, 2, 4, 8), dtype=torch.float64)
    exact = {(0, 1): (0.15, 0.15), (1, 2): (0.25, 0.21), (3, 4): (0.5, 0.1), (0, 2): (0.5, 0.5)}
    fake = FakeCompute(pos, speed, exact)
    res = swarm.certify_clearance(fake, coef, dur, radius, dt, S)
    assert res.gap == pytest.approx(0.05)
    vmax = 4.0 * (1 + 2e-9)
    # cleared by sampling: d_i >= 2 r + (V_i + V_max) gap -- drones 0..2 (0.45, 0.45, 0.41 needed), 3 and 4 (0.6 needed
    # against 0.9) are cleared, 5 is far from everything
    assert res.cleared_by_sampling.tolist() == [False, False, False, True, True, True]
    assert res.n_uncertain == 3
    # kept among U: (0, 1) at 0.3 < 0.3 + ..., (1, 2) at 0.25 < 0.26; (0, 2) at 0.55 >= 0.2 + 1.2 * 0.05 = 0.26
    assert fake.asked == [(0, 1), (1, 2)] and res.pairs.dtype == torch.int32
    assert res.hit.tolist() == [True, True, False, False, False, False]
    assert res.undecided.tolist() == [False] * 6
    cl = res.certified_lower.numpy()
    assert cl[0] == 0.15 and cl[1] == 0.15 and cl[2] == pytest.approx(2 * radius)
    assert cl[3] == pytest.approx(0.9 - 2 * vmax * 0.05, rel=1e-8) and cl[3] >= 2 * radius
    assert cl[5] == pytest.approx(39.1 - vmax * 0.05, rel=1e-8)
    np.testing.assert_allclose(res.sampled_min_dist.numpy(), [0.3, 0.25, 0.25, 0.9, 0.9, 39.1], rtol=1e-14)
    # an undecided pair: lower < 2 r <= min_dist
    fake.exact[(1, 2)] = (0.25, 0.19)
    fake.exact[(0, 1)] = (0.31, 0.3)
    res = swarm.certify_clearance(fake, coef, dur, radius, dt, S)
    assert res.hit.tolist() == [False] * 6 and res.undecided.tolist() == [False, True, True, False, False, False]
    # one rank only; failed drones are refused
    with pytest.raises(NotImplementedError):
        swarm.certify_clearance(fake, coef, dur, radius, dt, S, world=2)
    with pytest.raises(ValueError):
        swarm.certify_clearance(fake, coef, dur, radius, dt, S, status=torch.tensor([0, 0, 1, 0, 0, 0]))


class RestatedCompute(FakeCompute):
    """The stand-in with positions from the C oracle's sampler, speed peaks from limits_exact.fp64_peaks and the
    NumPy restatement in place of msnap_pair_clearance."""

    def __init__(self, coef, dur, dt, n_samples):
        import limits_exact
        pos = c_oracle.sample_positions(coef, dur, dt, n_samples)
        super().__init__(pos, limits_exact.fp64_peaks(coef, dur)[:, 0], {})
        self.coef_np, self.dur_np = coef, dur

    def pair_clearance(self, coef, dur, pairs):
        torch = self.torch
        md, tm, lower = CE.fp64_clearance(self.coef_np, self.dur_np, pairs.numpy())
        return (torch.from_numpy(md), torch.from_numpy(tm), torch.from_numpy(lower),
                torch.zeros((len(md),), dtype=torch.int32))


def test_certify_clearance_on_the_awkward_swarm_every_pair():
    """tests/test_clearance_gpu.py's swarm of 12 at +5000 m through the stand-in: all 66 pairs against the exact
    reference."""
    import torch
    coef, dur = CC.awkward_swarm(oracle_solve)
    comp = RestatedCompute(coef, dur, CC.AWKWARD_DT, CC.AWKWARD_SAMPLES)
    res = swarm.certify_clearance(comp, torch.from_numpy(coef), torch.from_numpy(dur), CC.AWKWARD_RADIUS, CC.AWKWARD_DT,
                                  CC.AWKWARD_SAMPLES)
    CC.check_certified({k: getattr(res, k).numpy() for k in ("certified_lower", "hit", "undecided", "cleared_by_sampling",
                                                              "pairs")}, coef, dur)


# ---------------------------------------------------------------------------------------------- C entries, build
def test_argument_checks_without_a_device():
    from drone_path_planning_python_amd import _lib, context
    lib = _lib.load()
    assert lib.msnap_version() == 500
    assert context.ST_PAIR == 4
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        assert re.search(r"MSNAP_ST_PAIR\s*=\s*4\b", f.read())
    for fn in (lib.msnap_pair_clearance, lib.msnap_pair_clearance_device):
        assert fn(None, 1, 1, None, None, 1, None, None, None, None, None) == -1
        assert fn(None, 1, 1, None, None, 0, None, None, None, None, None) == -1      # no context: before the no-op


def _need_tools(*paths):
    if not all(os.path.exists(p) for p in paths) or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.skip("no object file / ROCm LLVM tools here")


def test_exec_check_and_latch_census_cover_the_new_object():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    assert OBJ in chk.DEFAULT_OBJS and len(chk.DEFAULT_OBJS) == 8
    _need_tools(OBJ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), OBJ], capture_output=True,
                       text=True)
    assert r.returncode == 0 and "none under a reduced exec mask" in r.stdout, r.stdout + r.stderr
    assert chk.lane_latches(OBJ) == {}       # every loop of the file is wave-uniform


def test_new_kernels_use_no_scratch_and_fit_the_register_file(tmp_path):
    _need_tools(OBJ)
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "clr.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", OBJ, str(tmp_path / "copy.o")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    vgpr = [int(x) for x in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    agpr = [int(x) for x in re.findall(r"\.agpr_count:\s+(\d+)", notes)]
    # 2 flags kernels, and a lane and a fold kernel per (order, CROSS): the pairwise and the cross entry
    assert len(names) == 10 == len(scratch) == len(vgpr) == len(agpr)
    lane = {n: v for n, v in zip(names, vgpr) if "pair_lane_kernel" in n}
    assert len(lane) == 4 and sum("pair_fold_kernel" in n for n in names) == 4
    assert scratch == [0] * 10 and agpr == [0] * 10 and max(vgpr) <= 256, list(zip(names, vgpr, agpr, scratch))
    # the occupancy steps the timings rest on: 3 waves per SIMD at order 7, 2 at order 9
    assert sum("pair_lane_kernelILi8E" in n for n in lane) == 2 == sum("pair_lane_kernelILi10E" in n for n in lane)
    assert all(v <= (160 if "ILi8E" in n else 196) for n, v in lane.items()), lane
