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
    assert len(names) == 6 == len(scratch) == len(vgpr) == len(agpr)
    assert sum("clearance_lane_kernel" in n for n in names) == 2
    assert scratch == [0] * 6 and agpr == [0] * 6 and max(vgpr) <= 256, list(zip(names, vgpr, agpr, scratch))
