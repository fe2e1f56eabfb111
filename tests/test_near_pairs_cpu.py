"""Near pairs without a GPU: the NumPy reference (tests/near_pairs_ref.py) against swarm.uncertain_pairs, the argument
checks of the C entries, the header, certify_clearance through a stand-in compute object with and without `near_pairs`,
and the build checks on the new object."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import c_oracle
from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_cases as CC  # noqa: E402
import clearance_exact as CE  # noqa: E402
import near_pairs_ref as NP  # noqa: E402

from drone_path_planning_python_amd import swarm  # noqa: E402

OBJ = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_pairs.o")
COLLIDE_OBJ = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_collide.o")
LLVM = "/opt/rocm/lib/llvm/bin"


def test_reference_against_uncertain_pairs_on_a_seeded_swarm():
    import torch
    pos, speed = NP.box_swarm(11, 90, 13)
    radius = 0.5 * NP.base_for(pos, speed, frac=0.05)
    pairs, dist, band = NP.near_pairs(pos, 2.0 * radius, speed, NP.GAP, swarm.COMPARE_MARGIN)
    assert band == [] and 100 < len(pairs) < 400
    idx = torch.arange(90)
    want = swarm.uncertain_pairs(torch.from_numpy(pos), idx, torch.from_numpy(speed), radius, NP.GAP, torch, budget=9000)
    assert want.dtype == torch.int32 and np.array_equal(want.numpy(), pairs)      # same list, same order
    assert (pairs[:, 0] < pairs[:, 1]).all()
    key = pairs[:, 0].astype(np.int64) * 90 + pairs[:, 1]
    assert (np.diff(key) > 0).all()
    # a subset with global indices, as certify_clearance uses it
    sub = np.array([3, 4, 10, 11, 40, 41, 42, 77, 80, 89])
    want = swarm.uncertain_pairs(torch.from_numpy(pos[sub]), torch.from_numpy(sub), torch.from_numpy(speed[sub]),
                                 2.0 * radius, NP.GAP, torch)
    local, _, band = NP.near_pairs(pos[sub], 4.0 * radius, speed[sub], NP.GAP, swarm.COMPARE_MARGIN)
    assert band == [] and len(local) and np.array_equal(want.numpy(), sub[local])


def test_reference_ignores_non_finite_samples():
    pos, speed = NP.box_swarm(12, 9, 5)
    full, _, _ = NP.near_pairs(pos, 10.0)
    assert len(full) == 36
    pos[2] = np.nan
    pos[5, 1:3] = np.nan
    pairs, dist, _ = NP.near_pairs(pos, 10.0)
    assert len(pairs) == 28 and not (pairs == 2).any() and (pairs == 5).sum() == 7 and np.isfinite(dist).all()
    speed[4] = np.nan
    pairs, _, _ = NP.near_pairs(pos, 10.0, speed, NP.GAP)
    assert len(pairs) == 21 and not (pairs == 4).any()


def test_argument_checks_without_a_device():
    from drone_path_planning_python_amd import _lib
    lib = _lib.load()
    assert lib.msnap_version() == 500
    buf = (ctypes.c_double * 64)()
    out = (ctypes.c_int32 * 64)()
    found = ctypes.c_longlong(-7)
    p, o, f = ctypes.addressof(buf), ctypes.addressof(out), ctypes.addressof(found)
    nan = float("nan")
    for fn in (lib.msnap_formation_near_pairs, lib.msnap_formation_near_pairs_device):
        # no context: before everything else, the no-op shapes included
        assert fn(None, 4, 2, p, 1.0, None, 0.0, 0.0, 8, o, None, f) == -1
        assert fn(None, 0, 2, p, 1.0, None, 0.0, 0.0, 0, None, None, f) == -1
        assert fn(None, 1, 1, p, 1.0, None, 0.0, 0.0, 0, None, None, f) == -1
        # and every invalid argument is refused without one as well
        assert fn(None, 4, 2, None, 1.0, None, 0.0, 0.0, 8, o, None, f) == -1          # pos
        assert fn(None, 4, 2, p, 1.0, None, 0.0, 0.0, 8, o, None, None) == -1          # n_found
        assert fn(None, -1, 2, p, 1.0, None, 0.0, 0.0, 8, o, None, f) == -1
        assert fn(None, 4, 0, p, 1.0, None, 0.0, 0.0, 8, o, None, f) == -1
        assert fn(None, 4, 2, p, 1.0, None, 0.0, 0.0, -1, o, None, f) == -1
        assert fn(None, 4, 2, p, 1.0, None, 0.0, 0.0, 8, None, None, f) == -1          # pairs NULL, max_pairs > 0
        assert fn(None, 4, 2, p, nan, None, 0.0, 0.0, 8, o, None, f) == -1
        assert fn(None, 4, 2, p, 1.0, None, nan, 0.0, 8, o, None, f) == -1
        assert fn(None, 4, 2, p, 1.0, None, 0.0, nan, 8, o, None, f) == -1
        assert fn(None, 16385, 2, p, 1.0, None, 0.0, 0.0, 8, o, None, f) == -1
    assert found.value == -7


def test_header_declares_both_entries():
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        text = f.read()
    for name in ("msnap_formation_near_pairs", "msnap_formation_near_pairs_device"):
        assert re.search(rf"\bint {name}\(msnap_ctx \*ctx, int n_drones, int n_samples, const double \*pos,", text)
    assert "16384" in text[text.index("near pairs"):text.index("int msnap_formation_near_pairs(")]
    from drone_path_planning_python_amd import _lib
    for name in ("msnap_formation_near_pairs", "msnap_formation_near_pairs_device"):
        assert len(_lib.SIGNATURES[name][1]) == 12 and _lib.SIGNATURES[name][1][8] is ctypes.c_longlong


# ------------------------------------------------------------------------------ certify_clearance through stand-ins
class FakeCompute:
    """tests/test_clearance_cpu.py's stand-in restated: positions, peaks and exact answers handed in.  No near_pairs."""

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


class RestatedCompute(FakeCompute):
    """Positions from the C oracle's sampler, peaks from limits_exact.fp64_peaks, the NumPy restatement of K9."""

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


def with_near_pairs(cls):
    """The stand-in with DeviceCompute's near_pairs, backed by the reference."""
    class WithNearPairs(cls):
        calls = 0

        def near_pairs(self, pos, base, speed=None, gap=0.0, margin=0.0):
            torch = self.torch
            type(self).calls += 1
            pairs, dist, band = NP.near_pairs(pos.numpy(), base, None if speed is None else speed.numpy(), gap, margin)
            assert band == []
            return torch.from_numpy(pairs), torch.from_numpy(dist)
    return WithNearPairs


def same_result(a, b):
    import torch
    assert a.pairs.dtype == b.pairs.dtype == torch.int32 and a.pairs.shape == b.pairs.shape
    for k in ("pairs", "hit", "undecided", "certified_lower", "cleared_by_sampling", "pair_min_dist", "pair_lower"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def line_of_six():
    S = 11
    x = np.array([0.0, 0.3, 0.55, 10.0, 10.9, 50.0])      # drones on a line, standing still in the samples
    pos = np.zeros((6, S, 3))
    pos[:, :, 0] = x[:, None]
    speed = np.array([1.0, 1.0, 0.2, 4.0, 4.0, 0.0])
    exact = {(0, 1): (0.15, 0.15), (1, 2): (0.25, 0.21), (3, 4): (0.5, 0.1), (0, 2): (0.5, 0.5)}
    return pos, speed, exact, S


def test_certify_clearance_takes_near_pairs_where_the_compute_object_has_it():
    import torch
    pos, speed, exact, S = line_of_six()
    dur = torch.full((6, 2), 0.5, dtype=torch.float64)
    coef = torch.zeros((6, 2, 4, 8), dtype=torch.float64)
    plain = FakeCompute(pos, speed, exact)
    cls = with_near_pairs(FakeCompute)
    new = cls(pos, speed, exact)
    a = swarm.certify_clearance(plain, coef, dur, 0.1, 0.1, S)
    b = swarm.certify_clearance(new, coef, dur, 0.1, 0.1, S)
    assert cls.calls == 1 and new.asked == plain.asked == [(0, 1), (1, 2)]
    same_result(a, b)
    # pair_filter="torch" bypasses the method
    c = swarm.certify_clearance(new, coef, dur, 0.1, 0.1, S, pair_filter="torch")
    assert cls.calls == 1
    same_result(a, c)
    with pytest.raises(ValueError):
        swarm.certify_clearance(new, coef, dur, 0.1, 0.1, S, pair_filter="numpy")


def test_certify_clearance_on_the_awkward_swarm_both_filters():
    import torch

    def oracle_solve(wp, t, nc):
        coef, dur, info, _ = c_oracle.solve_batch(wp, t, ncoef=nc)
        assert not info.any()
        return coef, dur
    coef, dur = CC.awkward_swarm(oracle_solve)
    args = (torch.from_numpy(coef), torch.from_numpy(dur), CC.AWKWARD_RADIUS, CC.AWKWARD_DT, CC.AWKWARD_SAMPLES)
    a = swarm.certify_clearance(RestatedCompute(coef, dur, CC.AWKWARD_DT, CC.AWKWARD_SAMPLES), *args)
    cls = with_near_pairs(RestatedCompute)
    b = swarm.certify_clearance(cls(coef, dur, CC.AWKWARD_DT, CC.AWKWARD_SAMPLES), *args)
    assert cls.calls == 1 and a.pairs.shape[0] > 0
    same_result(a, b)
    CC.check_certified({k: getattr(b, k).numpy() for k in ("certified_lower", "hit", "undecided", "cleared_by_sampling",
                                                            "pairs")}, coef, dur)


# ------------------------------------------------------------------------------------------------------ the build
def _need_tools(*paths):
    if not all(os.path.exists(p) for p in paths) or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.skip("no object file / ROCm LLVM tools here")


def test_exec_check_and_latch_census_cover_the_new_object():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    assert len(chk.DEFAULT_OBJS) == 8 and chk.MORE_OBJS == [OBJ]
    _need_tools(OBJ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_exec_isa.py"), OBJ], capture_output=True,
                       text=True)
    assert r.returncode == 0 and "none under a reduced exec mask" in r.stdout, r.stdout + r.stderr
    assert chk.lane_latches(OBJ) == {}       # every loop of the file is wave-uniform


def _kernel_registers(obj, tmp_path):
    """(names, scratch bytes, VGPRs, AGPRs) of the kernels of one object file, from the code object's metadata"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "kernels.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, str(tmp_path / "copy.o")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    vgpr = [int(x) for x in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    agpr = [int(x) for x in re.findall(r"\.agpr_count:\s+(\d+)", notes)]
    assert len(names) == len(scratch) == len(vgpr) == len(agpr)
    return names, scratch, vgpr, agpr


def test_new_kernels_use_no_scratch_and_no_agprs(tmp_path):
    _need_tools(OBJ)
    names, scratch, vgpr, agpr = _kernel_registers(OBJ, tmp_path)
    assert len(names) >= 3
    assert any("pairs_mask_kernel" in n for n in names)
    assert scratch == [0] * len(names) and agpr == [0] * len(names)
    # the mask pass at the pairwise evaluator's 4 waves per SIMD (its __launch_bounds__): 512 / 4 -> 128 registers
    assert vgpr[[i for i, n in enumerate(names) if "pairs_mask_kernel" in n][0]] <= 128


def test_tile_kernels_of_the_pairwise_pass_keep_their_register_budget(tmp_path):
    """The kernels built on the shared register tile (csrc/msnap_pair_tile.h) and the group evaluator run at 4 waves per
    SIMD: 512 / 4 = 128 VGPRs, nothing in scratch or in AGPRs -- in any kernel of the object."""
    _need_tools(COLLIDE_OBJ)
    names, scratch, vgpr, agpr = _kernel_registers(COLLIDE_OBJ, tmp_path)
    assert scratch == [0] * len(names) and agpr == [0] * len(names), list(zip(names, scratch, agpr))
    for kernel in ("collide_span_kernel", "collide_eval_shares_kernel", "collide_eval_groups_kernel"):
        at = [i for i, n in enumerate(names) if kernel in n]
        assert len(at) == 1, (kernel, names)
        assert vgpr[at[0]] <= 128, (kernel, vgpr[at[0]])
