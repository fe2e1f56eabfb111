"""The table of K1 solve instances (csrc/msnap_solve_plan.h, plan_solve) that tests/test_solve_exact_gpu.py holds to the
60-digit solutions of tests/solve_exact.py: one entry per kernel instance a small batch can reach, with the options
that reach it and the msnap_last_kernel string it must report; the inputs every family of one (order, segment count)
shares; the project's accuracy bars; the solve into sentinel-filled outputs.  The table is static (the GPU tests need no
compiler); tests/test_solve_exact_cpu.py holds it, the restated ranges and formulas below included, to the launcher's
executed decision without a GPU."""
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------
# the project's bars on the coefficients, conftest.norm_rel
# ---------------------------------------------------------------------------
TOL = 1e-6        # north-star gate (BASELINE.json)
TIGHT = 1e-9      # order 7: what the algorithm delivers on the suite's grids (regression tripwire)
TIGHT9 = 1e-9     # order 9 on the suite's grids: pinned by the 60-digit solves of tests/golden/order9_golden.npz
                  # (SURVEY.md 8c iii); the fp64 oracles are within 2e-11 of them on every fixture case
STRESS_TOL = {7: 1e-9, 9: 2e-8}    # tools/solve_stress.py's draw (durations U(0.4, 2.5)), up to 24 / 20 segments
STRESS_MAX_SEG = {7: 24, 9: 20}

# ---------------------------------------------------------------------------
# the launcher's ranges (tests/test_solve_exact_cpu.py holds them to what plan_solve sends where)
# ---------------------------------------------------------------------------
TWIST_SEG = {7: range(2, 25), 9: range(2, 13)}        # solve_kernel_twist<K, ., M, 1 | 2 | 4>: 2..kTwistMaxSeg[9]
TWIN_SEG = {7: range(4, 21), 9: range(4, 21)}         # solve_kernel_twin<K, M>: 4..kTwinMaxSeg7 / kTwinMaxSeg
REG_SEG = {7: range(2, 21), 9: range(2, 21)}          # solve_kernel_reg<K, 10 | 20>: run-time M in 2..kRegMaxSeg2
REG_SPLIT = 10                                        # kRegMaxSeg: up to here the <K, 10> instance
GENERIC_SEG = {7: (1, 21, 25, 37, 49), 9: (1, 21, 32, 40)}   # solve_kernel<K, GS>: one segment and everything longer
# the smallest segment count whose stash leaves LDS for the global slab (solve_uses_global_scratch): with nu = K - 1,
# 8 * (16 M + (16 nu^2 + 64 nu)(M - 1) + 80 (M + 1)) + 16 * 68 * K > 160 KiB -- 3456 M + 2304 > 163840 at order 7,
# 4864 M + 1984 > 163840 at order 9
GS_MIN_SEG = {7: 47, 9: 34}
N_DRONES = 9         # a full 8-drone tile and one more (twist, twin); a partial 16-drone tile (reg, generic)
N_DRONES_GS = 3
RAISED = 7           # the drone whose clock starts at 0.25 s: the reference's start-row quirk
SHARED_SEG = 10

Case = namedtuple("Case", "family order M opts kernel n waves shared")


def khalf(order):
    return (order + 1) // 2


def scratch_bytes(order, M, tr_pitch=68):
    """rolled_lds_bytes: the dynamic LDS of solve_kernel<K, false>, transpose image + stash + input stage"""
    K = khalf(order)
    nu = K - 1
    words = 16 * M + 16 * nu * nu * max(M - 1, 0) + 64 * nu * max(M - 1, 0)
    return K * tr_pitch * 16 + (words + 16 * (M + 1) * 5) * 8


def generic_name(order, M, max_lds=160 * 1024):
    return "msnap::solve_kernel<%d, %s>" % (khalf(order), "true" if scratch_bytes(order, M) > max_lds else "false")


def _cases():
    out = []
    for order in (7, 9):
        K = khalf(order)
        for M in TWIST_SEG[order]:
            name = "msnap::solve_kernel_twist<%d, %d, %d>" % (K, (M - 2) - (M - 2) // 2, M)
            out.append(Case("twist", order, M, (), name, N_DRONES, (1, 2, 4), False))
        for M in TWIN_SEG[order]:
            out.append(Case("twin", order, M, ("no_twist",), "msnap::solve_kernel_twin<%d, %d>" % (K, M), N_DRONES,
                            (0,), False))
        for M in REG_SEG[order]:
            name = "msnap::solve_kernel_reg<%d, %d>" % (K, 10 if M <= REG_SPLIT else 20)
            out.append(Case("reg", order, M, ("no_twist", "no_twin"), name, N_DRONES, (0,), False))
        for M in GENERIC_SEG[order]:
            opts = ("no_twist",) if M in TWIST_SEG[order] else ()
            out.append(Case("generic", order, M, opts, generic_name(order, M), N_DRONES, (0,), False))
        out.append(Case("generic-GS", order, GS_MIN_SEG[order], (), "msnap::solve_kernel<%d, true>" % K, N_DRONES_GS,
                        (0,), False))
        # one shared-grid launch (times [M+1], the `shared` argument of the kernels) per family that serves 10 segments
        for c in [c for c in out if c.order == order and c.M == SHARED_SEG]:
            out.append(c._replace(shared=True))
    return out


CASES = _cases()


def case_id(c):
    return "%s-o%d-m%d%s" % (c.family, c.order, c.M, "-shared" if c.shared else "")


# ---------------------------------------------------------------------------
# inputs: the same for every family that serves one (order, M)
# ---------------------------------------------------------------------------
def inputs(order, M, grid, n=N_DRONES):
    """grid "even": synthetic.swarm, durations U(0.5, 2) -- what the suite solves everywhere; "uneven": waypoints
    U(-5, 5), yaw U(-pi, pi), durations U(0.4, 2.5) -- the draw of tools/solve_stress.py and of
    test_random_shapes_against_oracle; "shared": swarm's uniform grid, times [M+1].  On the per-drone grids drone
    RAISED (the last one of a smaller batch) has t += 0.25."""
    from drone_path_planning_python_amd.synthetic import swarm
    if grid == "shared":
        return swarm(31000 + 100 * order + M, n, M, shared_times=True)
    if grid == "even":
        wp, t = swarm(31000 + 100 * order + M, n, M)
    else:
        assert grid == "uneven"
        rng = np.random.default_rng(320000 + 1000 * order + M)
        wp = rng.uniform(-5.0, 5.0, size=(n, M + 1, 4))
        wp[..., 3] = rng.uniform(-np.pi, np.pi, size=(n, M + 1))
        T = rng.uniform(0.4, 2.5, size=(n, M))
        t = np.concatenate([np.zeros((n, 1)), np.cumsum(T, axis=1)], axis=1)
    t[raised(n)] += 0.25
    return wp, t


def raised(n):
    return min(RAISED, n - 1)


def bar(order, M, grid):
    """the bar of the project that covers this grid and length, and its name"""
    if grid in ("even", "shared"):
        return (TIGHT, "TIGHT") if order == 7 else (TIGHT9, "TIGHT9")
    if M <= STRESS_MAX_SEG[order]:
        return STRESS_TOL[order], "STRESS_TOL[%d]" % order
    return TOL, "TOL"


# ---------------------------------------------------------------------------
# one solve into fresh outputs
# ---------------------------------------------------------------------------
SENTINEL_BITS = 0x7FF8DEADBEEF0001


def solve_fresh(ctx, wp, t):
    """One msnap_solve_batch_device into FRESH device outputs pre-filled with sentinels (coefficients and durations NaN
    with a payload no kernel writes, status -7), so a piece, a duration or a status word that a kernel fails to store
    shows up as the sentinel instead of another run's value left in reused buffers.  Returns coef, dur, status."""
    import torch
    n, m1, _ = wp.shape
    m = m1 - 1
    ncoef = ctx.order + 1
    dev = torch.device("cuda", ctx.device_id)
    dwp = torch.from_numpy(np.ascontiguousarray(wp)).to(dev)
    dt = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    sentinel = np.array([SENTINEL_BITS], dtype=np.int64).view(np.float64)[0]
    coef = torch.full((n, m, 4, ncoef), sentinel, dtype=torch.float64, device=dev)
    dur = torch.full((n, m), sentinel, dtype=torch.float64, device=dev)
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.solve_batch_device(n, m, dwp, dt, t.ndim == 1, coef, dur, status)
    ctx.sync()
    out = coef.cpu().numpy(), dur.cpu().numpy(), status.cpu().numpy()
    # every word written: no sentinel survives
    for x in out[:2]:
        assert not (x.view(np.int64) == SENTINEL_BITS).any(), "an output the kernel did not store"
    assert not (out[2] == -7).any(), "a status word the kernel did not store"
    return out
