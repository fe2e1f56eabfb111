"""Dynamic limits without a GPU: the exact reference itself, the argument checks of the C-ABI, the exec-mask check on
the new translation unit, and swarm.retime_swarm's exchange under gloo at world 2 and 3 (the device arithmetic replaced
by a NumPy stand-in behind DeviceCompute's interface)."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limits_exact as LE  # noqa: E402


def _poly(nc, **terms):
    c = np.zeros(nc)
    for k, v in terms.items():
        c[int(k[1:])] = v
    return c


def test_exact_reference_on_hand_built_polynomials():
    nc = 8
    coef = np.zeros((2, 4, nc))
    # segment 0, T = 1: x = t^2/2 - t^3/3 (speed t(1-t): 1/4 at t = 1/2; acceleration 1 - 2t: 1 at both ends, the
    # earlier wins; jerk 2), yaw = t^3 (rate 3 t^2: 3 at t = 1)
    coef[0, 0] = _poly(nc, c2=0.5, c3=-1.0 / 3.0)
    coef[0, 3] = _poly(nc, c3=1.0)
    # segment 1, T = 2: y = 3t (speed 3 everywhere: the earliest time), nothing else moves
    coef[1, 1] = _poly(nc, c1=3.0)
    dur = np.array([1.0, 2.0])
    peaks, times = LE.exact_peaks(coef, dur)
    got = [float(p) for p in peaks]
    assert got[0] == pytest.approx(3.0, rel=1e-15) and float(times[0]) == pytest.approx(1.0, abs=1e-15)
    assert got[1] == pytest.approx(1.0, rel=1e-15) and float(times[1]) == pytest.approx(0.0, abs=1e-15)
    assert got[2] == pytest.approx(2.0, rel=1e-15)
    assert got[3] == pytest.approx(3.0, rel=1e-15) and float(times[3]) == pytest.approx(1.0, abs=1e-15)
    # one segment alone: the interior maximum of the speed
    p1, t1 = LE.exact_peaks(coef[:1], dur[:1])
    assert float(p1[0]) == pytest.approx(0.25, rel=1e-15) and float(t1[0]) == pytest.approx(0.5, rel=1e-15)
    # 2-D: x' = 1 - t, y' = t: |v|^2 = 1 - 2t + 2t^2 on [0, 1] is 1 at both ends (a tie: the earlier time)
    c2 = np.zeros((1, 4, nc))
    c2[0, 0] = _poly(nc, c1=1.0, c2=-0.5)
    c2[0, 1] = _poly(nc, c2=0.5)
    p2, t2 = LE.exact_peaks(c2, np.array([1.0]))
    assert float(p2[0]) == pytest.approx(1.0, rel=1e-15) and float(t2[0]) == pytest.approx(0.0, abs=1e-15)
    # the fp64 reference agrees on all of them
    assert np.allclose(LE.fp64_peaks(coef[None], dur[None])[0], got, rtol=1e-12)


def test_exact_reference_bounds_a_dense_sample():
    rng = np.random.default_rng(7)
    nc = 8
    for trial in range(3):
        coef = rng.standard_normal((3, 4, nc)) / np.arange(1, nc + 1) ** 2
        dur = rng.uniform(0.2, 2.0, size=3)
        peaks, _ = LE.exact_peaks(coef, dur)
        for q, (r, axes) in enumerate(LE.ORDERS):
            dense = 0.0
            for i in range(3):
                t = np.linspace(0.0, dur[i], 10_000)
                vals = np.zeros_like(t)
                for a in axes:
                    d = np.polynomial.polynomial.polyder(coef[i, a], r)
                    vals += np.polynomial.polynomial.polyval(t, d) ** 2
                dense = max(dense, float(np.sqrt(vals.max())))
            S = float(peaks[q])
            assert dense <= S * (1 + 1e-12), (trial, q, dense, S)
            assert dense >= S * (1 - 1e-6), (trial, q, dense, S)      # the sample comes close
        assert np.allclose(LE.fp64_peaks(coef[None], dur[None])[0], [float(p) for p in peaks], rtol=1e-9)


def test_argument_checks_without_a_device():
    from drone_path_planning_python_amd import _lib
    from drone_path_planning_python_amd.context import RETIME_COMMON, RETIME_FIT
    lib = _lib.load()
    assert lib.msnap_version() >= 300
    lim = (ctypes.c_double * 4)(1.0, 0.0, 0.0, 0.0)
    assert lib.msnap_dynamic_peaks(None, 1, 1, None, None, None, None, None) == -1
    assert lib.msnap_dynamic_peaks_device(None, 1, 1, None, None, None, None, None) == -1
    assert lib.msnap_time_scale(None, 1, 1, None, None, None, None, None) == -1
    assert lib.msnap_time_scale_device(None, 1, 1, None, None, None, None, None) == -1
    assert lib.msnap_retime_to_limits(None, 1, 1, None, None, lim, 0, None, None, None) == -1
    assert lib.msnap_retime_to_limits_device(None, 1, 1, None, None, lim, 0, None, None, None) == -1
    with open(os.path.join(ROOT, "include", "msnap.h")) as f:
        text = f.read()
    assert f"MSNAP_RETIME_FIT = {RETIME_FIT}" in text and f"MSNAP_RETIME_COMMON = {RETIME_COMMON}" in text
    from drone_path_planning_python_amd.swarm import check_limits
    check_limits([1.0, 0.0, np.inf, 2.0])
    for bad in ([-1.0, 0, 0, 0], [0, np.nan, 0, 0], [1.0, 2.0]):
        with pytest.raises(ValueError):
            check_limits(bad)


def test_exec_check_covers_the_limits_object():
    obj = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc", "msnap_limits.o")
    if not os.path.exists(obj):
        pytest.skip("no build here")
    tool = os.path.join(ROOT, "tools", "check_exec_isa.py")
    r = subprocess.run([sys.executable, tool, obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "msnap_limits.o" in r.stdout and "none under a reduced exec mask" in r.stdout
    with open(tool) as f:
        assert '"msnap_limits.o"' in f.read()       # and build() runs it by default


# ------------------------------------------------------------------------------------------------ retime_swarm, gloo
class NumpyLimitsCompute:
    """CPU stand-in with DeviceCompute's retime_to_limits / time_scale (tests only): peaks from limits_exact's fp64
    reference, the factor and the scaling as include/msnap.h states them."""

    def retime_to_limits(self, coef, dur, limits, fit=False, common=False):
        c, d = coef.numpy(), dur.numpy()
        n = d.shape[0]
        scale = np.full(n, np.nan)
        ok = np.isfinite(c).reshape(n, -1).all(axis=1) & np.isfinite(d).all(axis=1)
        if ok.any():
            pk = LE.fp64_peaks(c[ok], d[ok]) * (1 + 2e-9)
            k = np.zeros(int(ok.sum()))
            for q, p in enumerate((1.0, 2.0, 3.0, 1.0)):
                if 0 < limits[q] < np.inf:
                    k = np.maximum(k, (pk[:, q] / limits[q]) ** (1.0 / p))
            k = np.where(k > 0, k, 1.0) if fit else np.maximum(k, 1.0)
            scale[ok] = k
        if common and np.isfinite(scale).any():
            scale[np.isfinite(scale)] = np.nanmax(scale)
        s = torch.from_numpy(scale)
        co, do = self.time_scale(coef, dur, s)
        return co, do, s

    def time_scale(self, coef, dur, scale):
        c, d, k = coef.numpy().copy(), dur.numpy().copy(), scale.numpy()
        for i, kk in enumerate(k):
            if np.isfinite(kk) and kk > 0:
                c[i] *= (1.0 / kk) ** np.arange(c.shape[-1])
                d[i] *= kk
        return torch.from_numpy(c), torch.from_numpy(d)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _swarm(n, fail=()):
    rng = np.random.default_rng(3)
    coef = rng.standard_normal((n, 3, 4, 8)) / np.arange(1, 9) ** 2
    dur = rng.uniform(0.5, 1.5, size=(n, 3))
    for k in fail:
        coef[k] = np.nan
    return coef, dur


def _worker(rank, world, port, n, fail, limits, fit, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from drone_path_planning_python_amd.swarm import retime_swarm, shard_bounds
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        coef, dur = _swarm(n, fail)
        lo, hi = shard_bounds(n, world, rank)
        c, d, s = retime_swarm(NumpyLimitsCompute(), torch.from_numpy(coef[lo:hi].copy()),
                               torch.from_numpy(dur[lo:hi].copy()), limits, world, rank, dist=dist, fit=fit)
        q.put((rank, lo, hi, c.numpy(), d.numpy(), s.numpy()))
    finally:
        dist.destroy_process_group()


def _run_sharded(world, n, fail, limits, fit):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, fail, limits, fit, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(out)


@pytest.mark.parametrize("world,n,fail,fit", [(2, 7, (), False), (3, 8, (4,), True), (3, 2, (), False),
                                              (2, 3, (0, 1), False)])
def test_retime_swarm_sharded_equals_unsharded(world, n, fail, fit):
    limits = [0.4, 0.3, 0.0, 0.5]
    coef, dur = _swarm(n, fail)
    c_ref, d_ref, s_ref = NumpyLimitsCompute().retime_to_limits(torch.from_numpy(coef), torch.from_numpy(dur),
                                                               limits, fit=fit, common=True)
    parts = _run_sharded(world, n, fail, limits, fit)
    assert any(hi == lo for _, lo, hi, *_ in parts) == (n < world)       # (a rank with 0 drones took part)
    for _, lo, hi, c, d, s in parts:
        assert np.array_equal(s, s_ref.numpy()[lo:hi], equal_nan=True)
        assert np.array_equal(d, d_ref.numpy()[lo:hi], equal_nan=True)
        assert np.array_equal(c, c_ref.numpy()[lo:hi], equal_nan=True)
        for k in fail:
            if lo <= k < hi:
                assert np.isnan(s[k - lo]) and np.isnan(c[k - lo]).all()
