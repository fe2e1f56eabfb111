"""Exact reference of the K1 solve (msnap_solve_batch): the rest-to-rest collocation system of tests/states_exact.py at
60 digits -- rest at both ends, C^1..C^(2K-2) at the knots, interpolation -- with the reference's start-row quirk: the K
start rows of segment 0 are taken at local time t[0], not at 0, and their right-hand side is w_0 and zeros
(oracle/msnap_oracle.py::assemble_1d; the kernels implement it with a Taylor shift).  Assembly, the banded LU and the
residual assertion are states_exact's own (solve_checked); with t[0] == 0 the result is exact_solve's bit for bit.

seg_scaled: the error of a solution in units of each segment's own position scale.
"""
import mpmath as mp
import numpy as np

import states_exact as SE


def exact_solve_k1(times, wp, K):
    """times [M+1], wp [M+1, 4] float64 (taken exactly) -> coef [M, 4, 2K]: the 60-digit solution rounded once"""
    t = [mp.mpf(float(x)) for x in times]
    return SE.solve_checked(t, wp, [(None, None)], K, None if t[0] == 0 else t[0])[0]


_CACHE = {}


def exact_batch_k1(wp, t, K):
    """wp [N, M+1, 4], t [N, M+1] or [M+1] -> coef [N, M, 4, 2K].  Cached per process by the inputs' bytes, so the
    kernel families that serve one (order, segment count) share one solve; the cached array is read-only."""
    wp = np.ascontiguousarray(wp, dtype=np.float64)
    t = np.ascontiguousarray(t, dtype=np.float64)
    key = (K, wp.shape, t.shape, wp.tobytes(), t.tobytes())
    hit = _CACHE.get(key)
    if hit is None:
        N, M = wp.shape[0], wp.shape[1] - 1
        hit = np.empty((N, M, 4, 2 * K))
        for d in range(N):
            hit[d] = exact_solve_k1(t if t.ndim == 1 else t[d], wp[d], K)
        hit.setflags(write=False)
        _CACHE[key] = hit
    return hit


def seg_scaled(got, ref, dur):
    """Per drone, segment and axis max_k |c_k - r_k| T^k / max_k |r_k| T^k -- the coefficient error weighted as it
    reaches the position at the segment's far end, over the segment's own position scale.  got / ref [N, M, 4, NC],
    dur [N, M].  Returns (worst value, (drone, segment, axis, k) of it)."""
    got, ref = np.asarray(got), np.asarray(ref)
    pw = np.asarray(dur)[:, :, None, None] ** np.arange(ref.shape[-1])
    den = np.abs(ref * pw).max(axis=3, keepdims=True)
    e = np.abs(got - ref) * pw / np.where(den == 0, 1.0, den)
    at = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[at]), tuple(int(i) for i in at)


def norm_rel_at(got, ref):
    """conftest.norm_rel with the place of its worst element: (value, (drone, segment, axis, k))"""
    got, ref = np.asarray(got), np.asarray(ref)
    den = np.abs(ref).max(axis=(1, 3), keepdims=True)
    e = np.abs(got - ref) / np.where(den == 0, 1.0, den)
    at = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[at]), tuple(int(i) for i in at)
