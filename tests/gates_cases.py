"""Inputs for the edges of msnap_solve_gates that tests/gates_exact.py's case() does not reach (include/msnap.h, "gates";
DESIGN.md §5 K21): tests/test_gates_edges_cpu.py holds the structure of every builder and the NumPy restatement on it,
tests/test_gates_edges_gpu.py holds the kernel on the same inputs.

Every builder is a pure NumPy function of (order, ...) with fixed seeds and returns (wp, t, start, end, fix, via) in
the layout of GE.case -- t may be 1-D (shared), start / end may be None (rest).  via holds NaN under every clear bit
unless the builder says otherwise.  The waypoints, times and end states are SE.case's.
"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gates_exact as GE  # noqa: E402
import states_exact as SE  # noqa: E402

mp.mp.dps = 60

M_EDGE = 6                          # the segment count of every builder that does not say otherwise
N_SPARSE = 33                       # two full 16-drone tiles and a lone drone
STIFF_RATIO = {7: 30.0, 9: 10.0}    # G: at order 9 the float64 restatement leaves 2e-10 at a ratio of 30
FAR = 2.0 ** 22                     # H: the translation, metres
GRID = 2.0 ** -20                   # H: the waypoints' grid -- FAR + 14 m on it still fits a double exactly
ST_TIMES, ST_NONFINITE = 2, 3       # msnap_status


def half(order):
    return (order + 1) // 2


def used_bits(fix, K):
    """[N, M-1, K-1] bool: derivative q (index q-1) is prescribed at that knot"""
    return ((fix[:, :, None] >> np.arange(K - 1)) & 1).astype(bool)


def values(order, fix, seed):
    """via [N, M-1, 4, K-1] in the STATE_SCALE ranges, NaN under every clear bit of fix"""
    K = half(order)
    rng = np.random.default_rng(seed)
    via = rng.uniform(-1.0, 1.0, fix.shape + (4, K - 1)) * np.array(SE.STATE_SCALE[:K - 1])
    return np.where(used_bits(fix, K)[:, :, None, :], via, np.nan)


# ---- A. sparse tiles ------------------------------------------------------------------------------------------------
def sparse_masks(order):
    """fix [33, 5].  Tile 0: knot 1 gated by drone 3 only (every bit), knot 2 by nobody, knot 3 by drone 15 only
    (velocity), knot 4 by nobody, knot 5 by drones 0 and 8 with different masks.  Tile 1: nothing.  Tile 2, drone 32
    alone: knots 2 and 4."""
    K = half(order)
    full = 2 ** (K - 1) - 1
    fix = np.zeros((N_SPARSE, M_EDGE - 1), dtype=np.int32)
    fix[3, 0] = full
    fix[15, 2] = 1
    fix[0, 4] = 2
    fix[8, 4] = full ^ 2
    fix[32, 1] = 3
    fix[32, 3] = 4
    return fix


def sparse(order):
    wp, t, start, end = SE.case(order, M_EDGE, N_SPARSE)
    fix = sparse_masks(order)
    return wp, t, start, end, fix, values(order, fix, 230000 + order)


# ---- B. shared times ------------------------------------------------------------------------------------------------
def shared(order):
    """A's batch on one time grid: t is 1-D"""
    wp, t, start, end, fix, via = sparse(order)
    return wp, np.ascontiguousarray(t[0]), start, end, fix, via


# ---- C. rest ends ---------------------------------------------------------------------------------------------------
REST_COMBOS = ((False, False), (True, False), (False, True))      # (start given, end given)


def rest(order, combo):
    wp, t, start, end, fix, via = GE.case(order, M_EDGE)
    return wp, t, start if combo[0] else None, end if combo[1] else None, fix, via


# ---- D. prescribed zeros --------------------------------------------------------------------------------------------
def zeros(order, zero=0.0):
    """case()'s masks with every used value `zero` (0.0 or -0.0): a stop, a hold of zero acceleration"""
    wp, t, start, end, fix, via = GE.case(order, M_EDGE)
    return wp, t, start, end, fix, np.where(np.isnan(via), np.nan, zero)


# ---- E. every knot fully gated --------------------------------------------------------------------------------------
FULL_SEGMENTS = (2, 5)


def full(order, M, N=GE.N_CASE):
    K = half(order)
    wp, t, start, end = SE.case(order, M, N)
    fix = np.full((N, M - 1), 2 ** (K - 1) - 1, dtype=np.int32)
    return wp, t, start, end, fix, values(order, fix, 240000 + 100 * order + M)


def knot_states(start, end, via):
    """[N, M+1, 4, K-1]: the derivative vectors of every knot of a fully gated batch"""
    return np.concatenate([start[:, None], via, end[:, None]], axis=1)


def hermite_exact(t0, t1, w0, w1, s0, s1, K):
    """The degree-(2K-1) polynomial with value and derivatives 1 .. K-1 given at 0 and at T = t1 - t0 (the two float64
    times taken exactly, as gates_exact takes them), as one 2K x 2K solve at 60 digits (no closed form, nothing of
    gates_exact or states_exact): w0 / w1 [A], s0 / s1 [A, K-1] -> [A, 2K] float64, rounded once"""
    NC = 2 * K
    T = mp.mpf(float(t1)) - mp.mpf(float(t0))
    A = mp.zeros(NC, NC)
    for q in range(K):
        A[q, q] = mp.factorial(q)                                   # derivative q at 0
        for j in range(q, NC):                                      # derivative q at T
            A[K + q, j] = mp.factorial(j) / mp.factorial(j - q) * T ** (j - q)
    n_ax = len(w0)
    out = np.empty((n_ax, NC))
    for a in range(n_ax):
        b = mp.zeros(NC, 1)
        b[0], b[K] = mp.mpf(float(w0[a])), mp.mpf(float(w1[a]))
        for q in range(1, K):
            b[q], b[K + q] = mp.mpf(float(s0[a, q - 1])), mp.mpf(float(s1[a, q - 1]))
        x = mp.lu_solve(A, b)
        assert mp.norm(A * x - b, mp.inf) <= mp.mpf(10) ** -45 * (1 + mp.norm(x, mp.inf))
        out[a] = [float(x[j]) for j in range(NC)]
    return out


def hermite_batch(wp, t, states, K):
    """coef [N, M, 4, 2K]: every segment of every drone interpolates its two knots' states"""
    N, M = wp.shape[0], wp.shape[1] - 1
    out = np.empty((N, M, 4, 2 * K))
    for d in range(N):
        for i in range(M):
            out[d, i] = hermite_exact(t[d, i], t[d, i + 1], wp[d, i], wp[d, i + 1], states[d, i], states[d, i + 1], K)
    return out


# ---- F. a fault at every knot ---------------------------------------------------------------------------------------
FAULT_SEGMENTS = (5, 2)
N_FAULT = 16
FAULT_KINDS = ("nan", "+inf", "-inf", "mask 2^(K-1)", "mask -1")


def fault_of(order, M, d):
    """(knot 1 .. M-1, axis, derivative index 0 .. K-2, kind) of drone d's one fault"""
    K = half(order)
    return 1 + d % (M - 1), d % 4, d % (K - 1), FAULT_KINDS[d % len(FAULT_KINDS)]


def faults(order, M, which="all"):
    """full(order, M, 16) -- the clean batch -- and (fix, via) with one fault per drone of `which` ("all" or "odd"),
    laid out by fault_of: returns (clean, fix, via, faulted [16] bool)"""
    K = half(order)
    clean = full(order, M, N_FAULT)
    fix, via = clean[4].copy(), clean[5].copy()
    faulted = np.zeros(N_FAULT, dtype=bool)
    for d in range(N_FAULT):
        if which == "odd" and d % 2 == 0:
            continue
        knot, axis, q, kind = fault_of(order, M, d)
        if kind == "mask 2^(K-1)":
            fix[d, knot - 1] = 2 ** (K - 1)
        elif kind == "mask -1":
            fix[d, knot - 1] = -1
        else:
            via[d, knot - 1, axis, q] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
        faulted[d] = True
    return clean, fix, via, faulted


# ---- G. stiff durations ---------------------------------------------------------------------------------------------
def stiff(order):
    """case()'s masks and values on durations that alternate 1.5 s and 1.5 / R s; even drones begin with the long one,
    odd drones with the short one"""
    wp, _, start, end, fix, via = GE.case(order, M_EDGE)
    N = wp.shape[0]
    pair = np.array([1.5, 1.5 / STIFF_RATIO[order]])
    dur = np.stack([np.resize(pair if d % 2 == 0 else pair[::-1], M_EDGE) for d in range(N)])
    t = np.concatenate([np.zeros((N, 1)), np.cumsum(dur, axis=1)], axis=1)
    return wp, t, start, end, fix, via


# ---- H. translation -------------------------------------------------------------------------------------------------
def translated(order, gated):
    """(near, far): A's batch with the waypoints rounded to multiples of 2^-20 m, and the same 2^22 m away on every
    axis -- every waypoint of `far` is exact and so is every difference of two.  gated False: fix and via are None."""
    wp, t, start, end, fix, via = sparse(order)
    wp = np.round(wp / GRID) * GRID
    if not gated:
        fix = via = None
    return (wp, t, start, end, fix, via), (wp + FAR, t, start, end, fix, via)


# ---- I. symmetries --------------------------------------------------------------------------------------------------
def dyadic(order):
    """A's masks and values on dyadic durations (multiples of 1/64 s in [0.5, 2]), so that the running sums of the
    durations are exact in either direction"""
    wp, _, start, end, fix, via = sparse(order)
    rng = np.random.default_rng(250000 + order)
    dur = rng.integers(32, 129, (N_SPARSE, M_EDGE)) / 64.0
    t = np.concatenate([np.zeros((N_SPARSE, 1)), np.cumsum(dur, axis=1)], axis=1)
    return wp, t, start, end, fix, via


def scaled_in_value(case, s=4.0):
    """every length times s: waypoints, end states and gate values (NaN stays NaN); the coefficients scale by s"""
    wp, t, start, end, fix, via = case
    return s * wp, t, s * start, s * end, fix, s * via


def scaled_in_time(case, order, s=4.0):
    """t -> s t: the q-th derivative of every given state scales by s^-q; coefficient j scales by s^-j"""
    K = half(order)
    wp, t, start, end, fix, via = case
    f = s ** -np.arange(1.0, K)
    return wp, s * t, start * f, end * f, fix, via * f


def reversed_in_time(case, order):
    """The same path flown backwards: waypoints, durations, mask rows and value rows reverse, the end states swap, and
    every odd derivative changes sign"""
    K = half(order)
    wp, t, start, end, fix, via = case
    dur = np.diff(t, axis=1)
    tr = np.concatenate([np.zeros((t.shape[0], 1)), np.cumsum(dur[:, ::-1], axis=1)], axis=1)
    sign = np.array([(-1.0) ** q for q in range(1, K)])
    return (np.ascontiguousarray(wp[:, ::-1]), tr, end * sign, start * sign, np.ascontiguousarray(fix[:, ::-1]),
            np.ascontiguousarray(via[:, ::-1]) * sign)


# ---- the exact solutions, computed once per process -----------------------------------------------------------------
_REF = {}


def exact(key, case):
    """GE.exact_solve over the batch `case`, kept under `key`"""
    if key not in _REF:
        wp, t, start, end, fix, via = case
        N, M = wp.shape[0], wp.shape[1] - 1
        K = (np.asarray(via).shape[-1] + 1) if via is not None else (start.shape[-1] + 1)
        if fix is None:
            fix = np.zeros((N, M - 1), dtype=np.int32)
            via = np.full((N, M - 1, 4, K - 1), np.nan)
        ref = np.empty((N, M, 4, 2 * K))
        for d in range(N):
            ref[d] = GE.exact_solve(t if t.ndim == 1 else t[d], wp[d], None if start is None else start[d],
                                    None if end is None else end[d], fix[d], via[d], K)
        _REF[key] = ref
    return _REF[key]
