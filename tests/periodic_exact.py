"""Exact reference of the periodic minimum-snap solve (include/msnap.h, "closed-loop paths").

exact_periodic: superposition on the collocation system of tests/states_exact.py (its rows, its banded LU, one
factorisation for all right-hand sides).  With start = end = s the boundary-state solution is affine in s,
    x(s) = x_rest + sum_q s_q x_q ,
x_rest the rest-to-rest solution through the waypoints and x_q the response to the unit state e_q at both ends with all
waypoints zero (the same for every axis).  For any s derivatives 1..K-1 already agree across the seam; the periodic
optimum is the s that makes derivatives K..2K-2 agree there as well (the natural conditions of the minimisation over
the free seam state), a (K-1) x (K-1) system per axis.  Everything stays in 60 digits until the one rounding at the end.

dense_periodic: the same problem written directly -- the seam is one more knot, its rows written like an interior
knot's, one dense LU.  tests/test_periodic_cpu.py holds the two against each other.
"""
import os

import mpmath as mp
import numpy as np

import states_exact as SE

mp.mp.dps = 60

MAX_SEG = {7: 27, 9: 18}           # msnap_solve_periodic_max_segments (tests/test_periodic_cpu.py holds the library to it)
N_CASE = 17                        # one full 16-drone tile and a partial one
SEG_COUNTS = (2, 3, 10)            # and MAX_SEG[order]


def _solve_mp(t, wp, K):
    """t: knot times as mpf, wp [M+1, 4] float64 -> (x [4][NC M] as mpf, seam state s [4][K-1] as mpf)"""
    NC, NU = 2 * K, K - 1
    M = len(t) - 1
    T = [t[i + 1] - t[i] for i in range(M)]
    n = NC * M
    rows, src = SE._assemble(T, K)
    zero, one = mp.mpf(0), mp.mpf(1)
    rhs = []
    for a in range(4):                                   # rest to rest through the waypoints
        rhs.append([mp.mpf(float(wp[s[1], a])) if s is not None and s[0] == "w" else zero for s in src])
    for q in range(1, K):                                # unit state e_q at both ends, waypoints zero
        rhs.append([one if s is not None and s[0] in ("s", "e") and s[1] == q else zero for s in src])
    X = SE._banded_lu_solve(rows, rhs, n, NC)
    rows0, _ = SE._assemble(T, K)
    for x, col in zip(X, rhs):                           # the solutions against the unfactored rows
        scale = max(abs(v) for v in x) + 1
        for (lo, vals), want in zip(rows0, col):
            got = sum((v * x[lo + q] for q, v in enumerate(vals) if v != 0), zero)
            assert abs(got - want) <= scale * mp.mpf(10) ** -45, "residual"

    def jump(x, j):                                      # derivative j: end of the last segment minus start of the first
        end = sum((v * x[NC * (M - 1) + k] for k, v in enumerate(SE.deriv_row(NC, j, T[M - 1])) if v != 0), zero)
        return end - SE.falling(j, j) * x[j]

    A = mp.matrix(NU, NU)
    for r in range(NU):
        for q in range(NU):
            A[r, q] = jump(X[4 + q], K + r)
    out, seam = [], []
    for a in range(4):
        b = mp.matrix([-jump(X[a], K + r) for r in range(NU)])
        s = mp.lu_solve(A, b)
        x = [X[a][k] + sum((s[q] * X[4 + q][k] for q in range(NU)), zero) for k in range(n)]
        for j in range(1, NC - 1):                       # the seam is a knot like any other
            assert abs(jump(x, j)) <= (max(abs(v) for v in x) + 1) * mp.mpf(10) ** -40, "seam"
        out.append(x)
        seam.append([s[q] for q in range(NU)])
    return out, seam


def exact_periodic(times, wp, K):
    """times [M+1] (times[0] == 0) and wp [M+1, 4] float64, taken exactly -> coef [M, 4, 2K] and the seam state
    [4, K-1] (derivatives 1..K-1 at the first waypoint), each rounded once from 60 digits"""
    t = [mp.mpf(float(x)) for x in times]
    assert t[0] == 0
    NC, M = 2 * K, len(t) - 1
    X, seam = _solve_mp(t, wp, K)
    coef = np.empty((M, 4, NC))
    for a in range(4):
        for s in range(M):
            for q in range(NC):
                coef[s, a, q] = float(X[a][NC * s + q])
    return coef, np.array([[float(v) for v in row] for row in seam])


def dense_periodic(times, wp, K):
    """The periodic collocation written out: per segment the position at both ends; at every knot, the seam included
    (left segment M-1, right segment 0), continuity of derivatives 1..2K-2.  Returns x [4][NC M] as mpf."""
    NC = 2 * K
    t = [mp.mpf(float(x)) for x in times]
    M = len(t) - 1
    T = [t[i + 1] - t[i] for i in range(M)]
    n = NC * M
    A = mp.matrix(n, n)
    B = mp.matrix(n, 4)
    r = 0
    for i in range(M):
        right = (i + 1) % M                              # the segment that starts where segment i ends
        for k, v in enumerate(SE.deriv_row(NC, 0, mp.mpf(0))):
            A[r, NC * i + k] = v
        for a in range(4):
            B[r, a] = mp.mpf(float(wp[i, a]))
        r += 1
        for k, v in enumerate(SE.deriv_row(NC, 0, T[i])):
            A[r, NC * i + k] = v
        for a in range(4):
            B[r, a] = mp.mpf(float(wp[i + 1, a]))
        r += 1
        for j in range(1, NC - 1):
            for k, v in enumerate(SE.deriv_row(NC, j, T[i])):
                A[r, NC * i + k] += v
            for k, v in enumerate(SE.deriv_row(NC, j, mp.mpf(0))):
                A[r, NC * right + k] -= v
            r += 1
    assert r == n
    out = []
    for a in range(4):
        x = mp.lu_solve(A, B[:, a])
        out.append([x[k] for k in range(n)])
    return out


def rotate(wp, t, j):
    """The same loop started at knot j: waypoints and times of segments j..M-1, 0..j-1; the waypoints taken after the
    seam carry the lap offset wp[M] - wp[0]."""
    M = wp.shape[-2] - 1
    lap = wp[..., M:M + 1, :] - wp[..., 0:1, :]
    wp2 = np.concatenate([wp[..., j:M, :], wp[..., 0:j + 1, :] + lap], axis=-2)
    dur = np.diff(t, axis=-1)
    dur2 = np.concatenate([dur[..., j:], dur[..., :j]], axis=-1)
    t2 = np.concatenate([np.zeros(dur2.shape[:-1] + (1,)), np.cumsum(dur2, axis=-1)], axis=-1)
    return wp2, t2


# ---------------------------------------------------------------------------
# the cases of tests/test_periodic_gpu.py and their exact solutions
# ---------------------------------------------------------------------------
def case(order, M, N=N_CASE, kind="offset"):
    """Seeded inputs with states_exact.case's distributions: durations uniform in [0.5, 2] s, waypoint steps in
    [-2, 2] m.  kind "offset": wp[M] is one more random step, a nonzero lap offset on every axis; "closed": x, y, z
    return to wp[0] and yaw gains 2 pi; "shared": as "offset" with one time grid for the batch.
    Returns wp [N, M+1, 4], t [N, M+1] ([M+1] for "shared")."""
    rng = np.random.default_rng(150000 + 100 * order + M)
    dur = rng.uniform(0.5, 2.0, (N, M))
    t = np.concatenate([np.zeros((N, 1)), np.cumsum(dur, axis=1)], axis=1)
    wp = np.cumsum(rng.uniform(-2.0, 2.0, (N, M + 1, 4)), axis=1)
    if kind == "closed":
        wp[:, M, :3] = wp[:, 0, :3]
        wp[:, M, 3] = wp[:, 0, 3] + 2.0 * np.pi
    elif kind == "shared":
        t = np.ascontiguousarray(t[0])
    else:
        assert kind == "offset"
    return wp, t


def gpu_cases(order):
    """(M, kind) of every solve tests/test_periodic_gpu.py holds against 60 digits"""
    return [(M, "offset") for M in SEG_COUNTS + (MAX_SEG[order],)] + [(10, "shared"), (10, "closed")]


def golden_path(order):
    """The longest case of each order is recorded; one file per order"""
    name = "periodic_golden.npz" if order == 7 else "periodic_golden_order9.npz"
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)


def exact_batch(wp, t, K):
    """wp [N, M+1, 4], t [N, M+1] or [M+1] -> coef [N, M, 4, 2K], seam [N, 4, K-1]"""
    N, M = wp.shape[0], wp.shape[1] - 1
    coef, seam = np.empty((N, M, 4, 2 * K)), np.empty((N, 4, K - 1))
    for d in range(N):
        coef[d], seam[d] = exact_periodic(t if t.ndim == 1 else t[d], wp[d], K)
    return coef, seam


_REF = {}


def reference(order, M, kind="offset"):
    """(coef [N, M, 4, 2K], seam [N, 4, K-1]) for case(order, M, kind=kind): computed once here, or read from the
    recorded file for the longest"""
    key = (order, M, kind)
    if key not in _REF:
        wp, t = case(order, M, kind=kind)
        if M == MAX_SEG[order] and kind == "offset":
            g = np.load(golden_path(order))
            for name, arr in (("wp", wp), ("t", t)):
                assert np.array_equal(g[name], arr), f"{golden_path(order)} was recorded for other inputs ({name})"
            _REF[key] = (g["coef"], g["seam"])
        else:
            _REF[key] = exact_batch(wp, t, (order + 1) // 2)
    return _REF[key]
