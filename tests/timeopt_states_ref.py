"""NumPy restatement of the time allocation from and to given end states (include/msnap.h,
msnap_optimize_times_states; csrc/msnap_timeopt.hip with ENDS) for the tests and for
tests/golden/make_timeopt_states_golden.py.

The solve is the dense collocation system of tests/states_exact.py::_assemble -- the same rows in the same order -- in
fp64 with np.linalg.solve; tests/test_timeopt_states_cpu.py holds it to the 60-digit solution.  The iteration is
timeopt_ref.optimize itself, run with this solve as its `evaluate`: floor, direction, step rules and stopping measure
are imported, not copied."""
import contextlib
import math

import numpy as np

import timeopt_ref as R
from timeopt_ref import direction, floor_of, start_times, trial_times  # noqa: F401  (the shipped rules, re-exported)


def _falling(nc):
    """F[j, k] = k (k-1) .. (k-j+1), 0 for k < j"""
    F = np.zeros((nc, nc))
    for j in range(nc):
        for k in range(j, nc):
            F[j, k] = math.factorial(k) // math.factorial(k - j)
    return F


def _deriv_rows(nc, F, t):
    """row j: the j-th derivative of sum_k c_k t^k at t as a row over c (0**0 == 1)"""
    e = np.arange(nc)[None, :] - np.arange(nc)[:, None]
    with np.errstate(divide="ignore"):
        P = np.where(e >= 0, np.power(float(t), np.maximum(e, 0)), 0.0)
    return F * P


def assemble(T, K):
    """The rows of states_exact._assemble(T, K) as a dense fp64 matrix, and per row the source of its right-hand side:
    ("w", i), ("s", q), ("e", q) or None."""
    NC, M = 2 * K, len(T)
    F = _falling(NC)
    at0 = _deriv_rows(NC, F, 0.0)
    A = np.zeros((NC * M, NC * M))
    src = []
    r = 0
    A[r:r + K, 0:NC] = at0[:K]
    src += [("w", 0)] + [("s", j) for j in range(1, K)]
    r += K
    for i in range(1, M):
        lo = NC * (i - 1)
        end = _deriv_rows(NC, F, T[i - 1])
        A[r, lo:lo + NC] = end[0]
        A[r + 1, lo + NC:lo + 2 * NC] = at0[0]
        src += [("w", i), ("w", i)]
        r += 2
        n = NC - 2
        A[r:r + n, lo:lo + NC] = end[1:NC - 1]
        A[r:r + n, lo + NC:lo + 2 * NC] = -at0[1:NC - 1]
        src += [None] * n
        r += n
    A[r:r + K, NC * (M - 1):] = _deriv_rows(NC, F, T[M - 1])[:K]
    src += [("w", M)] + [("e", j) for j in range(1, K)]
    return A, src


def solve(wp, t, start, end, K):
    """wp [M+1, 4], t [M+1] with t[0] == 0, start / end [4, K-1] or None (rest) -> coef [M, 4, 2K]"""
    wp = np.asarray(wp, dtype=np.float64)
    T = np.diff(np.asarray(t, dtype=np.float64))
    M, NC = len(T), 2 * K
    A, src = assemble(T, K)
    B = np.zeros((NC * M, 4))
    for r, s in enumerate(src):
        if s is None:
            continue
        if s[0] == "w":
            B[r] = wp[s[1]]
        else:
            blk = start if s[0] == "s" else end
            if blk is not None:
                B[r] = np.asarray(blk, dtype=np.float64)[:, s[1] - 1]
    X = np.linalg.solve(A, B)                      # [NC M, 4]
    return np.ascontiguousarray(X.reshape(M, NC, 4).transpose(0, 2, 1))


def cost(coef, dur, w):
    return R.weighted(R.fast_cost(coef, np.asarray(dur, dtype=np.float64)), w)


def evaluate(wp, t, w, ncoef, start=None, end=None):
    """One trial: (J, g [M], coef) for the knot times t; None when the solve fails."""
    try:
        coef = solve(wp, t, start, end, ncoef // 2)
    except np.linalg.LinAlgError:
        return None
    J = cost(coef, np.diff(t), w)
    if not np.isfinite(J):
        return None
    g4 = R.snap_cost_grad(coef)
    g = np.array([R.weighted(g4[i], w) for i in range(g4.shape[0])])
    return float(J), g, coef


@contextlib.contextmanager
def given_states(start, end):
    """Inside, timeopt_ref.evaluate -- and with it everything built on it -- is the boundary-state solve."""
    orig = R.evaluate
    R.evaluate = lambda wp_, t_, w_, ncoef_, cost_fn=None: evaluate(wp_, t_, w_, ncoef_, start, end)
    try:
        yield
    finally:
        R.evaluate = orig


def optimize(wp, t, start=None, end=None, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200, tol=1e-4, ncoef=8,
             trace=None):
    """timeopt_ref.optimize with the boundary-state solve as its `evaluate`: the same dict, the same `trace`."""
    with given_states(start, end):
        return R.optimize(wp, t, weights, min_fraction, max_iter, tol, ncoef, None, trace=trace)


def unpack_cases(z):
    """The drones of tests/golden/timeopt_states_golden.npz as a list of dicts: k, group, order, combo, min_fraction,
    weights, shared, wp [M+1, 4] float64, t [M+1], start / end [4, K-1] or None, and the prefix knots p_t."""
    out = []
    for k in range(int(z["n"])):
        g = int(z["group"][k])
        lo, hi = int(z["off"][k]), int(z["off"][k + 1])
        order = int(z["order"][g])
        nd = (order + 1) // 2 - 1
        combo = str(z["combo"][k])
        out.append({"k": k, "group": g, "order": order, "combo": combo, "min_fraction": float(z["min_fraction"][g]),
                    "weights": tuple(float(x) for x in z["weights"][g]), "shared": bool(z["shared"][g]),
                    "wp": z["wp"][lo:hi].astype(np.float64), "t": z["t"][lo:hi],
                    "start": z["start"][k][:, :nd].copy() if combo in ("start", "both") else None,
                    "end": z["end"][k][:, :nd].copy() if combo in ("end", "both") else None,
                    "p_t": (z["p_t1"][lo:hi], z["p_t3"][lo:hi])})
    return out
