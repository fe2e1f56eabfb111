"""NumPy restatement of the time allocation on closed loops (include/msnap.h, msnap_optimize_times_periodic;
csrc/msnap_timeopt.hip with kTimeoptRing) for the tests and for tests/golden/make_timeopt_periodic_golden.py.

The solve is periodic_ref.solve, the fp64 model of the ring elimination that tests/test_periodic_cpu.py holds to the
60-digit solution.  The iteration is timeopt_ref.optimize itself, run with this solve as its `evaluate` through
timeopt_states_ref.given_states' way of swapping it in: floor, direction, step rules and stopping measure are imported,
not copied."""
import contextlib

import numpy as np

import periodic_ref as P
import timeopt_ref as R
import timeopt_states_ref as S
from timeopt_ref import direction, floor_of, start_times, trial_times  # noqa: F401  (the shipped rules, re-exported)


def solve(wp, t, K):
    """wp [M+1, 4], t [M+1] with t[0] == 0 -> coef [M, 4, 2K]"""
    return P.solve(wp, t, K)[0]


def cost(coef, dur, w):
    return R.weighted(R.fast_cost(coef, np.asarray(dur, dtype=np.float64)), w)


def evaluate(wp, t, w, ncoef):
    """One trial: (J, g [M], coef) for the knot times t; None when the solve fails."""
    try:
        coef = solve(wp, t, ncoef // 2)
    except np.linalg.LinAlgError:
        return None
    J = cost(coef, np.diff(t), w)
    if not np.isfinite(J):
        return None
    g4 = R.snap_cost_grad(coef)
    g = np.array([R.weighted(g4[i], w) for i in range(g4.shape[0])])
    return float(J), g, coef


@contextlib.contextmanager
def on_the_ring():
    """Inside, timeopt_ref.evaluate -- and with it everything built on it -- is the periodic solve.  The swap is
    timeopt_states_ref.given_states' own; only the function it installs is replaced."""
    with S.given_states(None, None):
        R.evaluate = lambda wp_, t_, w_, ncoef_, cost_fn=None: evaluate(wp_, t_, w_, ncoef_)
        yield


def optimize(wp, t, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200, tol=1e-4, ncoef=8, trace=None):
    """timeopt_ref.optimize with the periodic solve as its `evaluate`: the same dict, the same `trace`."""
    with on_the_ring():
        return R.optimize(wp, t, weights, min_fraction, max_iter, tol, ncoef, None, trace=trace)


def unpack_cases(z):
    """The drones of tests/golden/timeopt_periodic_golden.npz (flat arrays) as a list of dicts: k, group, order, kind,
    min_fraction, weights, shared, wp [M+1, 4] float64, t [M+1], and the prefix knots p_t (max_iter 1, 3)."""
    out = []
    for k in range(int(z["n"])):
        g = int(z["group"][k])
        lo, hi = int(z["off"][k]), int(z["off"][k + 1])
        out.append({"k": k, "group": g, "order": int(z["order"][g]), "kind": str(z["kind"][g]),
                    "min_fraction": float(z["min_fraction"][g]), "weights": tuple(float(x) for x in z["weights"][g]),
                    "shared": bool(z["shared"][g]), "wp": z["wp"][lo:hi].astype(np.float64), "t": z["t"][lo:hi],
                    "p_t": (z["p_t1"][lo:hi], z["p_t3"][lo:hi])})
    return out
