"""NumPy restatement of the time allocation through gates (include/msnap.h, msnap_optimize_times_gates;
csrc/msnap_timeopt_kernel.h with GATES) for the tests and for
tests/golden/make_timeopt_gates_golden.py.

The solve is tests/gates_ref.py::solve, the float64 model of the masked block sweep that tests/test_gates_cpu.py holds
to the 60-digit reference.  The iteration is timeopt_ref.optimize itself, run with this solve as its `evaluate`, the
pattern of timeopt_states_ref.given_states: floor, direction, step rules and stopping measure are imported, not copied.
The gradient is the closed form every mode uses, -sum_a w_a E_i,a: a gated component of a knot's derivative vector is
data, which the envelope argument does not look at (tests/test_timeopt_gates_cpu.py holds it to central differences of
the solved cost)."""
import contextlib

import numpy as np

import gates_ref
import timeopt_ref as R
from timeopt_ref import direction, floor_of, start_times, trial_times  # noqa: F401  (the shipped rules, re-exported)


def solve(wp, t, start, end, fix, via, K):
    """wp [M+1, 4], t [M+1] with t[0] == 0, start / end [4, K-1] or None, fix [M-1] or None (no gates),
    via [M-1, 4, K-1] -> coef [M, 4, 2K]"""
    M = len(t) - 1
    if fix is None:
        fix, via = np.zeros((max(M - 1, 0),), dtype=np.int32), np.zeros((max(M - 1, 0), 4, K - 1))
    return gates_ref.solve(wp, t, start, end, fix, via, K)


def cost(coef, dur, w):
    return R.weighted(R.fast_cost(coef, np.asarray(dur, dtype=np.float64)), w)


def evaluate(wp, t, w, ncoef, start=None, end=None, fix=None, via=None):
    """One trial: (J, g [M], coef) for the knot times t; None when the solve fails."""
    try:
        coef = solve(wp, t, start, end, fix, via, ncoef // 2)
    except np.linalg.LinAlgError:
        return None
    J = cost(coef, np.diff(t), w)
    if not np.isfinite(J):
        return None
    g4 = R.snap_cost_grad(coef)
    g = np.array([R.weighted(g4[i], w) for i in range(g4.shape[0])])
    return float(J), g, coef


@contextlib.contextmanager
def given_gates(start, end, fix, via):
    """Inside, timeopt_ref.evaluate -- and with it everything built on it -- is the gated boundary-state solve."""
    orig = R.evaluate
    R.evaluate = lambda wp_, t_, w_, ncoef_, cost_fn=None: evaluate(wp_, t_, w_, ncoef_, start, end, fix, via)
    try:
        yield
    finally:
        R.evaluate = orig


def optimize(wp, t, start=None, end=None, fix=None, via=None, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200,
             tol=1e-4, ncoef=8, trace=None):
    """timeopt_ref.optimize with the gated solve as its `evaluate`: the same dict, the same `trace`."""
    with given_gates(start, end, fix, via):
        return R.optimize(wp, t, weights, min_fraction, max_iter, tol, ncoef, None, trace=trace)


def gated_values(coef, fix, via):
    """[(knot i, q, got [4], want [4]), ..]: every gated derivative on the segment that leaves its knot, coef * q!"""
    from math import factorial
    out = []
    for i in range(1, coef.shape[0]):
        for q in range(1, coef.shape[2] // 2):
            if (int(fix[i - 1]) >> (q - 1)) & 1:
                out.append((i, q, coef[i, :, q] * factorial(q), np.asarray(via[i - 1])[:, q - 1]))
    return out


def unpack_cases(z):
    """The drones of tests/golden/timeopt_gates_golden.npz as a list of dicts: k, group, order, combo, min_fraction,
    weights, shared, wp [M+1, 4] float64, t [M+1], start / end [4, K-1] or None, fix [M-1] int32, via [M-1, 4, K-1]
    (NaN under clear bits), and the prefix knots p_t."""
    out = []
    for k in range(int(z["n"])):
        g = int(z["group"][k])
        lo, hi = int(z["off"][k]), int(z["off"][k + 1])
        glo, ghi = int(z["goff"][k]), int(z["goff"][k + 1])      # (M - 1 interior knots per drone)
        order = int(z["order"][g])
        nd = (order + 1) // 2 - 1
        combo = str(z["combo"][k])
        out.append({"k": k, "group": g, "order": order, "combo": combo, "min_fraction": float(z["min_fraction"][g]),
                    "weights": tuple(float(x) for x in z["weights"][g]), "shared": bool(z["shared"][g]),
                    "wp": z["wp"][lo:hi].astype(np.float64), "t": z["t"][lo:hi],
                    "start": z["start"][k][:, :nd].copy() if combo in ("start", "both") else None,
                    "end": z["end"][k][:, :nd].copy() if combo in ("end", "both") else None,
                    "fix": z["fix"][glo:ghi].copy(), "via": z["via"][glo:ghi, :, :nd].copy(),
                    "p_t": (z["p_t1"][lo:hi], z["p_t3"][lo:hi])})
    return out
