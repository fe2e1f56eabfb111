"""NumPy restatement of the time allocation with a free total duration (include/msnap.h, msnap_optimize_times_free;
csrc/msnap_timeopt_kernel.h with kTimeoptFree) for the tests and for tests/golden/make_timeopt_free_golden.py.

F(T) = sum_a w_a J_a(T) + k_T sum_i T_i over all segment durations, from and to given end states.  The solve, its
cost and the closed-form gradient -sum_a w_a E_i,a are tests/timeopt_states_ref.py's (the dense fp64 collocation system
of tests/states_exact.py); what is restated here is what the free mode changes: the raise of short durations that
nothing pays for, the gradient's time term, a direction without projection, a last knot that moves, and the current
total in the stopping measure.  The step rules are tests/timeopt_ref.py's constants and statements."""
import math

import numpy as np

import timeopt_ref as R
import timeopt_states_ref as S

ARMIJO, MAX_HALVINGS, BOUND_REL = R.ARMIJO, R.MAX_HALVINGS, R.BOUND_REL


def floor_of(t, min_fraction):
    """T_min = min_fraction t[M] / M, from the input total"""
    return R.floor_of(t, min_fraction)


def start_times(t, Tmin):
    """Durations below the floor raised to it, every other one the input's: the sum may grow.  An input with nothing
    below the floor is returned bit for bit; otherwise the knots are the running sum from 0."""
    T = np.diff(t)
    if not (T < Tmin).any():
        return t.copy()
    out = np.zeros_like(t)
    for i in range(len(T)):
        out[i + 1] = out[i] + (Tmin if T[i] < Tmin else T[i])
    return out


def evaluate(wp, t, w, kT, ncoef, start=None, end=None):
    """One trial: (F, g [M], J, coef) for the knot times t, g_i = k_T - sum_a w_a E_i,a; None when the solve fails."""
    ev = S.evaluate(wp, t, w, ncoef, start, end)
    if ev is None:
        return None
    J, gJ, coef = ev
    F = J + kT * float(t[-1])
    if not np.isfinite(F):
        return None
    return float(F), kT + gJ, float(J), coef


def direction(t, g, Tmin):
    """-g off the floor and what the step rules need of it: (d, |d|^2, max |d_i|, min T_i, cap).  One pass: a segment
    within T_min (1 + 1e-9) whose gradient is positive is not free."""
    T = np.diff(t)
    fixed = (T - Tmin <= BOUND_REL * Tmin) & (g > 0.0)
    d = np.where(fixed, 0.0, -g)
    neg = d < 0.0
    cap = float(np.min((T[neg] - Tmin) / -d[neg])) if neg.any() else math.inf
    return d, float(np.sum(d * d)), float(np.max(np.abs(d))), float(np.min(T)), cap


def trial_times(t, d, step, Tmin):
    """the running sum of max(T_i + step d_i, T_min) from 0, the last knot included"""
    T = np.diff(t)
    out = np.zeros_like(t)
    for i in range(len(T)):
        out[i + 1] = out[i] + max(T[i] + step * d[i], Tmin)
    return out


def measure(n2, F, total, M):
    return math.sqrt(n2) * total / (math.sqrt(M) * F) if F > 0 else 0.0


def optimize(wp, t, start=None, end=None, weights=(1, 1, 1, 1), time_weight=1.0, min_fraction=0.1, max_iter=200,
             tol=1e-4, ncoef=8, trace=None, grad_noise=None):
    """-> dict(t_out, cost0, cost, J, pg, iters, solves); the input must be a valid one (t[0] == 0, increasing,
    time_weight > 0).  `trace` receives one (step, accepted, margin) per trial as timeopt_ref.optimize's does.
    `grad_noise(g)`, when given, replaces every gradient (the generator's sensitivity runs)."""
    wp = np.asarray(wp, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    w = [float(x) for x in weights]
    kT = float(time_weight)
    M = len(t) - 1
    Tmin = floor_of(t, min_fraction)
    tc = start_times(t, Tmin)

    def ev_at(tt):
        ev = evaluate(wp, tt, w, kT, ncoef, start, end)
        if ev is not None and grad_noise is not None:
            ev = (ev[0], grad_noise(ev[1])) + ev[2:]
        return ev

    ev = ev_at(tc)
    if ev is None:
        raise ValueError("the solve fails at the input times")
    F, g, J, _ = ev
    F0, solves, iters, nback = F, 1, 0, 0
    d, n2, dmax, Tsmall, cap = direction(tc, g, Tmin)
    pg = measure(n2, F, float(tc[-1]), M)
    prop = 0.25 * Tsmall / dmax if dmax > 0 else math.inf
    step = min(prop, cap)
    run = pg > tol and max_iter > 0 and dmax > 0 and step > 0
    while run:
        tt = trial_times(tc, d, step, Tmin)
        ev = ev_at(tt)
        solves += 1
        accept = ev is not None and ev[0] <= F - ARMIJO * step * n2
        if trace is not None:
            trace.append((step, accept, abs(ev[0] - (F - ARMIJO * step * n2)) / F if ev is not None else math.inf))
        capped = step >= cap
        if accept:
            F, g, J, _ = ev
            tc = tt
            iters += 1
            d, n2, dmax, Tsmall, cap = direction(tc, g, Tmin)
            pg = measure(n2, F, float(tc[-1]), M)
            nprop = prop if capped else 2.0 * step
            nback = 0
            nxt = min(nprop, cap)
            done = (not pg > tol) or iters >= max_iter or (not dmax > 0) or (not nxt > 0)
        else:
            nprop = 0.5 * step
            nback += 1
            nxt = min(nprop, cap)
            done = nback >= MAX_HALVINGS
        step, prop = nxt, nprop
        run = not done
    return {"t_out": tc, "cost0": F0, "cost": F, "J": J, "pg": pg, "iters": iters, "solves": solves}


def unpack_cases(z):
    """The drones of tests/golden/timeopt_free_golden.npz as a list of dicts: k, group, kind, order, combo,
    min_fraction, weights, shared, time_weight, wp [M+1, 4] float64, t [M+1], start / end [4, K-1] or None, and the
    prefix knots p_t."""
    out = []
    for k in range(int(z["n"])):
        g = int(z["group"][k])
        lo, hi = int(z["off"][k]), int(z["off"][k + 1])
        order = int(z["order"][g])
        nd = (order + 1) // 2 - 1
        combo = str(z["combo"][k])
        out.append({"k": k, "group": g, "kind": str(z["kind"][g]), "order": order, "combo": combo,
                    "min_fraction": float(z["min_fraction"][g]), "weights": tuple(float(x) for x in z["weights"][g]),
                    "shared": bool(z["shared"][g]), "time_weight": float(z["time_weight"][k]),
                    "wp": z["wp"][lo:hi].astype(np.float64), "t": z["t"][lo:hi],
                    "start": z["start"][k][:, :nd].copy() if combo in ("start", "both") else None,
                    "end": z["end"][k][:, :nd].copy() if combo in ("end", "both") else None,
                    "p_t": (z["p_t1"][lo:hi], z["p_t3"][lo:hi])})
    return out
