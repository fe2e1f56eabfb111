"""NumPy restatement of the time allocation (include/msnap.h, "time allocation"; csrc/msnap_timeopt.hip) for the tests
and for tests/golden/make_timeopt_golden.py: the closed-form gradient, the projection, the step rules -- statement by
statement what the kernel does, in fp64, on the oracle's solve.  It differs from the kernel by rounding only."""
import math

import numpy as np

import msnap_oracle as oracle

ARMIJO = 1e-4
MAX_HALVINGS = 30
BOUND_REL = 1e-9


def energy_terms(coef):
    """Terms of the Ostrogradsky energy at a segment's start, in the library's order: coef [..., nc] -> [..., k].
    E = (k! c_k)^2 + 2 sum_{m=1..k-1} (-1)^m (k-m)! c_{k-m} (k+m)! c_{k+m}."""
    coef = np.asarray(coef, dtype=np.float64)
    k = coef.shape[-1] // 2
    f = [float(math.factorial(n)) for n in range(2 * k)]
    terms = [(f[k] * f[k]) * (coef[..., k] * coef[..., k])]
    for m in range(1, k):
        k2 = (-2.0 if m & 1 else 2.0) * f[k - m] * f[k + m]
        terms.append((k2 * coef[..., k - m]) * coef[..., k + m])
    return np.stack(terms, axis=-1)


def snap_cost_grad(coef):
    """-E per segment and axis: coef [..., M, 4, nc] -> [..., M, 4], the terms summed left to right."""
    t = energy_terms(coef)
    e = t[..., 0]
    for m in range(1, t.shape[-1]):
        e = e + t[..., m]
    return -e


def fast_cost(coef, dur):
    """The snap cost per axis [4] by the monomial Hessian (what msnap_snap_cost evaluates); equals oracle.snap_cost
    to rounding and is some hundred times faster."""
    M, _, nc = coef.shape
    k = nc // 2
    fac = np.array([math.factorial(k + q) / math.factorial(q) for q in range(k)])
    f = coef[:, :, k:] * fac                                   # [M, 4, k]
    e = np.arange(k)[:, None] + np.arange(k)[None, :] + 1      # exponent of T
    Q = dur[:, None, None] ** e[None] / e[None]                # [M, k, k]
    return np.einsum("map,mpq,maq->a", f, Q, f)


def weighted(v, w):
    p = [0.0 if w[a] == 0 else w[a] * v[a] for a in range(4)]
    return ((p[0] + p[1]) + p[2]) + p[3]


def evaluate(wp, t, w, ncoef, cost_fn=None):
    """One trial: (J, g [M], coef) for the knot times t; None when the solve fails."""
    try:
        coef, dur = oracle.solve_batch_fast(wp[None], t[None], ncoef)
    except np.linalg.LinAlgError:
        return None
    coef, dur = coef[0], dur[0]
    J = weighted((cost_fn or oracle.snap_cost)(coef, dur), w)
    if not np.isfinite(J):
        return None
    g4 = snap_cost_grad(coef)
    g = np.array([weighted(g4[i], w) for i in range(g4.shape[0])])
    return float(J), g, coef


def floor_of(t, min_fraction):
    M = len(t) - 1
    return min_fraction * t[M] / M


def start_times(t, Tmin):
    """Durations below the floor raised to it, the others' excess scaled by one factor: the sum is kept."""
    T = np.diff(t)
    below = T < Tmin
    if not below.any():
        return t.copy()
    excess = float(np.sum(np.where(below, Tmin - T, 0.0)))
    slack = float(np.sum(np.where(below, 0.0, T - Tmin)))
    keep = max(1.0 - excess / slack, 0.0) if slack > 0 else 0.0
    out = np.zeros_like(t)
    for i in range(len(T)):
        Tn = Tmin if below[i] else Tmin + (T[i] - Tmin) * keep
        out[i + 1] = t[-1] if i == len(T) - 1 else out[i] + Tn
    return out


def direction(t, g, Tmin):
    """-P g and what the step rules need of it: (d, |d|^2, max |d_i|, min T_i, cap)."""
    T = np.diff(t)
    M = len(T)
    fixed = np.zeros(M, dtype=bool)
    while True:
        cnt = int((~fixed).sum())
        mean = float(np.sum(np.where(fixed, 0.0, g))) / cnt if cnt > 0 else 0.0
        leaves = ~fixed & (T - Tmin <= BOUND_REL * Tmin) & (mean - g < 0.0)
        if not leaves.any():
            break
        fixed |= leaves
    d = np.where(fixed, 0.0, mean - g)
    neg = d < 0.0
    cap = float(np.min((T[neg] - Tmin) / -d[neg])) if neg.any() else math.inf
    return d, float(np.sum(d * d)), float(np.max(np.abs(d))), float(np.min(T)), cap


def trial_times(t, d, step, Tmin):
    T = np.diff(t)
    out = np.zeros_like(t)
    for i in range(len(T)):
        Tn = max(T[i] + step * d[i], Tmin)
        out[i + 1] = t[-1] if i == len(T) - 1 else out[i] + Tn
    return out


def measure(n2, J, ttotal, M):
    return math.sqrt(n2) * ttotal / (math.sqrt(M) * J) if J > 0 else 0.0


def optimize(wp, t, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200, tol=1e-4, ncoef=8, cost_fn=None, trace=None):
    """-> dict(t_out, cost0, cost, pg, iters, solves); the input must be a valid one (t[0] == 0, increasing).
    `trace`, a list, receives one (step, accepted, margin) per trial, margin = |J_new - (J - ARMIJO step |P g|^2)| / J:
    how far the trial was from the other decision (inf when its solve failed).  It changes nothing else."""
    wp = np.asarray(wp, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    w = [float(x) for x in weights]
    M = len(t) - 1
    ttotal = float(t[M])
    Tmin = floor_of(t, min_fraction)
    tc = start_times(t, Tmin)
    ev = evaluate(wp, tc, w, ncoef, cost_fn)
    if ev is None:
        raise ValueError("the solve fails at the input times")
    J, g, _ = ev
    J0, solves, iters, nback = J, 1, 0, 0
    d, n2, dmax, Tsmall, cap = direction(tc, g, Tmin)
    pg = measure(n2, J, ttotal, M)
    prop = 0.25 * Tsmall / dmax if dmax > 0 else math.inf
    step = min(prop, cap)
    run = pg > tol and max_iter > 0 and dmax > 0 and step > 0
    while run:
        tt = trial_times(tc, d, step, Tmin)
        ev = evaluate(wp, tt, w, ncoef, cost_fn)
        solves += 1
        accept = ev is not None and ev[0] <= J - ARMIJO * step * n2
        if trace is not None:
            trace.append((step, accept, abs(ev[0] - (J - ARMIJO * step * n2)) / J if ev is not None else math.inf))
        capped = step >= cap
        if accept:
            J, g, _ = ev
            tc = tt
            iters += 1
            d, n2, dmax, Tsmall, cap = direction(tc, g, Tmin)
            pg = measure(n2, J, ttotal, M)
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
    return {"t_out": tc, "cost0": J0, "cost": J, "pg": pg, "iters": iters, "solves": solves}


def unpack_cases(z):
    """The drones of tests/golden/timeopt_wide_golden.npz (flat arrays) as a list of dicts: k, group, order,
    min_fraction, weights, shared, wp [M+1, 4] float64, t [M+1], and the prefix knots p_t (max_iter 1, 3)."""
    out = []
    for k in range(int(z["n"])):
        g = int(z["group"][k])
        lo, hi = int(z["off"][k]), int(z["off"][k + 1])
        out.append({"k": k, "group": g, "order": int(z["order"][g]), "min_fraction": float(z["min_fraction"][g]),
                    "weights": tuple(float(x) for x in z["weights"][g]), "shared": bool(z["shared"][g]),
                    "wp": z["wp"][lo:hi].astype(np.float64), "t": z["t"][lo:hi],
                    "p_t": (z["p_t1"][lo:hi], z["p_t3"][lo:hi])})
    return out
