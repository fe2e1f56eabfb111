"""What the NumPy fp64 restatements of the certified walks share (csrc/msnap_walk.h; clearance_exact.fp64_clearance,
mesh_clearance_exact.fp64_mesh_clearance), test side only: the Bernstein weights, the Taylor shift, the positions at
absolute times, the stackless walk over the dyadic sub-intervals with its bookkeeping of what was proven, and the
contract's inequalities, which the two headers word alike."""
from __future__ import annotations

from math import comb

import numpy as np

# include/msnap.h, "pairwise clearance" and "mesh clearance": r = ABS_ROUND + c 2^-52 R, c the module's own constant
REL_CLOSE = 1e-9        # lower >= min_dist (1 - REL_CLOSE) - ABS_CLOSE - r when the walk closes
ABS_CLOSE = 1e-9
REL_ROUND = 1e-13       # lower <= D (1 + REL_ROUND) + r and D <= min_dist (1 + REL_ROUND) + r
ABS_ROUND = 1e-13
EPS = 2.0 ** -52


def round_terms(R, c_round):
    """The part of the rounding allowance that does not scale with the distance: ABS_ROUND + c_round 2^-52 R."""
    return ABS_ROUND + c_round * EPS * R


def contract_violations(min_dist, lower, D, closed, R, c_round, lower_le_min_dist):
    """The inequalities of include/msnap.h that (min_dist, lower) break against the exact D (an mpf): a list of text.
    lower_le_min_dist: the mesh clearance's header also states lower <= min_dist."""
    D = float(D)
    r = round_terms(R, c_round)
    bad = []
    if not lower <= D * (1 + REL_ROUND) + r:
        bad.append(f"lower {lower!r} above D {D!r}")
    if not D <= min_dist * (1 + REL_ROUND) + r:
        bad.append(f"min_dist {min_dist!r} below D {D!r}")
    if lower_le_min_dist and not lower <= min_dist:
        bad.append(f"lower {lower!r} above min_dist {min_dist!r}")
    if closed and not lower >= min_dist * (1 - REL_CLOSE) - ABS_CLOSE - r:
        bad.append(f"lower {lower!r} not within the closed-walk bound of min_dist {min_dist!r}")
    return bad


def round_ratio(min_dist, lower, D, R, attained=None):
    """What the module's C_ROUND has to cover, in units of 2^-52 R: the larger of lower - D and D - min_dist, less the
    distance-relative part of the allowance (negative: no coordinate term is needed).  `attained`: the exact distance
    at t_min -- then also |min_dist - attained|, the rounding of the attained value itself, which does not depend on
    whether the walk happened to stop right at the infimum."""
    D = float(D)
    r = max(lower - D * (1 + REL_ROUND), D - min_dist * (1 + REL_ROUND))
    if attained is not None:
        r = max(r, abs(min_dist - float(attained)) - REL_ROUND * float(attained))
    return r / (EPS * R)


def _bernstein_weights(n):
    w = np.zeros((n + 1, n + 1))
    for i in range(n + 1):
        for k in range(i + 1):
            w[i, k] = comb(i, k) / comb(n, k)
    return w


def _taylor(c, a):
    """c [L, D + 1] (ascending) -> coefficients of c(x + a), a [L]; in place on a copy."""
    c = c.copy()
    D = c.shape[1] - 1
    for k in range(D):
        for j in range(D - 1, k - 1, -1):
            c[:, j] = a * c[:, j + 1] + c[:, j]
    return c


def _positions(coef, dur, d, t):
    """msnap_eval_flat's lookup and Horner: positions [P, 3] of drones d [P] at absolute times t [P]."""
    K = np.add.accumulate(dur[d], axis=1)
    seg = np.minimum((t[:, None] > K).sum(axis=1), dur.shape[1] - 1)
    off = np.concatenate([np.zeros((len(d), 1)), K], axis=1)[np.arange(len(d)), seg]
    tl = t - off
    c = coef[d, seg, :3, :]                       # [P, 3, nc]
    v = np.zeros((len(d), 3))
    for j in range(c.shape[2] - 1, -1, -1):
        v = v * tl[:, None] + c[:, :, j]
    return v


def trailing_ones(ix):
    """ix [A] uint64 -> the number of trailing one bits of each [A] int64."""
    up = np.zeros(len(ix), dtype=np.int64)
    tmp = ix.copy()
    while True:
        m = (tmp & np.uint64(1)) == 1
        if not m.any():
            return up
        up += m
        tmp = np.where(m, tmp >> np.uint64(1), tmp)


def take_attained(candidates, best, best_u):
    """(value [A], time [A]) candidates, earlier first, against (best, best_u): the smaller value, then the earlier
    time.  Returns new arrays."""
    nb, nu = best.copy(), best_u.copy()
    for gv, uv in candidates:
        take = (gv < nb) | ((gv == nb) & (uv < nu))
        nb = np.where(take, gv, nb)
        nu = np.where(take, uv, nu)
    return nb, nu


def walk(L, node, max_depth, max_nodes):
    """The walk of L lanes for a minimum, each over the dyadic sub-intervals of [0, 1] (csrc/msnap_walk.h: WalkNode,
    ProvenBound).  node(act, a, hh, best, best_u) -> (bound, nb, nu, wants_split) for the active lanes act at their nodes
    [a, a + hh]: the node's lower bound, the best attained value and its time after the node, and whether the bound
    leaves the node open (it is split unless at max_depth).  Returns (best, best_u, low, nodes, capped) per lane: low is
    what the walk proved, capped the lanes that met the depth cap with an open node or the node guard."""
    best = np.full(L, np.inf)
    best_u = np.zeros(L)
    low = np.full(L, np.inf)
    root = np.full(L, np.inf)
    idx = np.zeros(L, dtype=np.uint64)
    lvl = np.zeros(L, dtype=np.int64)
    nodes = np.zeros(L, dtype=np.int64)
    capped = np.zeros(L, dtype=bool)
    act = np.arange(L)
    while len(act):
        hh = np.ldexp(1.0, -lvl[act])
        a = idx[act].astype(np.float64) * hh
        bound, nb, nu, wants = node(act, a, hh, best[act], best_u[act])
        best[act], best_u[act] = nb, nu
        at_cap = lvl[act] >= max_depth
        split = wants & ~at_cap
        ix = idx[act]
        up = trailing_ones(ix)
        root[act] = np.where(nodes[act] == 0, bound, root[act])
        nodes[act] += 1
        finished = ~split & (up == lvl[act])
        guard = ~finished & (nodes[act] >= max_nodes)
        lw = np.where(split, low[act], np.fmin(low[act], bound))
        low[act] = np.where(guard, np.fmin(lw, root[act]), lw)
        capped[act] |= guard | (wants & at_cap)
        idx[act] = np.where(split, ix << np.uint64(1), (ix >> up.astype(np.uint64)) + np.uint64(1))
        lvl[act] = np.where(split, lvl[act] + 1, lvl[act] - up)
        act = act[~(finished | guard)]
    return best, best_u, low, nodes, capped
