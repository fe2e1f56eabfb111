"""References for the path extent (include/msnap.h, "path extent"), test side only.

exact_extent: the coefficients, the fp64 knot times (running sums, as the library forms them) and the direction taken as
exact Fractions; per segment q = n.p as an exact rational polynomial in the segment's local time, the real roots of q'
in [0, T] from mpmath.polyroots at 60 digits, q there and at both ends; S = the maximum, at its earliest time.
fp64_extent: a plain NumPy fp64 restatement of the kernel's walk (csrc/msnap_extent.hip) on dyadic_walk's helpers,
vectorised over the (drone, segment, direction) lanes -- for the node counts and for measuring the rounding of the fp64
method against exact_extent.  Not bit-exact with the kernel (no fused multiply-add here)."""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

import clearance_exact as CE
import dyadic_walk as DW
from clearance_exact import DPS      # (exact_interval_min brings _mpf, _squarefree and the root finding with it)
from dyadic_walk import EPS, _bernstein_weights, _positions, _taylor

# include/msnap.h, "path extent": ext <= S + r, S <= upper + r, r = ABS_ROUND + C_ROUND_EXTENT 2^-52 R_k, and
# upper <= ext + REL_CLOSE |ext| + ABS_CLOSE + r when the walk closes
C_ROUND_EXTENT = 9.0    # ten times the worst measured, 0.86 (tools/extent_rounding.py), rounded up
ABS_ROUND = 1e-13
REL_CLOSE = 1e-9
ABS_CLOSE = 1e-9
# csrc/msnap_extent.hip
MAX_DEPTH = 40
MAX_NODES = 4096
PRUNE_REL = 1e-9
PRUNE_ABS = 1e-9


def extent_R(coef_d, dur_d, n):
    """R_k of include/msnap.h for one drone (coef [M, 4, nc], dur [M]) and one direction n [3]: the largest value over
    the segments i of sum_a |n_a| sum_j |c_{a,j}| T_i^j."""
    coef_d, dur_d, n = np.asarray(coef_d, dtype=np.float64), np.asarray(dur_d, dtype=np.float64), np.abs(np.asarray(n, dtype=np.float64))
    pw = dur_d[:, None] ** np.arange(coef_d.shape[2])[None, :]                     # [M, nc]
    per_axis = (np.abs(coef_d[:, :3, :]) * pw[:, None, :]).sum(axis=2)             # [M, 3]
    return float((per_axis * n[None, :]).sum(axis=1).max())


def round_terms(R):
    return ABS_ROUND + C_ROUND_EXTENT * EPS * R


def _scalar(coef_d, i, n):
    """q = n.p of segment i as exact Fractions (ascending)."""
    nf = [Fraction(float(x)) for x in n]
    return [sum(nf[a] * Fraction(float(coef_d[i, a, j])) for a in range(3)) for j in range(coef_d.shape[2])]


def exact_extent(coef_d, dur_d, n, segments=None):
    """coef [M, 4, nc], dur [M] of one drone, n [3] -> (S, t) as mpf: the supremum of n.p over the whole path, each
    segment on its closed [0, T_i], and the earliest absolute time that attains it.  `segments`: the indices of the
    segments that can hold it (default: all) -- candidate_segments tells them from the fp64 bounds."""
    k = CE.knots(dur_d)
    starts = [0.0] + k[:-1]
    best, bt = None, None
    with mpmath.workdps(DPS):
        for i in range(len(k)):
            if segments is not None and i not in segments:
                continue
            q = _scalar(coef_d, i, n)
            v, tau = CE.exact_interval_min([-x for x in q], Fraction(0), Fraction(float(dur_d[i])))
            v, t = -v, mpmath.mpf(starts[i]) + tau
            if best is None or v > best or (v == best and t < bt):
                best, bt = v, t
        return best, bt


def exact_value_at(coef_d, dur_d, n, t):
    """n.p(t) as mpf at an absolute time t (a float), through msnap_eval_flat's lookup."""
    with mpmath.workdps(DPS):
        t = mpmath.mpf(t)
        k = CE.knots(dur_d)
        i = next((i for i, x in enumerate(k) if t <= x), len(k) - 1)
        tl = t - ([0.0] + k)[i]
        return sum(mpmath.mpf(float(n[a])) * mpmath.polyval([mpmath.mpf(float(x)) for x in coef_d[i, a][::-1]], tl)
                   for a in range(3))


def contract_violations(ext, upper, S, closed=True, R=0.0):
    """The inequalities of include/msnap.h that (ext, upper) break against the exact S (an mpf): a list of text.
    dyadic_walk.contract_violations, mirrored for a maximum.  `R`: extent_R (0: the allowance without its coordinate
    term, which is stricter)."""
    S = float(S)
    r = round_terms(R)
    bad = []
    if not ext <= upper:
        bad.append(f"ext {ext!r} above upper {upper!r}")
    if not ext <= S + r:
        bad.append(f"ext {ext!r} above S {S!r}")
    if not S <= upper + r:
        bad.append(f"upper {upper!r} below S {S!r}")
    if closed and not upper <= ext + REL_CLOSE * abs(ext) + ABS_CLOSE + r:
        bad.append(f"upper {upper!r} not within the closed-walk bound of ext {ext!r}")
    return bad


def round_ratio(ext, upper, S, R, attained=None):
    """What C_ROUND_EXTENT has to cover, in units of 2^-52 R_k: the largest of ext - S, S - upper and (with `attained`,
    the exact value at t_ext) |ext - attained|."""
    S = float(S)
    r = max(ext - S, S - upper)
    if attained is not None:
        r = max(r, abs(ext - float(attained)))
    return r / (EPS * R)


def unfused_dot(n, p):
    """(n_x x + n_y y) + n_z z, every operation rounded once: n [..., 3], p [..., 3]."""
    return (n[..., 0] * p[..., 0] + n[..., 1] * p[..., 1]) + n[..., 2] * p[..., 2]


# ------------------------------------------------------------------------------------------------ fp64 restatement
def fp64_extent(coef, dur, dirs, stats=None):
    """coef [N, M, 4, nc], dur [N, M] (finite, durations > 0), dirs [K, 3] (finite) -> (ext, t_ext, upper), each
    [N, K], by the kernel's method in NumPy fp64.  `stats` (a dict) receives the nodes per lane ("nodes", [N, M, K]),
    the lanes that met the depth cap or the node guard ("capped") and the lanes' proven upper bounds ("lane_upper")."""
    coef, dur, dirs = (np.asarray(x, dtype=np.float64) for x in (coef, dur, dirs))
    N, M, nc = dur.shape[0], dur.shape[1], coef.shape[3]
    K, D = dirs.shape[0], nc - 1
    Wt = _bernstein_weights(D)
    di, si, ki = (x.reshape(-1) for x in np.meshgrid(np.arange(N), np.arange(M), np.arange(K), indexing="ij"))
    L = len(di)
    ends = np.add.accumulate(dur, axis=1)
    starts = np.concatenate([np.zeros((N, 1)), ends[:, :-1]], axis=1)
    T, t0 = dur[di, si], starts[di, si]
    E = t0 + T
    c = coef[di, si, :3, :]                                                           # [L, 3, nc]
    n = dirs[ki]
    q = n[:, 2:3] * c[:, 2, :] + (n[:, 1:2] * c[:, 1, :] + n[:, 0:1] * c[:, 0, :])
    e = -(q * T[:, None] ** np.arange(D + 1))

    def node(act, a, hh, best, best_u):
        f = _taylor(e[act], a) * hh[:, None] ** np.arange(D + 1)
        vm = np.zeros(len(act))
        v1 = np.zeros(len(act))
        for j in range(D, -1, -1):
            vm = vm * 0.5 + f[:, j]
            v1 = v1 + f[:, j]
        bound = (f @ Wt.T).min(axis=1)
        nb, nu = DW.take_attained(((f[:, 0], a), (vm, a + 0.5 * hh), (v1, a + hh)), best, best_u)
        return bound, nb, nu, bound < nb - PRUNE_REL * np.abs(nb) - PRUNE_ABS

    best, best_u, low, nodes, capped = DW.walk(L, node, MAX_DEPTH, MAX_NODES)
    tm = np.minimum(T * best_u + t0, E)
    val = unfused_dot(n, _positions(coef, dur, di, tm)).reshape(N, M, K)
    tm = tm.reshape(N, M, K)
    ext = val.max(axis=1)
    t_ext = np.where(val == ext[:, None, :], tm, np.inf).min(axis=1)
    upper = np.maximum((-low).reshape(N, M, K).max(axis=1), ext)
    if stats is not None:
        stats["nodes"] = nodes.reshape(N, M, K)
        stats["capped"] = capped.reshape(N, M, K)
        stats["lane_upper"] = (-low).reshape(N, M, K)
    return ext, t_ext, upper


def candidate_segments(coef, dur, dirs, rel=1e-6):
    """[N][K] sets of the segments whose fp64 upper bound is within `rel` of the (drone, direction)'s largest attained
    value: the only ones that can hold the supremum (exact_extent's `segments`)."""
    st = {}
    ext, _, _ = fp64_extent(coef, dur, dirs, stats=st)
    keep = st["lane_upper"] >= ext[:, None, :] - rel * np.abs(ext[:, None, :]) - 1e-9
    return [[set(np.nonzero(keep[d, :, k])[0].tolist()) for k in range(keep.shape[2])] for d in range(keep.shape[0])]


# ------------------------------------------------------------------------------------------------ shared test helper
def check_contract(path_extent, eval_flat, coef, dur, dirs, with_R=True, closed=True, pick=None):
    """`path_extent(coef, dur, dirs)` (Context.path_extent, or the restatement behind the same signature): no status
    raised, ext <= upper, 0 <= t_ext <= total everywhere; against exact_extent (on the candidate segments) the header's
    inequalities for every (drone, direction) -- or for those of `pick`, a list of (drone, direction), where the exact
    reference on all of them would take too long.  `eval_flat(coef, dur, ts)` or None: with it, the attained claim bit
    for bit.  Returns (ext, t_ext, upper, worst round_ratio)."""
    coef, dur, dirs = (np.asarray(x, dtype=np.float64) for x in (coef, dur, dirs))
    ext, t_ext, upper, status = path_extent(coef, dur, dirs)
    N, K = ext.shape
    assert (status == 0).all()
    total = np.add.accumulate(dur, axis=1)[:, -1]
    assert (ext <= upper).all() and (t_ext >= 0.0).all() and (t_ext <= total[:, None]).all()
    if eval_flat is not None:
        for d in range(N):
            pos = eval_flat(coef[d:d + 1], dur[d:d + 1], t_ext[d])[0, :, :3]          # [K, 3]
            assert np.array_equal(unfused_dot(dirs, pos), ext[d]), d
    cands = candidate_segments(coef, dur, dirs)
    worst = 0.0
    for d, k in (pick if pick is not None else [(d, k) for d in range(N) for k in range(K)]):
        S, _ = exact_extent(coef[d], dur[d], dirs[k], cands[d][k])
        R = extent_R(coef[d], dur[d], dirs[k])
        bad = contract_violations(ext[d, k], upper[d, k], S, closed=closed, R=R if with_R else 0.0)
        assert not bad, (d, k, bad)
        if R > 0.0:
            worst = max(worst, round_ratio(ext[d, k], upper[d, k], S, R, exact_value_at(coef[d], dur[d], dirs[k], t_ext[d, k])))
    print(f"worst rounding / (2^-52 R): {worst:.3f} (C_ROUND_EXTENT {C_ROUND_EXTENT})")
    assert worst < C_ROUND_EXTENT
    return ext, t_ext, upper, worst


def restated(coef, dur, dirs):
    """fp64_extent behind Context.path_extent's signature."""
    ext, t_ext, upper = fp64_extent(coef, dur, dirs)
    return ext, t_ext, upper, np.zeros(ext.shape[0], dtype=np.int32)
