"""Exact reference of the solve with prescribed derivatives at interior waypoints (include/msnap.h, "gates"; DESIGN.md
§5 K21), and the cases of tests/test_gates_cpu.py and tests/test_gates_gpu.py.

exact_solve: the 60-digit collocation of tests/states_exact.py with one row replaced per prescribed derivative.
Prescribing derivative q of the path at interior knot i takes u_i[q] out of the unknowns, and with it the stationarity
condition in u_i[q] -- which is the continuity of derivative 2K-1-q at that knot (order 7: v <-> d6, a <-> d5,
j <-> d4).  That continuity row becomes "derivative q at local time 0 of segment i = value"; the continuity of
derivative q itself stays, so the segment before meets the value too.  The mask is shared by a drone's four axes, so
one LU serves them; the residual of every solution against the unfactored rows is asserted as states_exact does.
"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import states_exact as SE  # noqa: E402
from states_exact import _assemble, _banded_lu_solve, deriv_row  # noqa: E402

mp.mp.dps = 60


def _gated_rows(T, K, fix):
    """states_exact's rows with the replacements of the mask `fix` [M-1]; src gains ("g", i, q): the q-th derivative
    prescribed at knot i"""
    NC, M = 2 * K, len(T)
    rows, src = _assemble(T, K)
    zero = mp.mpf(0)
    for i in range(1, M):
        m = int(fix[i - 1])
        assert 0 <= m < 2 ** (K - 1)
        first = K + (i - 1) * NC + 2              # the row of derivative 1's continuity at knot i
        for q in range(1, K):
            if (m >> (q - 1)) & 1:
                r = first + (2 * K - 1 - q) - 1
                assert src[r] is None
                rows[r] = (NC * (i - 1), [zero] * NC + deriv_row(NC, q, zero))
                src[r] = ("g", i, q)
    return rows, src


def exact_solve(times, wp, start, end, fix, via, K):
    """times [M+1], wp [M+1, 4], start / end [4, K-1] or None (rest), fix [M-1] ints, via [M-1, 4, K-1] (entries under
    a clear bit are not read) -> coef [M, 4, 2K] float64: the 60-digit solution rounded once"""
    NC = 2 * K
    t = [mp.mpf(float(x)) for x in times]
    assert t[0] == 0
    M = len(t) - 1
    T = [t[i + 1] - t[i] for i in range(M)]
    n = NC * M
    rows, src = _gated_rows(T, K, fix)
    assert len(rows) == n
    rhs = []
    for a in range(4):
        col = []
        for s in src:
            if s is None:
                col.append(mp.mpf(0))
            elif s[0] == "w":
                col.append(mp.mpf(float(wp[s[1], a])))
            elif s[0] == "g":
                v = float(via[s[1] - 1, a, s[2] - 1])
                assert np.isfinite(v)
                col.append(mp.mpf(v))
            else:
                blk = start if s[0] == "s" else end
                col.append(mp.mpf(0) if blk is None else mp.mpf(float(blk[a, s[1] - 1])))
        rhs.append(col)
    X = _banded_lu_solve(rows, rhs, n, NC)
    rows0, _ = _gated_rows(T, K, fix)             # the solutions against the unfactored rows
    for x, col in zip(X, rhs):
        scale = max(abs(v) for v in x) + 1
        for (lo, vals), want in zip(rows0, col):
            got = sum((v * x[lo + q] for q, v in enumerate(vals) if v != 0), mp.mpf(0))
            assert abs(got - want) <= scale * mp.mpf(10) ** -45, "residual"
    c = np.empty((M, 4, NC))
    for a in range(4):
        for s in range(M):
            for q in range(NC):
                c[s, a, q] = float(X[a][NC * s + q])
    return c


# ---------------------------------------------------------------------------
# the cases of the tests and their exact solutions
# ---------------------------------------------------------------------------
MAX_SEG = dict(SE.MAX_SEG)         # msnap_solve_gates_max_segments: the gates take no LDS, the range is solve_states'
N_CASE = SE.N_CASE                 # 17: one full 16-drone tile and a partial one
GPU_SEGMENTS = {order: (2, 3, 10, MAX_SEG[order]) for order in (7, 9)}


def masks(order, M, N=N_CASE):
    """fix [N, M-1] int32.  Knot 1 of drone d carries d for d < 2^(K-1) and a non-empty mask after that, so every mask
    value occurs within a 16-drone tile and the empty one once; knots 1 and 2 and knot M-1 are never thinned out, so there are gates at the first knot, at the last one and at
    two adjacent ones; the other knots carry (d + d div 2^(K-1) + 5 (i-1)) mod 2^(K-1) or, one in two, nothing."""
    K = (order + 1) // 2
    nm = 2 ** (K - 1)
    rng = np.random.default_rng(210000 + 100 * order + M)
    fix = np.zeros((N, max(M - 1, 0)), dtype=np.int32)
    for d in range(N):
        for i in range(1, M):
            if i == 1:
                fix[d, 0] = d if d < nm else nm - 1 - (d - nm) % (nm - 1)
            else:
                keep = i in (2, M - 1) or rng.random() < 0.5
                fix[d, i - 1] = (d + d // nm + 5 * (i - 1)) % nm if keep else 0
    return fix


def case(order, M, N=N_CASE):
    """SE.case(order, M) with gates: (wp, t, start, end, fix, via).  The values lie in the STATE_SCALE ranges; via holds
    NaN under every clear bit (such an entry is never used)."""
    K = (order + 1) // 2
    wp, t, start, end = SE.case(order, M, N)
    fix = masks(order, M, N)
    rng = np.random.default_rng(220000 + 100 * order + M)
    via = rng.uniform(-1.0, 1.0, (N, max(M - 1, 0), 4, K - 1)) * np.array(SE.STATE_SCALE[:K - 1])
    used = ((fix[:, :, None] >> np.arange(K - 1)[None, None, :]) & 1).astype(bool)            # [N, M-1, K-1]
    via = np.where(used[:, :, None, :], via, np.nan)
    return wp, t, start, end, fix, via


def golden_path(order):
    """The longest case of each order is recorded (half a minute of mpmath each); one file per order."""
    name = "gates_golden.npz" if order == 7 else "gates_golden_order9.npz"
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)


_REF = {}


def reference(order, M):
    """coef [N, M, 4, 2K] for case(order, M) with both end states: computed here, or read from the recorded file for
    the longest"""
    key = (order, M)
    if key in _REF:
        return _REF[key]
    K = (order + 1) // 2
    wp, t, start, end, fix, via = case(order, M)
    if M == MAX_SEG[order] and os.path.exists(golden_path(order)):
        g = np.load(golden_path(order))
        for name, arr in (("wp", wp), ("t", t), ("start", start), ("end", end), ("fix", fix), ("via", via)):
            assert np.array_equal(g[name], arr, equal_nan=True), f"{golden_path(order)} was recorded for other inputs ({name})"
        ref = g["coef"]
    else:
        ref = compute_reference(order, M)
    _REF[key] = ref
    return ref


def compute_reference(order, M):
    K = (order + 1) // 2
    wp, t, start, end, fix, via = case(order, M)
    ref = np.empty((wp.shape[0], M, 4, 2 * K))
    for d in range(wp.shape[0]):
        ref[d] = exact_solve(t[d], wp[d], start[d], end[d], fix[d], via[d], K)
    return ref


if __name__ == "__main__":      # python tests/gates_exact.py: record the longest case of each order
    for order in (7, 9):
        M = MAX_SEG[order]
        wp, t, start, end, fix, via = case(order, M)
        np.savez_compressed(golden_path(order), wp=wp, t=t, start=start, end=end, fix=fix, via=via,
                            coef=compute_reference(order, M))
        print("recorded", golden_path(order))
