"""float64 NumPy model of gates_solve_kernel's masked sweep (csrc/msnap_gates.hip, Sweep<K>::chain_masked; DESIGN.md
§5 K21).

The Hermite-form system of DESIGN.md §3 over the interior knots' derivative vectors u_1 .. u_{M-1}, with u_0, u_M data:
    O_{i-1}^T u_{i-1} + D_i u_i + O_i u_{i+1} = y_i .
Forward over knots 1..M-1:   S = D_i - O_{i-1}^T G_{i-1},  y = y_i - O_{i-1}^T z_{i-1}  (knot 1: O_0^T u_0);
        for every prescribed component c of u_i:  y[free] -= S[free, c] g[c];  row and column c of S become the
        identity's;  y[c] = g[c];  the G solve takes O_i with row c zeroed;
        G_i = S^-1 O_i(zeroed),  z_i = S^-1 y;  the carry O_i^T G_i, O_i^T z_i uses the whole O_i.
Backward:                    u_i = z_i - G_i u_{i+1} from u_M.
Then every segment from its two end vectors as recover_segment does.  The same order of steps as the kernel, not the
same rounding (and no refine_end): tests/test_gates_cpu.py holds this model to the 60-digit reference, the GPU tests
hold the kernel.
"""
import os
import sys
from math import factorial

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_consts  # noqa: E402

_C = {}


def _consts(K):
    if K not in _C:
        c = gen_consts.consts(K)
        _C[K] = {n: np.array([[float(v) for v in row] for row in c[n]]) for n in ("HSS", "HSE", "HEE", "CS", "CE")}
    return _C[K]


def solve(wp, t, start, end, fix, via, K):
    """wp [M+1, 4], t [M+1], start / end [4, K-1] or None, fix [M-1], via [M-1, 4, K-1] -> coef [M, 4, 2K]"""
    c = _consts(K)
    wp = np.asarray(wp, dtype=np.float64)
    T = np.diff(np.asarray(t, dtype=np.float64))
    M, NU, KK = len(T), K - 1, 2 * K - 1
    idx = np.arange(1, K)
    dw = np.diff(wp, axis=0)                                                    # [M, 4]
    u0 = np.zeros((NU, 4)) if start is None else np.asarray(start, dtype=np.float64).T
    uM = np.zeros((NU, 4)) if end is None else np.asarray(end, dtype=np.float64).T

    def P(i):
        return T[i] ** (idx[:, None] + idx[None, :] - float(KK))

    SS = [P(i) * c["HSS"][1:, 1:] for i in range(M)]                            # start side of segment i
    EE = [P(i) * c["HEE"][1:, 1:] for i in range(M)]                            # end side
    O = [P(i) * c["HSE"][1:, 1:] for i in range(M)]                             # couples u_i (rows) to u_{i+1}
    rs = [(T[i] ** (idx - float(KK)) * c["HSE"][1:, 0])[:, None] * dw[i][None, :] for i in range(M)]
    re = [(T[i] ** (idx - float(KK)) * c["HEE"][1:, 0])[:, None] * dw[i][None, :] for i in range(M)]

    G, z = [None] * M, [None] * M
    OtG, Otz = np.zeros((NU, NU)), O[0].T @ u0
    for i in range(1, M):
        S = EE[i - 1] + SS[i] - OtG
        y = -(re[i - 1] + rs[i]) - Otz                                          # [NU, 4]
        Oz = O[i].copy()
        fixed = [q for q in range(NU) if (int(fix[i - 1]) >> q) & 1]
        free = [q for q in range(NU) if q not in fixed]
        g = np.asarray(via[i - 1], dtype=np.float64).T                          # [NU, 4]
        for q in fixed:
            y[free] -= S[free, q][:, None] * g[q][None, :]
        for q in fixed:
            S[q, :] = 0.0
            S[:, q] = 0.0
            S[q, q] = 1.0
            y[q] = g[q]
            Oz[q, :] = 0.0
        G[i] = np.linalg.solve(S, Oz)
        z[i] = np.linalg.solve(S, y)
        OtG, Otz = O[i].T @ G[i], O[i].T @ z[i]
    u = [None] * (M + 1)
    u[0], u[M] = u0, uM
    for i in range(M - 1, 0, -1):
        u[i] = z[i] - G[i] @ u[i + 1]

    coef = np.zeros((M, 4, 2 * K))
    for i in range(M):
        pw = (T[i] ** np.arange(K))[:, None]
        es = np.vstack([np.zeros((1, 4)), u[i]]) * pw
        ee = np.vstack([dw[i][None, :], u[i + 1]]) * pw
        ahi = c["CS"] @ es + c["CE"] @ ee
        coef[i, :, 0] = wp[i]
        for m in range(1, K):
            coef[i, :, m] = u[i][m - 1] / factorial(m)
        for m in range(K):
            coef[i, :, K + m] = ahi[m] * T[i] ** (-(K + m))
    return coef


def solve_batch(wp, t, start, end, fix, via, K):
    """wp [N, M+1, 4], t [N, M+1] or [M+1], start / end [N, 4, K-1] or None, fix [N, M-1], via [N, M-1, 4, K-1]
    -> coef [N, M, 4, 2K]"""
    N, M = wp.shape[0], wp.shape[1] - 1
    coef = np.empty((N, M, 4, 2 * K))
    for d in range(N):
        coef[d] = solve(wp[d], t if t.ndim == 1 else t[d], None if start is None else start[d],
                        None if end is None else end[d], fix[d], via[d], K)
    return coef
