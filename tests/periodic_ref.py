"""float64 NumPy model of periodic_solve_kernel's recurrence (csrc/msnap_periodic.hip).

The Hermite-form system of DESIGN.md §3 with the seam as knot 0 (left segment M-1, right segment 0) is block cyclic
tridiagonal in the knots' derivative vectors u_0 .. u_{M-1}, u_M = u_0:
    O_{i-1}^T u_{i-1} + D_i u_i + O_i u_{i+1} = y_i .
Forward over knots 1..M-1:   S_i = D_i - O_{i-1}^T G_{i-1},  G_i = S_i^-1 O_i,  z_i = S_i^-1 (y_i - O_{i-1}^T z_{i-1}),
                             H_1 = S_1^-1 O_0^T,  H_i = -S_i^-1 O_{i-1}^T H_{i-1}:   u_i = z_i - G_i u_{i+1} - H_i u_0
Backward:                    p_{M-1} = z_{M-1},  Q_{M-1} = G_{M-1} + H_{M-1},
                             p_i = z_i - G_i p_{i+1},  Q_i = H_i - G_i Q_{i+1}:      u_i = p_i - Q_i u_0
Seam:                        (D_0 - O_{M-1}^T Q_{M-1} - O_0 Q_1) u_0 = y_0 - O_{M-1}^T p_{M-1} - O_0 p_1
Then every segment from its two end vectors as recover_segment does.  The same order of steps as the kernel, not the
same rounding: tests/test_periodic_cpu.py holds this model to the 60-digit reference, the GPU tests hold the kernel.
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


def solve(wp, t, K):
    """wp [M+1, 4], t [M+1] -> coef [M, 4, 2K], seam state u_0 [4, K-1]"""
    c = _consts(K)
    wp = np.asarray(wp, dtype=np.float64)
    T = np.diff(np.asarray(t, dtype=np.float64))
    M, NU, KK = len(T), K - 1, 2 * K - 1
    assert M >= 2
    idx = np.arange(1, K)
    dw = np.diff(wp, axis=0)                                                    # [M, 4]

    def P(i):
        return T[i] ** (idx[:, None] + idx[None, :] - float(KK))

    SS = [P(i) * c["HSS"][1:, 1:] for i in range(M)]                            # start side of segment i
    EE = [P(i) * c["HEE"][1:, 1:] for i in range(M)]                            # end side
    O = [P(i) * c["HSE"][1:, 1:] for i in range(M)]                             # couples u_i (rows) to u_{i+1}
    rs = [(T[i] ** (idx - float(KK)) * c["HSE"][1:, 0])[:, None] * dw[i][None, :] for i in range(M)]
    re = [(T[i] ** (idx - float(KK)) * c["HEE"][1:, 0])[:, None] * dw[i][None, :] for i in range(M)]
    D = [EE[i - 1] + SS[i] for i in range(M)]                                   # knot i (i - 1 = -1: segment M-1)
    y = [-(re[i - 1] + rs[i]) for i in range(M)]                                # [NU, 4]

    G, H, z = [None] * M, [None] * M, [None] * M
    OtG, Otz, C = np.zeros((NU, NU)), np.zeros((NU, 4)), O[0].T                 # C: the carried right-hand side of H
    for i in range(1, M):
        S = D[i] - OtG
        G[i] = np.linalg.solve(S, O[i])
        z[i] = np.linalg.solve(S, y[i] - Otz)
        H[i] = np.linalg.solve(S, C)
        OtG, Otz, C = O[i].T @ G[i], O[i].T @ z[i], -(O[i].T @ H[i])
    p, Q = [None] * M, [None] * M
    p[M - 1], Q[M - 1] = z[M - 1], G[M - 1] + H[M - 1]
    for i in range(M - 2, 0, -1):
        p[i] = z[i] - G[i] @ p[i + 1]
        Q[i] = H[i] - G[i] @ Q[i + 1]
    S0 = D[0] - O[M - 1].T @ Q[M - 1] - O[0] @ Q[1]
    u0 = np.linalg.solve(S0, y[0] - O[M - 1].T @ p[M - 1] - O[0] @ p[1])
    u = [u0] + [p[i] - Q[i] @ u0 for i in range(1, M)] + [u0]                   # [M+1][NU, 4]

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
    return coef, np.ascontiguousarray(u0.T)


def solve_batch(wp, t, K):
    """wp [N, M+1, 4], t [N, M+1] or [M+1] -> coef [N, M, 4, 2K], seam [N, 4, K-1]"""
    N, M = wp.shape[0], wp.shape[1] - 1
    coef, seam = np.empty((N, M, 4, 2 * K)), np.empty((N, 4, K - 1))
    for d in range(N):
        coef[d], seam[d] = solve(wp[d], t if t.ndim == 1 else t[d], K)
    return coef, seam
