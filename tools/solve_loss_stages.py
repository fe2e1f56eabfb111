#!/usr/bin/env python3
"""Where the K1 solve loses its digits at order 9: the stages of the algorithm of DESIGN.md section 3 (reduced block
tridiagonal system in the knots' derivatives, solve, recovery of the monomial coefficients), each replaced in turn by
60-digit arithmetic, on the inputs of tests/solve_cases.py against the 60-digit solutions of tests/solve_exact.py.
fp64 here is NumPy's on the CPU with gen_consts.py's model of the kernel (model_solve's assembly and recovery), not the
kernel's instruction sequence: the columns say which stage CAN produce the kernels' error, the kernels' own figures of
profiles/solve_accuracy.jsonl stand beside them.

  cond(R)       2-norm condition number of the reduced system
  entries       the reduced system with its entries rounded to fp64 (constants, powers of T, products) solved at 60 digits:
                the error the ROUNDING OF THE SYSTEM alone puts into the knot derivatives, max |u - u_exact| / max |u_exact|
  solve: block  fp64 block sweep without pivoting across blocks (S_i = D_i - O^T G, Cholesky per block) + fp64 recovery
  solve: dense  fp64 LU with partial pivoting of the same reduced system + fp64 recovery
  solve: 60 dig the rounded system solved at 60 digits + fp64 recovery
  recovery      exact knot derivatives (rounded once) through the fp64 recovery alone
  (the last four: conftest.norm_rel of the coefficients, worst drone of the eight with t[0] == 0)

usage: solve_loss_stages.py [order] > profiles/solve_loss_stages.md.  No GPU; about two minutes."""
import json
import os
import sys
from math import factorial

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import gen_consts  # noqa: E402
import solve_cases as SC  # noqa: E402
import solve_exact as SX  # noqa: E402
from conftest import norm_rel  # noqa: E402

mp.mp.dps = 60


def reduced_system(wp, t, k, c):
    """gen_consts.model_solve's assembly: R u = rhs, u = (d^1..d^(k-1)) at the interior knots, four axes"""
    HSS, HSE, HEE = c["HSS"], c["HSE"], c["HEE"]
    KK, M, T, nu = 2 * k - 1, len(t) - 1, np.diff(t), k - 1
    R = np.zeros((nu * (M - 1), nu * (M - 1)))
    rhs = np.zeros((nu * (M - 1), 4))
    idx = np.arange(1, k)
    for i in range(1, M):
        r0 = nu * (i - 1)
        Pm = T[i - 1] ** (idx[:, None] + idx[None, :] - KK)
        Pp = T[i] ** (idx[:, None] + idx[None, :] - KK)
        R[r0:r0 + nu, r0:r0 + nu] = Pm * HEE[1:, 1:] + Pp * HSS[1:, 1:]
        if i + 1 < M:
            R[r0:r0 + nu, r0 + nu:r0 + 2 * nu] = Pp * HSE[1:, 1:]
            R[r0 + nu:r0 + 2 * nu, r0:r0 + nu] = (Pp * HSE[1:, 1:]).T
        rhs[r0:r0 + nu] = -((T[i - 1] ** (idx - KK) * HEE[1:, 0])[:, None] * (wp[i] - wp[i - 1])[None, :]
                            + (T[i] ** (idx - KK) * HSE[1:, 0])[:, None] * (wp[i + 1] - wp[i])[None, :])
    return R, rhs, T


def recover(u, wp, T, k, c):
    """gen_consts.model_solve's recovery of the monomial coefficients from the knots' derivatives"""
    M, nu = len(T), k - 1
    d = np.zeros((M + 1, k, 4))
    d[:, 0, :] = wp
    for i in range(1, M):
        d[i, 1:, :] = u[nu * (i - 1):nu * i]
    coef = np.zeros((M, 4, 2 * k))
    for i in range(M):
        pw = (T[i] ** np.arange(k))[:, None]
        es, ee = d[i] * pw, d[i + 1] * pw
        es[0] = 0.0
        ee[0] = wp[i + 1] - wp[i]
        ahi = c["CS"] @ es + c["CE"] @ ee
        for m in range(k):
            coef[i, :, m] = d[i, m] / factorial(m)
            coef[i, :, k + m] = ahi[m] * T[i] ** (-(k + m))
    return coef


def block_sweep(R, rhs, nu):
    """DESIGN.md section 3's recurrence: no pivoting across blocks, each S_i factored as an SPD block"""
    n = R.shape[0] // nu
    G, z = [], []
    for i in range(n):
        S = R[nu * i:nu * i + nu, nu * i:nu * i + nu].copy()
        y = rhs[nu * i:nu * i + nu].copy()
        if i:
            O = R[nu * (i - 1):nu * i, nu * i:nu * i + nu]
            S -= O.T @ G[-1]
            y -= O.T @ z[-1]
        L = np.linalg.cholesky(S)
        solve = lambda B: np.linalg.solve(L.T, np.linalg.solve(L, B))      # noqa: E731
        G.append(solve(R[nu * i:nu * i + nu, nu * (i + 1):nu * (i + 2)]) if i + 1 < n else None)
        z.append(solve(y))
    u = [None] * n
    u[n - 1] = z[n - 1]
    for i in range(n - 2, -1, -1):
        u[i] = z[i] - G[i] @ u[i + 1]
    return np.concatenate(u)


def main(order):
    k = SC.khalf(order)
    c = {n: np.array(v, dtype=float) for n, v in gen_consts.consts(k).items() if n != "k"}
    rec = os.path.join(ROOT, "profiles", "solve_accuracy.jsonl")
    kern = {}
    if os.path.exists(rec):
        for r in map(json.loads, open(rec)):
            if r["order"] == order and r["family"] in ("twin", "reg"):
                kern[(r["M"], r["grid"], r["family"])] = r["norm_rel"]
    print("# Order %d: which stage of the reduced solve loses the digits\n" % order)
    print("Built by `tools/solve_loss_stages.py %d` (CPU; columns explained in its docstring).  `twin` / `reg`: the "
          "kernels' norm_rel on the same (order, M, grid) from `profiles/solve_accuracy.jsonl`, all nine drones.\n" % order)
    print("| M | grid | cond(R) | entries | solve: block | solve: dense | solve: 60 dig | recovery | twin | reg |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for M, grid in [(10, "even"), (10, "uneven"), (20, "even")] + [(M, "uneven") for M in range(13, 21)]:
        wp, t = SC.inputs(order, M, grid)
        keep = [d for d in range(wp.shape[0]) if d != SC.RAISED]
        exact = SX.exact_batch_k1(wp[keep], t[keep], k)
        w = {n: 0.0 for n in ("cond", "entries", "block", "dense", "mp", "recovery")}
        for j, d in enumerate(keep):
            R, rhs, T = reduced_system(wp[d], t[d], k, c)
            u_exact = np.concatenate([np.array([exact[j][i, :, n] * factorial(n) for n in range(1, k)])
                                      for i in range(1, M)])
            Rm = mp.matrix(R.tolist())
            cols = [mp.lu_solve(Rm, mp.matrix(rhs[:, a].tolist())) for a in range(4)]
            u_mp = np.array([[float(cols[a][r]) for a in range(4)] for r in range(R.shape[0])])
            for name, v in (("cond", np.linalg.cond(R)),
                            ("entries", np.abs(u_mp - u_exact).max() / np.abs(u_exact).max()),
                            ("block", norm_rel(recover(block_sweep(R, rhs, k - 1), wp[d], T, k, c), exact[j])),
                            ("dense", norm_rel(recover(np.linalg.solve(R, rhs), wp[d], T, k, c), exact[j])),
                            ("mp", norm_rel(recover(u_mp, wp[d], T, k, c), exact[j])),
                            ("recovery", norm_rel(recover(u_exact, wp[d], T, k, c), exact[j]))):
                w[name] = max(w[name], float(v))
        print("| %d | %s | %.1e | %.1e | %.1e | %.1e | %.1e | %.1e | %s | %s |" % (
            M, grid, w["cond"], w["entries"], w["block"], w["dense"], w["mp"], w["recovery"],
            *("%.1e" % kern[(M, grid, f)] if (M, grid, f) in kern else "" for f in ("twin", "reg"))))
        sys.stdout.flush()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 9)
