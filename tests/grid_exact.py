"""Exact references for the shared-grid GEMM (msnap_solve_grid, csrc/msnap_grid.hip), test side only.

The operator of a prepared grid is the K1 solve of the unit waypoint vectors (unit_waypoints), so a test can obtain the
very same numbers from solve_batch on those waypoints (operator_from_coef) and compare the product
C[(d, a)][(seg, k)] = sum_j W[(d, a)][j] G[j][seg][k] with it: bit for bit when every row of W is one signed power of
two (one_hot_rows: the other terms of the fused sum are 0 * g = 0), and against the exact rational sum (exact_product)
for dense rows.  expected_instance and slicing restate the launch rules of msnap_grid.hip (and, above 63 segments, of
msnap_solve.hip) as they stand; they are deliberately not imported from the library."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)          # unit roundoff of fp64

# msnap_grid.hip
GRID_MAX_CT, GRID_MAX_KS, STREAM_MAX_KS = 8, 4, 16
# msnap_solve.hip / msnap_internal.h / msnap_sweep.h: what the K1 solve's long-path name depends on
MAX_LDS_BYTES, TR_PITCH = 160 * 1024, 68


def ceil_div(a, b):
    return -(-a // b)


def uniform_grid(m):
    """The reference's grid for m poses: t_i = i * (10 / m) (oracle.path_times)."""
    step = 10.0 / m
    return np.array([step * i for i in range(m)])


def ratio_grid(m):
    """Non-uniform grid: durations alternate 0.25, 0.75 (1:3; every time is a multiple of 1/4: differences exact)."""
    return np.concatenate([[0.0], np.cumsum(np.where(np.arange(m - 1) % 2 == 0, 0.25, 0.75))])


def unit_waypoints(m):
    """[P, m, 4] with wp'[p][i][a] = 1 iff i == 4p + a: the m unit waypoint vectors, 4 per pseudo-drone."""
    P = ceil_div(m, 4)
    wp = np.zeros((P, m, 4))
    for j in range(m):
        wp[j >> 2, j, j & 3] = 1.0
    return wp


def operator_from_coef(coef):
    """K1 result [P, M, 4, nc] on unit_waypoints(M + 1) -> G [M + 1, M, nc], G[j] = coef[j >> 2, :, j & 3, :]."""
    coef = np.asarray(coef)
    P, M, _, nc = coef.shape
    return np.ascontiguousarray(coef.transpose(0, 2, 1, 3).reshape(4 * P, M, nc)[:M + 1])


def k1_long_path_name(order, M):
    """last_kernel() of the K1 solve beyond every unrolled instance (more than 24 segments): the rolled kernel, on
    a global scratch slab once its tile no longer fits the LDS."""
    K = (order + 1) // 2
    nu = K - 1
    words = 16 * M + 16 * nu * nu * (M - 1) + 64 * nu * (M - 1)
    lds = K * TR_PITCH * 16 + (words + 16 * (M + 1) * 5) * 8
    return "msnap::solve_kernel<%d, %s>" % (K, "false" if lds <= MAX_LDS_BYTES else "true")


def expected_instance(order, M, N, n_cu):
    nc = order + 1
    nct, nks = ceil_div(M * nc, 16), ceil_div(M + 1, 4)
    if nct <= GRID_MAX_CT and nks <= GRID_MAX_KS:
        return "msnap::grid_gemm_kernel<%d, %d>" % (nc, M)
    if nks <= STREAM_MAX_KS:
        return "msnap::grid_gemm_stream_kernel<%d, %d, %d>" % (nc, nks, 4 if N >= 64 * n_cu else 1)
    assert M > 24
    return k1_long_path_name(order, M)


def family(name):
    """'reg' | 'stream1' | 'stream4' | 'k1' of an expected_instance name."""
    if "grid_gemm_kernel" in name:
        return "reg"
    if "grid_gemm_stream_kernel" in name:
        return "stream4" if name.endswith(", 4>") else "stream1"
    return "k1"


def slicing(order, M, N, n_cu, waves_per_cu):
    """(slices, cts) of launch_stream_nks: blockIdx.y extent and column tiles per slice."""
    nct = ceil_div(M * (order + 1), 16)
    if N >= 64 * n_cu:
        return 1, nct
    target = n_cu * (waves_per_cu if waves_per_cu > 0 else 16)
    nrg = ceil_div(N, 4)
    slices = max(1, min(ceil_div(target, nrg), nct))
    cts = ceil_div(nct, slices)
    return ceil_div(nct, cts), cts


def slicing_regime(order, M, N, n_cu, waves_per_cu):
    """'a': one column tile per slice; 'b': cts > 1 dividing nct; 'c': cts > 1 with a shorter last slice."""
    nct = ceil_div(M * (order + 1), 16)
    _, cts = slicing(order, M, N, n_cu, waves_per_cu)
    return "a" if cts == 1 else "b" if nct % cts == 0 else "c"


def slicing_shapes(order, n_cu, waves_per_cu=1):
    """{regime: (M, N)} for the streaming RT = 1 kernel on a device of n_cu CUs: ten column tiles (20 segments at
    order 7, 16 at order 9) and the smallest N with a partial last row tile in each regime."""
    M, out = {7: 20, 9: 16}[order], {}
    for N in range(5, 64 * n_cu):
        if N % 4 == 0:
            continue
        r = slicing_regime(order, M, N, n_cu, waves_per_cu)
        if r not in out and slicing(order, M, N, n_cu, waves_per_cu)[0] > 1:
            out[r] = (M, N)
        if len(out) == 3:
            break
    return out


def one_hot_rows(N, m, seed):
    """wp [N, m, 4] with one non-zero waypoint s[d, a] = +-2^e, e in [-8, 8], at index j[d, a] per (drone, axis) row.
    Row r = 4d + a takes j = perm[r % m] of a seeded permutation with perm[0] = m - 1: the last waypoint always occurs,
    every waypoint occurs once 4N >= m, and the 16 rows of a 4-drone row tile carry different j (all of them when
    m < 16).  Returns (wp, j, s)."""
    rng = np.random.default_rng(seed)
    perm = np.concatenate([[m - 1], rng.permutation(m - 1)]).astype(np.int64)
    j = perm[np.arange(4 * N) % m].reshape(N, 4)
    s = np.ldexp(rng.choice([-1.0, 1.0], size=(N, 4)), rng.integers(-8, 9, size=(N, 4)))
    wp = np.zeros((N, m, 4))
    d, a = np.meshgrid(np.arange(N), np.arange(4), indexing="ij")
    wp[d, j, a] = s
    return wp, j, s


def _common_ints(x):
    """Floats -> (ints, e) with x == ints / 2^e exactly."""
    fr = [Fraction(float(v)) for v in x]
    den = max(f.denominator for f in fr)            # (powers of two: the largest is the common one)
    return [f.numerator * (den // f.denominator) for f in fr], den


def exact_product(W_rows, G):
    """W_rows [R, m], G [m, ...] (floats) -> (sum_j W_j G_j, sum_j |W_j| |G_j|), each a list of R lists of Fractions
    over the flattened trailing axes of G.  Exact: every float is a dyadic rational, the sums are formed in integers
    over the common denominator and returned as fractions.Fraction."""
    W_rows = np.asarray(W_rows, dtype=np.float64)
    G2 = np.asarray(G, dtype=np.float64).reshape(np.shape(G)[0], -1)
    m, C = G2.shape
    gi, gden = _common_ints(G2.reshape(-1))
    gcols = [[gi[j * C + c] for j in range(m)] for c in range(C)]
    gabs = [[abs(v) for v in col] for col in gcols]
    sums, mags = [], []
    for row in W_rows:
        wi, wden = _common_ints(row)
        wa = [abs(v) for v in wi]
        den = gden * wden
        sums.append([Fraction(sum(w * g for w, g in zip(wi, col)), den) for col in gcols])
        mags.append([Fraction(sum(w * g for w, g in zip(wa, col)), den) for col in gabs])
    return sums, mags


def bound_ratios(got_rows, W_rows, G):
    """|got - exact| / (2^-53 sum |W||G|) per entry as floats [R, C] (0 where the magnitude sum is 0 and got is too;
    inf where only the magnitude sum is)."""
    sums, mags = exact_product(W_rows, G)
    got_rows = np.asarray(got_rows, dtype=np.float64).reshape(len(sums), -1)
    out = np.zeros(got_rows.shape)
    for r, (srow, mrow) in enumerate(zip(sums, mags)):
        for c, (sv, mv) in enumerate(zip(srow, mrow)):
            err = abs(Fraction(float(got_rows[r, c])) - sv)
            out[r, c] = float(err / (U * mv)) if mv else (0.0 if err == 0 else np.inf)
    return out
