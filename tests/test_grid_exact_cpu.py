"""The exact references of the shared-grid GEMM tests (tests/grid_exact.py) checked without a GPU: the instance rule
enumerates exactly the instances the library builds, the GPU tests' parameter lists reach every one of them, a NumPy
emulation of the product meets the same exactness and bound, and the column-slicing shapes are in their regimes."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_exact as gx  # noqa: E402
import test_grid_exact_gpu as G  # noqa: E402


def _gemm_names():
    reg = {f"msnap::grid_gemm_kernel<8, {M}>" for M in range(1, 16)} | \
          {f"msnap::grid_gemm_kernel<10, {M}>" for M in range(1, 13)}
    stream = {f"msnap::grid_gemm_stream_kernel<8, {nks}, {rt}>" for nks in range(5, 17) for rt in (1, 4)} | \
             {f"msnap::grid_gemm_stream_kernel<10, {nks}, {rt}>" for nks in range(4, 17) for rt in (1, 4)}
    return reg, stream


K1_NAMES = {"msnap::solve_kernel<4, true>", "msnap::solve_kernel<5, true>"}     # 64 and 65 segments: global scratch


@pytest.mark.parametrize("n_cu", [64, 256, 304])
def test_instance_rule_enumerates_the_77_gemm_instances_and_the_gpu_lists_reach_them_all(n_cu):
    reg, stream = _gemm_names()
    assert len(reg) == 27 and len(stream) == 50
    # grid_gemm_stream_kernel<8, 4, RT> is instantiated (launch_stream_nc's switch starts at 4 for both orders) but
    # unreachable: at order 7 every segment count of at most 4 k steps (M <= 15) has at most 8 column tiles and takes
    # the register kernel.  It is therefore in neither set.
    assert not any(n.startswith("msnap::grid_gemm_stream_kernel<8, 4,") for n in stream)
    names = {gx.expected_instance(order, M, N, n_cu)
             for order in (7, 9) for M in range(1, 66) for N in (9, G.rt4_drones(n_cu))}
    assert {n for n in names if "grid_gemm" in n} == reg | stream
    assert {n for n in names if "grid_gemm" not in n} == K1_NAMES
    for order in (7, 9):
        for M in range(1, 66):
            assert (gx.family(gx.expected_instance(order, M, 9, n_cu)) == "k1") == (M > 63)

    # no instance is left out by the GPU tests' one-hot lists
    visited = set()
    for order, M in G.ONE_HOT_CASES:
        for N in G.SMALL_N + ((G.BIG_N,) if M in G.BIG_N_M[order] else ()):
            visited.add(gx.expected_instance(order, M, N, n_cu))
    assert not any(gx.family(n) == "stream4" for n in visited)          # (all of these are small batches)
    for order, nks, M in G.RT4_CASES:
        assert gx.ceil_div(M + 1, 4) == nks and (M + 1) % 4 != 0
        visited.add(gx.expected_instance(order, M, G.rt4_drones(n_cu), n_cu))
    assert visited == names
    assert G.rt4_drones(n_cu) % 4 != 0 and G.rt4_drones(n_cu) % 16 != 0

    for order in (7, 9):
        # BIG_N: at least four segment counts per family; RT = 4: whole and partial last column tiles
        fams = [gx.family(gx.expected_instance(order, M, G.BIG_N, n_cu)) for M in G.BIG_N_M[order]]
        assert fams.count("reg") >= 4 and fams.count("stream1") >= 4 and fams.count("k1") >= 1
        rem = {(M * (order + 1)) % 16 == 0 for o, _, M in G.RT4_CASES if o == order}
        assert rem == {True, False}
        dense = {gx.family(gx.expected_instance(o, M, G.rt4_drones(n_cu) if rt4 else G.DENSE_N, n_cu))
                 for o, M, rt4 in G.DENSE_CASES if o == order}
        assert dense == {"reg", "stream1", "stream4"}
        assert {o_M for o_M in G.FUSED_CASES if o_M[0] == order} == {(order, M) for M in range(1, 12)}
        for fam, M in G.STATUS_CASES + G.ARENA_CASES:
            N = G.rt4_drones(n_cu) if fam == "stream4" else 10
            assert gx.family(gx.expected_instance(order, M, N, n_cu)) == fam


def test_k1_long_path_name_switches_to_global_scratch_with_the_lds_limit():
    """The formula behind the two K1 names, at segment counts on either side of the 160 KiB limit."""
    assert gx.k1_long_path_name(7, 25) == "msnap::solve_kernel<4, false>"
    assert gx.k1_long_path_name(9, 25) == "msnap::solve_kernel<5, false>"
    assert gx.k1_long_path_name(7, 64) == "msnap::solve_kernel<4, true>"
    assert gx.k1_long_path_name(9, 65) == "msnap::solve_kernel<5, true>"


def test_unit_waypoints_and_one_hot_rows():
    for m in (1, 2, 5, 16, 17, 66):
        wp = gx.unit_waypoints(m)
        assert wp.shape == (gx.ceil_div(m, 4), m, 4) and wp.sum() == m
        for j in range(m):
            assert wp[j >> 2, j, j & 3] == 1.0
    for N, m in ((1, 2), (3, 5), (9, 16), (5, 66), (17, 66), (523, 64)):
        wp, j, s = gx.one_hot_rows(N, m, N + m)
        assert (np.count_nonzero(wp, axis=1) == 1).all()
        d, a = np.meshgrid(np.arange(N), np.arange(4), indexing="ij")
        np.testing.assert_array_equal(wp[d, j, a], s)
        e = np.log2(np.abs(s))
        assert (e == np.round(e)).all() and e.min() >= -8 and e.max() <= 8
        assert (j == m - 1).any()
        if 4 * N >= m:
            assert set(j.reshape(-1).tolist()) == set(range(m))
        for rt in range(gx.ceil_div(N, 4)):
            tile = j[4 * rt:4 * rt + 4].reshape(-1)
            assert len(set(tile.tolist())) == min(len(tile), m)


def _oracle_operator(order, M, t):
    import msnap_oracle as oracle
    coef, _ = oracle.solve_batch_fast(gx.unit_waypoints(M + 1), t, ncoef=order + 1)
    return gx.operator_from_coef(coef)


@pytest.mark.parametrize("order,M", [(7, 1), (7, 6), (9, 12), (7, 20), (9, 33), (7, 63), (9, 63)])
def test_numpy_emulation_of_the_product(order, M):
    """einsum over the oracle's operator: one-hot rows give s * G[j] exactly, dense rows stay within the bound the
    GPU test applies to the kernels."""
    m = M + 1
    for grid in G.GRIDS.values():
        t = grid(m)
        Gop = _oracle_operator(order, M, t)
        assert Gop.shape == (m, M, order + 1) and np.isfinite(Gop).all()
        # the operator reproduces the waypoints: c0 of segment i is waypoint i
        np.testing.assert_allclose(Gop[:M, :, 0], np.eye(M), atol=1e-6)
        N = 19
        wp, j, s = gx.one_hot_rows(N, m, 3 * M)
        got = np.einsum("dja,jsk->dsak", wp, Gop)
        np.testing.assert_array_equal(got, (Gop[j] * s[:, :, None, None]).transpose(0, 2, 1, 3))
        wp = np.random.default_rng(M).uniform(-5.0, 5.0, size=(N, m, 4))
        got = np.einsum("dja,jsk->dsak", wp, Gop)
        rows = [(d, i % 4) for i, d in enumerate((0, 1, 2, 3, 9, N - 3, N - 2, N - 1))]
        W = np.stack([wp[d, :, a] for d, a in rows])
        ratios = gx.bound_ratios(np.stack([got[d, :, a, :] for d, a in rows]), W, Gop)
        assert ratios.max() <= m + 4, ratios.max()


def test_exact_product_is_exact():
    W = np.array([[1.0, 2.0 ** -60, -1.0], [3.0, 0.0, 0.1]])
    Gm = np.array([[1.0, 0.5], [1.0, 2.0 ** 40], [1.0, 0.25]])
    sums, mags = gx.exact_product(W, Gm)
    assert sums[0] == [Fraction(1, 2 ** 60), Fraction(1, 4) + Fraction(1, 2 ** 20)]
    assert mags[0] == [2 + Fraction(1, 2 ** 60), Fraction(3, 4) + Fraction(1, 2 ** 20)]
    assert sums[1] == [3 + Fraction(0.1), Fraction(3, 2) + Fraction(0.1) / 4]
    # fp64 loses the small term of row 0, column 0 entirely: ratio = |0 - 2^-60| / (2^-53 * (2 + 2^-60)) ~ 2^-8
    r = gx.bound_ratios(np.array([[0.0, 0.25 + 2.0 ** -20], [3.1, 1.525]]), W, Gm)
    assert abs(r[0, 0] - 2.0 ** -8) < 1e-9 and r[0, 1] == 0.0 and r[1].max() <= 2.0


def test_slicing_regimes_of_the_chosen_shapes():
    # the worked example of the launch rule: 256 CUs, order 7, 20 segments, 400 drones -> slices of 4, 4 and 2 tiles
    assert gx.slicing(7, 20, 400, 256, 1) == (3, 4)
    assert gx.slicing_regime(7, 20, 400, 256, 1) == "c"
    # the shapes the GPU tests pick on 256 CUs, frozen: a change of the launch rule moves them
    assert gx.slicing_shapes(7, 256) == {"a": (20, 5), "b": (20, 113), "c": (20, 253)}
    assert gx.slicing_shapes(9, 256) == {"a": (16, 5), "b": (16, 113), "c": (16, 253)}     # ten column tiles too
    for order in (7, 9):
        assert gx.ceil_div(G.SLICE_M[order] * (order + 1), 16) == 10
        assert [gx.slicing(order, G.SLICE_M[order], N, 256, 1) for N in (5, 113, 253)] == [(10, 1), (5, 2), (4, 3)]
        # default target of 16 waves per CU: small batches are sliced down to single column tiles
        assert gx.slicing(order, G.SLICE_M[order], 253, 256, 0) == (10, 1)
        assert gx.slicing(order, G.SLICE_M[order], 253, 256, 4) == (10, 1)
        for n_cu in (64, 104, 256, 304):
            shapes = gx.slicing_shapes(order, n_cu)
            assert set(shapes) == {"a", "b", "c"}
            for regime, (M, N) in shapes.items():
                assert M == G.SLICE_M[order] and N % 4 != 0 and N < 64 * n_cu
                slices, cts = gx.slicing(order, M, N, n_cu, 1)
                nct = gx.ceil_div(M * (order + 1), 16)
                assert slices > 1 and (slices - 1) * cts < nct <= slices * cts
                assert (cts == 1, cts > 1 and nct % cts == 0, cts > 1 and nct % cts != 0) == \
                       (regime == "a", regime == "b", regime == "c")
    # RT = 4 batches are not sliced
    assert gx.slicing(7, 20, 64 * 256, 256, 1) == (1, 10)
