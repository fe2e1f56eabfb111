"""Kernels either side of the solve, through the C-ABI, against the oracle:
pack (a7), formation transform (a8), sampler (a5), the two collision passes,
and the node-level functions that chain them."""
import math
import os

import numpy as np
import pytest

import msnap_oracle as O
from conftest import GOLDEN_DIR, norm_rel

pytestmark = pytest.mark.gpu


def test_pack_pol_matrix_bit_exact(ctx7, golden):
    coef, dur = golden["cfg2_coef"][:20], golden["cfg2_dur"][:20]
    got = ctx7.pack_pol_matrix(coef, dur)
    assert got.dtype == np.float32 and got.shape == (20, 10, 33)
    for d in range(20):
        np.testing.assert_array_equal(got[d], O.pack_pol_matrix(coef[d], dur[d]))


def test_pack_order9(ctx9):
    rng = np.random.default_rng(1)
    coef = rng.normal(size=(5, 4, 4, 10))
    dur = rng.uniform(0.5, 2, size=(5, 4))
    got = ctx9.pack_pol_matrix(coef, dur)
    assert got.shape == (5, 4, 41)
    for d in range(5):
        np.testing.assert_array_equal(got[d], O.pack_pol_matrix(coef[d], dur[d]))


def test_formation_transform(ctx7):
    rng = np.random.default_rng(2)
    P = 50
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[0] = [0, 0, 0, 1]
    q[1] = [1, 0, 0, 0]          # trace = -1: the non-default GetQuaternion branches
    q[2] = [0, 1, 0, 0]
    q[3] = [0, 0, 1, 0]
    rb = np.concatenate([rng.uniform(-5, 5, size=(P, 3)), q], axis=1)
    off = np.array([[0.5, 0, 0], [-0.5, 0, 0], [0.1, -0.7, 0.3]])
    got = ctx7.formation_transform(rb, off)
    ref = O.formation_transform(rb, off)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-14)
    # the two reference drones sit 1 m apart on the body x axis (drones_traj_generator.py:22-25)
    np.testing.assert_allclose(np.linalg.norm(got[0, :, :3] - got[1, :, :3], axis=1), 1.0, atol=1e-12)


def test_sampler_bit_exact_incl_knots_and_past_end(ctx7, golden):
    coef, dur = golden["cfg2_coef"][:12], golden["cfg2_dur"][:12]
    total = dur.sum(axis=1).max()
    S = int(total / 0.1) + 15                       # runs past every drone's end: extrapolation
    got = ctx7.sample(coef, dur, 0.1, S, 4)
    ref = O.sample_positions(coef, dur, 0.1, S, naxes=4)
    np.testing.assert_array_equal(got, ref)
    # samples exactly on knots: uniform 0.2 s pieces sampled every 0.1 s
    mat = np.loadtxt(os.path.join(GOLDEN_DIR, "Pol_matrix_1.csv"), delimiter=",")
    c = mat[:, 1:].reshape(1, 49, 4, 8).astype(np.float64)
    d = mat[:, 0].reshape(1, 49).astype(np.float64)
    got = ctx7.sample(c, d, 0.1, 105, 3)
    ref = O.sample_positions(c, d, 0.1, 105, naxes=3)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("n,m,s_extra,dt,naxes", [(1, 1, 3, 0.1, 3), (7, 3, 5, 0.07, 4), (33, 10, 0, 0.1, 3), (300, 10, 9, 0.1, 3),
                                                  (19, 20, 2, 0.25, 3), (5, 49, 0, 0.1, 4), (3, 120, 4, 0.05, 3),
                                                  (9, 6, 0, 0.0, 3), (4, 10, 3000, 0.01, 3), (64, 8, 1, 1.0 / 3.0, 3)])
def test_sampler_ranges_bit_exact(ctx7, n, m, s_extra, dt, naxes):
    """The (drone, piece, axis) sampler against the reference's search loop (C and NumPy oracles), bit for
    bit: piece boundaries on and off the sample grid, zero-length pieces, drones with negative or NaN
    durations (the generic search), dt = 0, paths longer than the LDS image (the generic kernel)."""
    import c_oracle
    rng = np.random.default_rng(100 * n + m)
    coef = rng.normal(size=(n, m, 4, 8))
    dur = rng.uniform(0.3, 1.7, size=(n, m))
    dur[0, :] = np.round(dur[0, :] * 10.0) / 10.0             # knots on multiples of 0.1
    if n > 2 and m > 2:
        dur[1, 1] = 0.0                                        # a piece that owns no sample
        dur[2, m // 2] = -0.4                                  # not a partition: the generic search
    if n > 4:
        dur[4, 0] = np.nan
    total = float(np.nanmax(np.nansum(np.abs(dur), axis=1)))
    S = (int(total / dt) if dt > 0 else 7) + 1 + s_extra
    got = ctx7.sample(coef, dur, dt, S, naxes)
    ref = c_oracle.sample_positions(coef, dur, dt, S, naxes)
    np.testing.assert_array_equal(got, ref)
    good = [d for d in range(n) if (dur[d] >= 0).all()][:3]    # the reference asserts on a negative local time
    np.testing.assert_array_equal(got[good, :40], O.sample_positions(coef[good], dur[good], dt, min(S, 40), naxes=naxes))


def test_sampler_output_sweeps_odd_bases_and_grid_stride_rounds(ctx7):
    """The two output forms the shapes above do not reach, bit for bit against the C oracle.  28 pieces x 3 axes put 3
    drones into a workgroup and 41 samples make a drone's block 123 doubles: the second workgroup's block starts at an
    odd word and leaves by the 8-byte sweep (369 words: two rounds of 256 threads, the second partial), the first by the
    16-byte one (184 pairs and the odd tail); 7 drones leave the last workgroup one.  4000 samples do not fit the LDS
    image: 300 x 4000 (drone, sample) items are more than the generic kernel's grid of (CUs x 16) x 256 threads, a
    second, partial grid-stride round."""
    import c_oracle
    rng = np.random.default_rng(41)
    coef = rng.normal(size=(7, 28, 4, 8))
    dur = rng.uniform(0.02, 0.05, size=(7, 28))
    np.testing.assert_array_equal(ctx7.sample(coef, dur, 0.025, 41, 3), c_oracle.sample_positions(coef, dur, 0.025, 41, 3))
    coef = rng.normal(size=(300, 2, 4, 8))
    dur = rng.uniform(0.3, 1.7, size=(300, 2))
    np.testing.assert_array_equal(ctx7.sample(coef, dur, 0.001, 4000, 3), c_oracle.sample_positions(coef, dur, 0.001, 4000, 3))


def test_sampler_order9_and_solved_swarm(ctx9):
    import c_oracle
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(21, 50, 10)
    coef, dur, status = ctx9.solve_batch(wp, t)
    assert (status == 0).all()
    S = int(dur.sum(axis=1).max() / 0.1) + 4
    np.testing.assert_array_equal(ctx9.sample(coef, dur, 0.1, S, 3), c_oracle.sample_positions(coef, dur, 0.1, S, 3))


def test_formation_collide_against_oracle(ctx7):
    rng = np.random.default_rng(4)
    for n, S in [(1, 5), (2, 3), (37, 21), (300, 9)]:
        pos = rng.uniform(-2, 2, size=(n, S, 3))
        md, partner, hit = ctx7.formation_collide(pos, pos, 0.15)
        rmd, rpartner, rhit = O.formation_collide(pos, 0.15)
        np.testing.assert_allclose(md, rmd, rtol=0, atol=1e-9)
        np.testing.assert_array_equal(partner, rpartner)
        np.testing.assert_array_equal(hit, rhit)
    # sharded rows against all columns == unsharded
    pos = rng.uniform(-1, 1, size=(101, 12, 3))
    rad = 0.5 * float(np.median(O.formation_collide(pos, 0.0)[0]))
    rmd, rpartner, rhit = O.formation_collide(pos, rad)
    assert rhit.any() and not rhit.all()
    for lo, hi in [(0, 40), (40, 101)]:
        md, partner, hit = ctx7.formation_collide(pos[lo:hi], pos, rad, row_offset=lo)
        np.testing.assert_allclose(md, rmd[lo:hi], rtol=0, atol=1e-9)
        np.testing.assert_array_equal(partner, rpartner[lo:hi])
        np.testing.assert_array_equal(hit, rhit[lo:hi])


@pytest.mark.parametrize("n,s,ro,r", [(70, 5, 0, 70), (200, 9, 0, 200), (333, 23, 0, 333), (333, 23, 100, 97),
                                      (333, 23, 0, 64), (333, 23, 269, 64), (500, 4, 130, 370), (97, 3, 0, 97),
                                      (1000, 13, 0, 1000), (1000, 13, 640, 200), (129, 40, 0, 129),
                                      (128, 7, 0, 128), (257, 12, 0, 257), (260, 6, 128, 130), (135, 19, 3, 129),
                                      (200, 8, 0, 200), (140, 14, 5, 130), (150, 20, 0, 150),
                                      (100, 91, 0, 100), (300, 96, 37, 200), (260, 49, 0, 260)])
def test_formation_collide_tiles(ctx7, n, s, ro, r):
    """The span kernel: pairs inside the rows' own column range are evaluated once and credited to
    both drones (column-side minima through the per-wave LDS fold), everything else one-sidedly.
    Row counts around the 128-row (two rows per lane) / 8-column block edges, shards at unaligned
    offsets, sample counts around the 6-sample chunk, paths long enough for a small launch to split its
    shares over 2 - 8 sample parts, with exact ties between equidistant neighbours
    (lattice positions): distances, partners (lowest index wins) and hits must equal the oracle's bit
    for bit."""
    rng = np.random.default_rng(1000 * n + s)
    pos = rng.uniform(-3.0, 3.0, size=(n, s, 3))
    # a lattice part: many exactly equal distances, so partner choice is decided by the index rule
    k = n // 3
    pos[:k] = np.round(pos[:k] * 2.0) / 2.0
    pos[5] = pos[4] + np.array([0.25, 0.0, 0.0])           # a close pair across the whole path
    rmd, rpartner, rhit = O.formation_collide(pos, 0.3)
    md, partner, hit = ctx7.formation_collide(pos[ro:ro + r], pos, 0.3, row_offset=ro)
    np.testing.assert_array_equal(md, rmd[ro:ro + r])
    np.testing.assert_array_equal(partner, rpartner[ro:ro + r])
    np.testing.assert_array_equal(hit, rhit[ro:ro + r])


@pytest.mark.parametrize("parts", [2, 4, 8])
def test_formation_collide_sample_parts(ctx7, parts):
    """Every share taken by several waves with a range of the sample chunks each (what a small launch
    does by itself), forced on a swarm big enough to have two-sided blocks and several row blocks:
    row-side and column-side partial minima of the parts must merge to the oracle's answer."""
    rng = np.random.default_rng(900 + parts)
    pos = rng.uniform(-3.0, 3.0, size=(700, 55, 3))
    pos[:200] = np.round(pos[:200] * 2.0) / 2.0
    ref = O.formation_collide(pos, 0.3)
    ctx7.set_option("collide_sample_parts", parts)
    try:
        got = ctx7.formation_collide(pos, pos, 0.3)
        shard = ctx7.formation_collide(pos[300:650], pos, 0.3, row_offset=300)
    finally:
        ctx7.set_option("collide_sample_parts", 0)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(shard, ref):
        np.testing.assert_array_equal(a, b[300:650])


def test_formation_collide_seeded_shapes(ctx7):
    """Thirty seeded shapes (swarm size, sample count, shard position and length drawn at random; a lattice
    part for exact ties) against the C oracle, bit for bit: the shape-dependent paths of the launch -- block
    instances of 2 / 4 / 8 columns, plain remainder samples or an overlapped last chunk, sample parts of
    small launches, shards that start and end inside row blocks -- in combinations nobody listed by hand."""
    import c_oracle
    rng = np.random.default_rng(20260104)
    for _ in range(30):
        n = int(rng.integers(2, 900))
        s = int(rng.integers(1, 70))
        pos = rng.uniform(-4.0, 4.0, size=(n, s, 3))
        k = n // 4
        pos[:k] = np.round(pos[:k] * 2.0) / 2.0
        ref = c_oracle.formation_collide(pos, 0.25)
        ro = int(rng.integers(0, n))
        r = int(rng.integers(1, n - ro + 1))
        for lo, cnt in ((0, n), (ro, r)):
            got = ctx7.formation_collide(pos[lo:lo + cnt], pos, 0.25, row_offset=lo)
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b[lo:lo + cnt], err_msg=f"n={n} s={s} rows=[{lo},{lo + cnt})")


def test_formation_collide_rows_not_among_columns(ctx7):
    """rows beyond the columns (row_offset + n_rows > n_cols): one-sided everywhere, no self to exclude."""
    rng = np.random.default_rng(77)
    pos = rng.uniform(-2.0, 2.0, size=(150, 11, 3))
    md, partner, hit = ctx7.formation_collide(pos[100:150], pos[:120], 0.3, row_offset=100)
    ref = O.formation_collide(pos[:120], 0.3)
    np.testing.assert_array_equal(md[:20], ref[0][100:120])     # rows 100..119 are columns too
    np.testing.assert_array_equal(partner[:20], ref[1][100:120])
    for q in range(20, 50):                                    # rows 120..149 meet every column
        d = pos[:120] - pos[100 + q][None]
        d2 = O.fma_square(d[..., 2], O.fma_square(d[..., 1], d[..., 0] * d[..., 0])).min(axis=1)
        assert md[q] == np.sqrt(d2.min()) and partner[q] == int(np.argmin(d2))


@pytest.mark.parametrize("n,s", [(1, 8), (2, 6), (3, 5), (65, 6), (64, 7), (129, 1)])
def test_formation_collide_small_edges(ctx7, n, s):
    """One drone (nobody to meet: +inf / -1 / no hit), exactly one sample chunk, fewer samples than a chunk
    (the plain-loop kernel), one row more than a row block."""
    import c_oracle
    rng = np.random.default_rng(n * 31 + s)
    pos = rng.uniform(-1.0, 1.0, size=(n, s, 3))
    md, partner, hit = ctx7.formation_collide(pos, pos, 0.2)
    rmd, rpartner, rhit = c_oracle.formation_collide(pos, 0.2)
    np.testing.assert_array_equal(md, rmd)
    np.testing.assert_array_equal(partner, rpartner)
    np.testing.assert_array_equal(hit, rhit)
    if n == 1:
        assert np.isinf(md[0]) and partner[0] == -1 and not hit[0]


@pytest.mark.parametrize("n,s,t", [(3, 10, 0), (5, 1, 1), (7, 64, 65), (4, 200, 130), (2, 2100, 12)])
def test_mesh_sweep_edges(ctx7, n, s, t):
    """No triangles (+inf, no hit), a single sample, more triangles than one lane group (65, 130), more samples
    than one workgroup pass (2100): the exact cull must not change any distance."""
    import c_oracle
    rng = np.random.default_rng(n * 17 + s + t)
    pos = rng.uniform(-3.0, 3.0, size=(n, s, 3))
    tris = rng.uniform(-4.0, 4.0, size=(t, 3, 3))
    if t > 3:
        tris[3, 1] = tris[3, 0]                     # a degenerate triangle (two equal vertices)
    md, hit = ctx7.mesh_sweep(pos, tris, 0.4)
    rmd, rhit = c_oracle.mesh_sweep(pos, tris, 0.4)
    np.testing.assert_allclose(md, rmd, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(hit, rhit)
    if t == 0:
        assert np.isinf(md).all() and not hit.any()


@pytest.mark.parametrize("cap", [1, 3, 12])
def test_mesh_sweep_as_a_capped_grid_walks_all_drones(ctx7, cap):
    """ "mesh_waves_per_cu": the sweep as a grid smaller than the swarm whose workgroups walk the drones (what a sweep
    beside another stream's kernels runs as): bit for bit the one-workgroup-per-drone results, incl. a drone count that
    is not a multiple of the grid, two waves per workgroup, NaN paths and the test counter."""
    rng = np.random.default_rng(40 + cap)
    n, s = 2003, 100
    pos = rng.uniform(-3.0, 3.0, size=(n, s, 3))
    pos[17] = np.nan
    pos[1999, 40:] = np.inf
    tris = rng.uniform(-4.0, 4.0, size=(70, 3, 3))
    ref = ctx7.mesh_sweep(pos, tris, 0.4)
    ctx7.set_option("mesh_count_tests", 1)
    ctx7.mesh_sweep(pos, tris, 0.4)
    tests_ref = ctx7.get_option("mesh_count_tests")
    try:
        ctx7.set_option("mesh_waves_per_cu", cap)
        ctx7.set_option("mesh_count_tests", 1)
        got = ctx7.mesh_sweep(pos, tris, 0.4)
        assert ctx7.get_option("mesh_count_tests") == tests_ref > 0
    finally:
        ctx7.set_option("mesh_waves_per_cu", 0)
        ctx7.set_option("mesh_count_tests", 0)
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])
    assert np.isinf(got[0][17]) and not got[1][17]


def test_mesh_sweep_against_oracle(ctx7, tmp_path):
    from drone_path_planning_python_amd import stl
    wall = stl.box_mesh((-2, 3.9, 0), (2, 4.1, 1.6))        # env-scene-ltu-experiment.stl's box
    fn = str(tmp_path / "wall.stl")
    stl.save_stl(fn, wall)
    tris = stl.load_stl(fn)
    rng = np.random.default_rng(5)
    pos = rng.uniform([-3, 2, -0.5], [3, 6, 2.5], size=(40, 17, 3))
    pos[0, 0] = [0.0, 4.0, 0.8]                             # inside the wall
    pos[1, :] = [0.0, 3.0, 1.0]                             # 0.9 m in front of it
    md, hit = ctx7.mesh_sweep(pos, tris, 0.15)
    rmd, rhit = O.mesh_sweep(pos, tris, 0.15)
    np.testing.assert_allclose(md, rmd, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(hit, rhit)
    assert abs(md[1] - 0.9) < 1e-6 and not hit[1]
    assert rhit.any() and not rhit.all()


def test_path_to_pol_node(ctx7, tmp_path):
    """scripts/drones_pols_generator.py path_to_pol: time grid, yaw, solve, float32 pack, CSV, message."""
    from drone_path_planning_python_amd.nodes import drones_pols_generator as dpg
    from drone_path_planning_python_amd.nodes import msgs
    n = 50
    s = np.linspace(0, 1, n)
    pos = np.stack([0.5 + 0.1 * np.sin(6 * s), 3.0 + 2.0 * s, 1.0 + 0.3 * np.sin(3 * s + 0.2)], axis=1)
    yaw = 0.6 * s
    quat = np.stack([np.zeros(n), np.zeros(n), np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
    path = msgs.path_from_arrays(pos, quat)

    class Pub:
        def __init__(self):
            self.sent = []

        def publish(self, m):
            self.sent.append(m)

    dpg.piece_pols_pub = Pub()
    try:
        msg = dpg.path_to_pol(path, 1, ctx=ctx7, out_dir=str(tmp_path))
    finally:
        pub, dpg.piece_pols_pub = dpg.piece_pols_pub, None
    assert pub.sent == [msg] and msg.cf_id == 1
    ref_mat, ref_coef, _ = O.path_to_pol(pos, quat)
    mat = np.loadtxt(os.path.join(tmp_path, "Pol_matrix_1.csv"), delimiter=",")
    assert mat.shape == (49, 33)
    # float32 outputs of an fp64 solve that agrees to ~1e-9: at most an ulp apart
    den = np.abs(ref_mat).max(axis=0)
    assert (np.abs(mat - ref_mat).max(axis=0) / np.where(den == 0, 1, den)).max() < 3e-7
    np.testing.assert_allclose(msg.durations, [np.float32(0.2)] * 49, rtol=1e-6)
    assert len(msg.poly_x) == 49 * 8 and msg.poly_z[0] == np.float32(pos[0, 2])


def test_callbacks_fire_once(ctx7, tmp_path, monkeypatch):
    from drone_path_planning_python_amd.nodes import drones_pols_generator as dpg
    from drone_path_planning_python_amd.nodes import msgs
    calls = []
    monkeypatch.setattr(dpg, "path_to_pol", lambda path, cfid: calls.append(cfid))
    monkeypatch.setattr(dpg.callback1, "counter", 0)
    monkeypatch.setattr(dpg.callback2, "counter", 0)
    p = msgs.path_from_arrays(np.zeros((3, 3)), np.tile([0, 0, 0, 1.0], (3, 1)))
    dpg.callback1(p)
    dpg.callback1(p)
    dpg.callback2(p)
    assert calls == [1, 2]


def test_transform_node(ctx7):
    """scripts/drones_traj_generator.py transform: two drones at +-0.5 m body x."""
    from drone_path_planning_python_amd.nodes import drones_traj_generator as dtg
    from drone_path_planning_python_amd.nodes import msgs
    rng = np.random.default_rng(6)
    P = 20
    yaw = rng.uniform(-3, 3, P)
    quat = np.stack([np.zeros(P), np.zeros(P), np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
    pos = rng.uniform(-3, 3, size=(P, 3))
    path = msgs.path_from_arrays(pos, quat, frame_id="world")
    p1, p2 = dtg.transform(path)
    a1, q1 = msgs.path_to_arrays(p1)
    a2, q2 = msgs.path_to_arrays(p2)
    ref = O.formation_transform(np.concatenate([pos, quat], 1), np.array(dtg.drone_positions, dtype=float))
    np.testing.assert_allclose(a1, ref[0, :, :3], atol=1e-14)
    np.testing.assert_allclose(a2, ref[1, :, :3], atol=1e-14)
    np.testing.assert_allclose(q1, ref[0, :, 3:], atol=1e-14)
    assert p1.header.frame_id == "world" and len(p2.poses) == P
    paths = dtg.transform_formation(path, [[0, 0, 0], [0.3, 0.3, 0.0], [0, 0, -0.4]], ctx=ctx7)
    assert len(paths) == 3
    np.testing.assert_allclose(msgs.path_to_arrays(paths[0])[0], pos, atol=1e-14)


def test_config3_pipeline_formation_swarm(ctx7):
    """configs[2] in miniature: rigid-body paths -> formation transform -> solve ->
    sample -> pairwise pass; hit set fixed by the oracle on the same inputs."""
    from drone_path_planning_python_amd.nodes.drones_pols_generator import yaw_from_quaternion
    from drone_path_planning_python_amd.synthetic import formation_swarm
    offsets = np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.2, 0]])      # third drone 0.54 m from the others
    rb, t = formation_swarm(3, 24, 10, offsets)
    G, m, _ = rb.shape
    out = np.stack([ctx7.formation_transform(rb[g], offsets) for g in range(G)])     # [G,K,m,7]
    poses = out.reshape(G * 3, m, 7)
    wp = np.empty((G * 3, m, 4))
    wp[..., :3] = poses[..., :3]
    wp[..., 3] = [[yaw_from_quaternion(q) for q in row] for row in poses[..., 3:]]
    coef, dur, status = ctx7.solve_batch(wp, t)
    assert (status == 0).all()
    S = len(np.arange(0.0, float(dur[0].sum()), 0.1))
    pos = ctx7.sample(coef, dur, 0.1, S, 3)
    md, partner, hit = ctx7.formation_collide(pos, pos, 0.3)
    rcoef, rdur = O.solve_batch_fast(wp, t)
    assert norm_rel(coef, rcoef) <= 1e-9
    rpos = O.sample_positions(rcoef, rdur, 0.1, S)
    rmd, rpartner, rhit = O.formation_collide(rpos, 0.3)
    np.testing.assert_allclose(md, rmd, atol=1e-7)
    np.testing.assert_array_equal(hit, rhit)
    assert hit.reshape(G, 3)[:, 2].all()          # the close drone always collides (0.54 m < 0.6 m)


def test_flatness_evaluator_against_reference(ctx7, golden):
    """Trajectory.eval on the reference's src/traj.csv: reference outputs (golden flat_*)
    and the oracle's restatement on a dense time grid, incl. piece boundaries."""
    mat = np.loadtxt(os.path.join(GOLDEN_DIR, "traj.csv"), delimiter=",", skiprows=1, usecols=range(33))
    coef = mat[:, 1:].reshape(1, -1, 4, 8)
    dur = mat[:, 0].reshape(1, -1)
    out = ctx7.eval_flat(coef, dur, golden["flat_t"])
    np.testing.assert_allclose(out[0], golden["flat_out"], rtol=1e-12, atol=1e-13)
    knots = np.cumsum(dur[0])
    total = min(float(np.sum(dur[0])), float(knots[-1]))      # the reference asserts t <= np.sum(durations)
    ts = np.unique(np.concatenate([np.arange(0.0, total, 0.05), knots[:-1], [0.0, total]]))
    out = ctx7.eval_flat(coef, dur, ts)
    for s, t in enumerate(ts):
        pos, vel, acc, omega, yaw = O.trajectory_eval(mat, float(t))
        ref = np.concatenate([pos, vel, acc, omega, [yaw]])
        np.testing.assert_allclose(out[0, s], ref, rtol=1e-11, atol=1e-12)
    # outside [0, duration]: NaN (the reference asserts)
    out = ctx7.eval_flat(coef, dur, np.array([-0.1, knots[-1] + 0.5]))
    assert np.isnan(out).all()


def test_get_nav_path_msg(ctx7, golden):
    """trajectory_visualising.get_nav_path_msg (reference visualization.py:39-71) on the reference's
    src/traj.csv and on a Pol_matrix file with the reference's skiprows quirk: poses against the
    oracle's restatement (positions + offset, quaternion_from_euler(0, 0, -yaw))."""
    from drone_path_planning_python_amd.trajectory_visualising import Trajectory, get_nav_path_msg, get_nav_path_msgs
    from drone_path_planning_python_amd.nodes import msgs
    tr = Trajectory()
    tr.loadcsv(os.path.join(GOLDEN_DIR, "traj.csv"))
    mat = np.loadtxt(os.path.join(GOLDEN_DIR, "traj.csv"), delimiter=",", skiprows=1, usecols=range(33))
    offset = [0, 0, -0.5]                                       # scripts/path_vis.py:18-19
    msg = get_nav_path_msg(tr, 0.1, offset, ctx=ctx7)
    ref = O.nav_path_poses(mat, 0.1, offset)
    assert msg.header.frame_id == "world" and len(msg.poses) == ref.shape[0] == len(np.arange(0, tr.duration, 0.1))
    pos, quat = msgs.path_to_arrays(msg)
    np.testing.assert_allclose(pos, ref[:, :3], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(quat, ref[:, 3:], rtol=1e-12, atol=1e-13)
    # the visual node's own inputs: header-less Pol_matrix files read with skiprows=1 (first piece dropped)
    trs, mats = [], []
    for name in ("Pol_matrix_1.csv", "Pol_matrix_2.csv"):
        t2 = Trajectory()
        t2.loadcsv(os.path.join(GOLDEN_DIR, name))
        assert t2.n_pieces() == 48
        trs.append(t2)
        mats.append(np.loadtxt(os.path.join(GOLDEN_DIR, name), delimiter=",", skiprows=1, usecols=range(33)))
    out = get_nav_path_msgs(trs, 0.1, [[0, 0, -0.5], [0.1, 0, -0.5]], ctx=ctx7)
    for m, mat2, off in zip(out, mats, ([0, 0, -0.5], [0.1, 0, -0.5])):
        ref = O.nav_path_poses(mat2.astype(np.float64), 0.1, off)
        pos, quat = msgs.path_to_arrays(m)
        np.testing.assert_allclose(pos, ref[:, :3], rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(quat, ref[:, 3:], rtol=1e-11, atol=1e-11)


def test_flatness_evaluator_batch_on_solved_swarm(ctx7):
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(31, 9, 6)
    coef, dur, status = ctx7.solve_batch(wp, t)
    ts = np.linspace(0.0, float(dur.sum(axis=1).min()), 23)
    out = ctx7.eval_flat(coef, dur, ts)
    for d in range(9):
        matd = O.pack_pol_matrix(coef[d], dur[d]).astype(np.float64)
        matd[:, 0] = dur[d]
        matd[:, 1:] = coef[d].reshape(6, 32)
        for s in (0, 7, 22):
            pos, vel, acc, omega, yaw = O.trajectory_eval(matd, float(ts[s]))
            ref = np.concatenate([pos, vel, acc, omega, [yaw]])
            np.testing.assert_allclose(out[d, s], ref, rtol=1e-10, atol=1e-10)


def test_formation_pass_mesh_on_side_stream(ctx7):
    """formation_pass with a mesh: the sweep runs on the side context's stream beside the pairwise pass and
    must equal the sweep launched in stream order (and the pairwise results must not notice it)."""
    import torch
    from drone_path_planning_python_amd import Context, stl, swarm as sw
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(43, 300, 6)
    wp[..., :3] *= 0.4
    tris = torch.from_numpy(np.ascontiguousarray(stl.box_mesh((-1, -1, -1), (0.5, 0.2, 0.3)))).cuda()
    side = Context(ctx7.device_id, 7, 16)
    try:
        twp, tt = torch.from_numpy(wp).cuda(), torch.from_numpy(t).cuda()
        plain = sw.DeviceCompute(ctx7, torch)
        coef, dur, status = plain.solve(twp, tt)
        S = 45
        ref = sw.formation_pass(plain, coef, dur, 300, 1, 0, 0.1, S, 0.2, torch=torch, mesh_tris=tris)
        both = sw.DeviceCompute(ctx7, torch, side_ctx=side)
        for _ in range(3):      # repeated: the side stream's ordering against the main stream's reuse of buffers
            res = sw.formation_pass(both, coef, dur, 300, 1, 0, 0.1, S, 0.2, torch=torch, mesh_tris=tris)
            torch.cuda.synchronize()
            for a, b in ((res.mesh_min_dist, ref.mesh_min_dist), (res.mesh_hit, ref.mesh_hit), (res.min_dist, ref.min_dist),
                         (res.partner, ref.partner), (res.hit, ref.hit)):
                np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert ref.mesh_hit.any().item() and not ref.mesh_hit.all().item()
        with pytest.raises(RuntimeError):
            both.mesh_end()
    finally:
        torch.cuda.synchronize()
        ctx7.use_own_stream()
        side.close()


def test_device_formation_pass_single_rank(ctx7):
    """swarm.DeviceCompute end to end on device tensors (world = 1: no collective),
    against the host-pointer entry points."""
    import torch
    from drone_path_planning_python_amd import swarm as sw
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(41, 70, 8)
    wp[..., :3] *= 0.3
    comp = sw.DeviceCompute(ctx7, torch)
    try:
        coef, dur, status = comp.solve(torch.from_numpy(wp).cuda(), torch.from_numpy(t).cuda())
        assert int(status.abs().sum().item()) == 0
        S = 40
        res = sw.formation_pass(comp, coef, dur, 70, 1, 0, 0.1, S, 0.2, dist=None, torch=torch)
        tris = torch.from_numpy(np.ascontiguousarray(
            __import__("drone_path_planning_python_amd.stl", fromlist=["box_mesh"]).box_mesh((-1, -1, -1), (0, 0, 0)))).cuda()
        mmd, mhit = comp.mesh(res.positions_all, tris, 0.2)
        torch.cuda.synchronize()
    finally:
        ctx7.use_own_stream()
    hcoef, hdur, _ = ctx7.solve_batch(wp, t)
    np.testing.assert_array_equal(coef.cpu().numpy(), hcoef)
    hpos = ctx7.sample(hcoef, hdur, 0.1, S, 3)
    np.testing.assert_array_equal(res.positions_all.cpu().numpy(), hpos)
    hmd, hpartner, hhit = ctx7.formation_collide(hpos, hpos, 0.2)
    np.testing.assert_array_equal(res.min_dist.cpu().numpy(), hmd)
    np.testing.assert_array_equal(res.partner.cpu().numpy(), hpartner)
    np.testing.assert_array_equal(res.hit.cpu().numpy().astype(bool), hhit)
    hm, hh = ctx7.mesh_sweep(hpos, tris.cpu().numpy(), 0.2)
    np.testing.assert_array_equal(mmd.cpu().numpy(), hm)
    assert (res.lo, res.hi) == (0, 70)


def test_c_abi_from_plain_c(tmp_path):
    """include/msnap.h consumed by a C99 program compiled with gcc (no C++, no Python in the
    loop): configs[0] solved on the GPU against the reference's known-answer vector."""
    import subprocess
    from conftest import ROOT
    from drone_path_planning_python_amd import _lib
    exe = str(tmp_path / "abi_smoke")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "abi_smoke.c"), "-o", exe, "-L", libdir, "-lmsnap", "-lm",
                    "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "max abs err" in out and "dur 1.0 2.0 1.0" in out


def test_snap_cost_and_optimality(ctx7, golden):
    """J from the GPU equals exact polynomial integration, and the solved trajectory is the
    minimiser: any other feasible trajectory (same waypoints and end conditions, C^3) costs more.
    This is the QP view of the reference's collocation system."""
    wp, t = golden["cfg2_wp"][:6], golden["cfg2_t"][:6]
    coef, dur, status = ctx7.solve_batch(wp, t)
    J = ctx7.snap_cost(coef, dur)
    for d in range(6):
        np.testing.assert_allclose(J[d], O.snap_cost(coef[d], dur[d]), rtol=1e-10)
    np.testing.assert_allclose(J, ctx7.snap_cost(golden["cfg2_coef"][:6], golden["cfg2_dur"][:6]), rtol=1e-9)
    # a feasible competitor: move one interior waypoint time slightly -> different knot derivatives,
    # re-time back by evaluating on the original grid is not feasible in general; instead perturb the
    # interior knot derivatives directly through the Hermite form of each segment
    rng = np.random.default_rng(0)
    d = 0
    M = dur.shape[1]
    for trial in range(5):
        pert = coef[d].copy()
        # endpoint states of every segment (value + 3 derivatives at both ends), axis by axis
        for a in range(4):
            states = np.zeros((M + 1, 4))
            for i in range(M):
                c = coef[d, i, a]
                states[i] = [c[0], c[1], 2 * c[2], 6 * c[3]]
            cl = coef[d, M - 1, a]
            for j in range(4):
                der = np.polynomial.Polynomial(cl).deriv(j)
                states[M, j] = der(dur[d, M - 1])
            states[1:M, 1:] += rng.normal(scale=0.05, size=(M - 1, 3)) * np.abs(states[1:M, 1:]).max()
            for i in range(M):
                T = dur[d, i]
                A = np.zeros((8, 8))
                for j in range(4):
                    A[j] = O.deriv_row(j, 0.0)
                    A[4 + j] = O.deriv_row(j, T)
                pert[i, a] = np.linalg.solve(A, np.concatenate([states[i], states[i + 1]]))
        Jp = O.snap_cost(pert, dur[d])
        assert (Jp >= J[d] * (1 - 1e-9)).all() and (Jp > J[d]).any()


@pytest.mark.parametrize("env_name,robot_name,lo,hi", [
    ("env-scene-ltu-experiment.stl", "custom_triangle_robot.stl", (-3, 2.5, -0.5), (3, 5.5, 2.5)),
    ("env-scene-hole.stl", "robot-scene-triangle.stl", (-5, -3, -3), (5, 3, 3)),
])
def test_mesh_validity_batch(ctx7, env_name, robot_name, lo, hi):
    """Batched isStateValid (RB_planning_sep_coll_check.py:208-226) on the reference's own STL
    scenes (vertices rounded to 2 dp as fcl_checker.py:19-25 does), against the oracle's
    separating-axis predicate; FCL itself is absent, so the predicate's parity is unpinned."""
    from drone_path_planning_python_amd import stl
    env = stl.load_stl_planner(os.path.join(GOLDEN_DIR, env_name))
    rob = stl.load_stl_planner(os.path.join(GOLDEN_DIR, robot_name))
    rng = np.random.default_rng(11)
    n = 300
    states = np.column_stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n),
                              rng.uniform(lo[2], hi[2], n), rng.uniform(-np.pi, np.pi, n)])
    got = ctx7.mesh_validity(states, rob, env)
    ref = O.mesh_validity(states, rob, env)
    np.testing.assert_array_equal(got, ref)
    assert ref.any() and not ref.all()


def test_mesh_validity_reference_start_goal(ctx7):
    """The live configuration of scripts/rigidBodyPath.py:139-147: start (0,3,1) and goal (0,5,1)
    on either side of the wall at y in [3.9, 4.1] are valid, a pose inside the wall is not."""
    from drone_path_planning_python_amd import stl
    env = stl.load_stl_planner(os.path.join(GOLDEN_DIR, "env-scene-ltu-experiment.stl"))
    rob = stl.load_stl_planner(os.path.join(GOLDEN_DIR, "custom_triangle_robot.stl"))
    states = np.array([[0, 3, 1, 0], [0, 5, 1, 0], [0, 4, 1, 0.3], [0, 4, 2.5, 0.0], [0, 3.6, 1.0, np.pi / 2]])
    np.testing.assert_array_equal(ctx7.mesh_validity(states, rob, env), [True, True, False, True, False])
    assert ctx7.mesh_validity(np.zeros((0, 4)), rob, env).shape == (0,)


def test_mesh_sweep_on_reference_obstacle(ctx7):
    """Drone-vs-mesh sweep against the reference's obstacle file (resources/stl, copied as data)."""
    from drone_path_planning_python_amd import stl
    tris = stl.load_stl(os.path.join(GOLDEN_DIR, "env-scene-hole.stl"))
    assert tris.shape == (56, 3, 3)
    rng = np.random.default_rng(12)
    pos = rng.uniform([-5, -1.5, -3], [5, 1.5, 3], size=(24, 15, 3))
    md, hit = ctx7.mesh_sweep(pos, tris, 0.15)
    rmd, rhit = O.mesh_sweep(pos, tris, 0.15)
    np.testing.assert_allclose(md, rmd, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(hit, rhit)


@pytest.mark.parametrize("script", ["01_single_trajectory.py", "02_swarm_batch.py", "03_formation_collision.py"])
def test_examples_run(script):
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script)], check=True, capture_output=True,
                         text=True, timeout=300).stdout
    assert len(out.splitlines()) >= 3


@pytest.mark.parametrize("n,m,S", [(70, 8, 40), (300, 10, 91), (129, 20, 96), (5, 3, 7), (260, 6, 300)])
def test_sampler_row_image_feeds_the_pairwise_pass(ctx7, n, m, S):
    """msnap_sample_collide_device: the positions are the sampler's, bit for bit, and its second output IS the
    transposed row image [S][3][pitch] (incl. paths too long for the LDS image: 300 samples); the pairwise
    pass run from that image equals the pass that transposes by itself, the host-pointer entry and the oracle."""
    import torch
    import c_oracle
    from drone_path_planning_python_amd import swarm as sw
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(700 + n, n, m)
    wp[..., :3] *= 0.3
    comp = sw.DeviceCompute(ctx7, torch)
    try:
        coef, dur, status = comp.solve(torch.from_numpy(wp).cuda(), torch.from_numpy(t).cuda())
        assert int(status.abs().sum().item()) == 0
        pos = comp.sample(coef, dur, 0.1, S)
        pos2, pos_t = comp.sample_rows_t(coef, dur, 0.1, S)
        np.testing.assert_array_equal(pos2.cpu().numpy(), pos.cpu().numpy())
        pitch = (n + 127) // 128 * 128
        img = pos_t.cpu().numpy().reshape(S, 3, pitch)
        np.testing.assert_array_equal(img[:, :, :n], pos.cpu().numpy().transpose(1, 2, 0))
        a = comp.collide(pos, 0, pos, 0.2)
        b = comp.collide(pos2, 0, pos2, 0.2, rows_t=pos_t)
        ref = c_oracle.formation_collide(pos.cpu().numpy(), 0.2)
        for x, y, z in zip(a, b, ref):
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
            np.testing.assert_array_equal(y.cpu().numpy().astype(z.dtype), z)
        res = sw.formation_pass(comp, coef, dur, n, 1, 0, 0.1, S, 0.2, torch=torch)      # takes the row-image route
        np.testing.assert_array_equal(res.min_dist.cpu().numpy(), ref[0])
        np.testing.assert_array_equal(res.partner.cpu().numpy(), ref[1])
    finally:
        torch.cuda.synchronize()
        ctx7.use_own_stream()


def test_collide_rows_that_are_not_the_slice_of_the_columns(ctx7):
    """include/msnap.h: the once-per-pair evaluation assumes pos_rows == pos_cols[row_offset : row_offset + n_rows].
    The host-pointer entry compares the arrays and evaluates one-sidedly when they differ (device callers set
    "collide_no_sym"); either way the rows' minima against the given columns must be exact."""
    rng = np.random.default_rng(77)
    cols = rng.uniform(-3, 3, size=(400, 30, 3))
    rows = rng.uniform(-3, 3, size=(300, 30, 3))              # NOT cols[50:350]
    md, partner, hit = ctx7.formation_collide(rows, cols, 0.25, row_offset=50)
    assert ctx7.get_option("collide_last_sym") == 0
    d2 = np.full((300, 400), np.inf)
    for j in range(400):
        d = cols[j][None] - rows
        d2[:, j] = np.fmin.reduce(O.fma_square(d[..., 2], O.fma_square(d[..., 1], d[..., 0] * d[..., 0])), axis=1)
    d2[np.arange(300), 50 + np.arange(300)] = np.inf        # a row never meets the column of its own global index
    np.testing.assert_array_equal(md, np.sqrt(d2.min(axis=1)))
    np.testing.assert_array_equal(partner, d2.argmin(axis=1))
    # the aliased call takes the symmetric route again
    ctx7.formation_collide(cols[50:350], cols, 0.25, row_offset=50)
    assert ctx7.get_option("collide_last_sym") == 1


def test_mesh_sweep_with_partially_nonfinite_paths(ctx7):
    """A 64-sample stretch that mixes NaN / inf and finite samples (e.g. Horner overflow late in a path): the
    non-finite samples never win a minimum, and they must not distort the cull of the finite ones -- the
    bounding box of the stretch is built from the finite samples only.  Against the C oracle on the
    reference's wall scene, with the finite samples on both sides of the non-finite ones."""
    import c_oracle
    from drone_path_planning_python_amd import stl
    tris = np.concatenate([stl.load_stl(os.path.join(GOLDEN_DIR, "env-scene-hole.stl")),
                           stl.load_stl(os.path.join(GOLDEN_DIR, "env-scene-ltu-experiment.stl"))])
    rng = np.random.default_rng(5)
    n, S = 48, 96
    start = rng.uniform([-6, -8, -2], [6, -3, 3], size=(n, 1, 3))
    pos = start + np.linspace(0, 1, S)[None, :, None] * rng.uniform([-2, 8, -1], [2, 14, 1], size=(n, 1, 3))
    for d in range(n):
        k = d % 6
        if k == 0:
            pos[d, 5:40] = np.nan                       # a NaN stretch inside the first wave
        elif k == 1:
            pos[d, ::2, 1] = np.nan                     # every other sample, one coordinate
        elif k == 2:
            pos[d, 60:] = np.inf                        # overflow late in the path
        elif k == 3:
            pos[d, :64] = np.nan                        # the whole first wave
        elif k == 4:
            pos[d] = np.nan                             # a failed drone
    md, hit = ctx7.mesh_sweep(pos, tris, 0.3)
    rmd, rhit = c_oracle.mesh_sweep(pos, tris, 0.3)
    np.testing.assert_allclose(md, rmd, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(hit, rhit)
    assert np.isinf(md[4]) and not hit[4] and hit.any()


@pytest.mark.parametrize("order,n,m,S,fused", [(7, 4096, 10, 91, 1), (7, 4096, 20, 96, 0), (7, 257, 5, 33, 1),
                                               (9, 100, 11, 40, 1), (7, 37, 12, 50, 0), (7, 64, 24, 30, 0),
                                               (9, 1000, 10, 91, 1), (7, 5, 1, 7, 1), (9, 333, 7, 64, 1),
                                               (7, 130, 8, 700, 1), (7, 40, 6, 2700, 0), (7, 3100, 3, 20, 1),
                                               (7, 4099, 9, 91, 1), (9, 3333, 11, 91, 1)])
def test_solve_and_sampler_in_one_launch(order, n, m, S, fused):
    """msnap_solve_grid_sample_device: coefficients, durations, status, positions and the hand-over buffer are those of
    msnap_solve_grid_device followed by the sampler, bit for bit -- through the fused kernel where it applies (the
    kernel name says which ran) and through the two launches beyond its range (12 and more segments, 2700 samples); a drone with
    a non-finite waypoint gets its status and NaN outputs exactly as there."""
    import torch
    from drone_path_planning_python_amd import Context, swarm as sw
    from drone_path_planning_python_amd.synthetic import swarm
    ctx = Context(order=order)
    try:
        wp, _ = swarm(900 + n, n, m)
        wp[..., :3] *= 0.3
        if n > 4:
            wp[3, m // 2, 1] = np.nan
            wp[n - 1, 0, 3] = np.inf
        t = np.linspace(0.0, 10.0, m + 1)
        ctx.prepare_grid(t)
        comp = sw.DeviceCompute(ctx, torch)
        d_wp = torch.from_numpy(wp).cuda()
        for n_cols in (None, n):
            c0, d0, s0 = comp.solve_grid(d_wp)
            if n_cols is None:
                p0, t0 = comp.sample(c0, d0, 0.1, S), None
            else:
                p0, t0 = comp.sample_rows_t(c0, d0, 0.1, S, n_cols=n_cols)
            c1, d1, s1, p1, t1 = comp.solve_grid_sample(d_wp, 0.1, S, n_cols=n_cols)
            assert ctx.last_kernel().startswith("msnap::grid_sample_kernel") == bool(fused), ctx.last_kernel()
            for a, b in ((c0, c1), (d0, d1), (s0, s1), (p0, p1)):
                np.testing.assert_array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
            assert (t0 is None) == (t1 is None)
            if t0 is not None:
                keys = ctx.collide_takes_broad_phase(n, 0, n, S)
                used = n * 6 * 8 + n * 4 if keys else None      # boxes + keys; the row image's padding rows are not written
                a, b = t0.cpu().numpy().view(np.uint8), t1.cpu().numpy().view(np.uint8)
                if keys:
                    np.testing.assert_array_equal(a[:used], b[:used])
                else:
                    pitch = (n + 127) // 128 * 128
                    np.testing.assert_array_equal(t0.cpu().numpy().reshape(S, 3, pitch)[:, :, :n],
                                                  t1.cpu().numpy().reshape(S, 3, pitch)[:, :, :n])
                # and the pairwise pass accepts either hand-over
                r0 = comp.collide(p0, 0, p0, 0.2, rows_t=t0)
                r1 = comp.collide(p1, 0, p1, 0.2, rows_t=t1)
                for x, y in zip(r0, r1):
                    np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
        if n > 4:
            st = s1.cpu().numpy()
            assert st[3] != 0 and st[n - 1] != 0 and np.count_nonzero(st) == 2
            assert np.isnan(p1[3].cpu().numpy()).all() and np.isfinite(p1[2].cpu().numpy()).all()
        # the A/B switch runs the two kernels
        ctx.set_option("no_grid_sample", 1)
        c2, d2, s2, p2, _ = comp.solve_grid_sample(d_wp, 0.1, S)
        assert not ctx.last_kernel().startswith("msnap::grid_sample_kernel")
        np.testing.assert_array_equal(p2.cpu().numpy().view(np.uint8), p1.cpu().numpy().view(np.uint8))
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_reused_outputs_are_the_same_tensors_with_the_same_results(ctx7):
    """swarm.DeviceCompute(reuse_outputs=True): every method hands back the same output tensors on each call (valid
    until its next call); the results are those of the allocating form, and two methods never share a buffer (the
    pairwise pass's min_dist and the mesh sweep's have the same shape)."""
    import torch
    from drone_path_planning_python_amd import swarm as sw
    from drone_path_planning_python_amd.synthetic import swarm
    n, m, S = 300, 10, 40
    wp, _ = swarm(31, n, m)
    wp[..., :3] *= 0.3
    t = np.linspace(0.0, 10.0, m + 1)
    ctx7.prepare_grid(t)
    d_wp = torch.from_numpy(wp).cuda()
    tris = torch.from_numpy(np.random.default_rng(5).uniform(-3, 3, size=(20, 3, 3))).cuda()
    plain, reuse = sw.DeviceCompute(ctx7, torch), sw.DeviceCompute(ctx7, torch, reuse_outputs=True)
    try:
        ref = plain.solve_grid_sample(d_wp, 0.1, S, n_cols=n)
        a = reuse.solve_grid_sample(d_wp, 0.1, S, n_cols=n)
        b = reuse.solve_grid_sample(d_wp, 0.1, S, n_cols=n)
        pitch = (n + 127) // 128 * 128
        for k, (x, y, z) in enumerate(zip(ref, a, b)):
            assert y.data_ptr() == z.data_ptr() and x.data_ptr() != y.data_ptr()
            xs, ys = x.cpu().numpy(), y.cpu().numpy()
            if k == 4:      # the row image [S][3][pitch]: its padding rows are not written
                xs, ys = xs.reshape(S, 3, pitch)[:, :, :n], ys.reshape(S, 3, pitch)[:, :, :n]
            np.testing.assert_array_equal(xs, ys)
        c1 = reuse.collide(a[3], 0, a[3], 0.2, rows_t=a[4])
        m1 = reuse.mesh(a[3], tris, 0.2)
        assert c1[0].data_ptr() != m1[0].data_ptr() and c1[2].data_ptr() != m1[1].data_ptr()
        c0 = plain.collide(ref[3], 0, ref[3], 0.2, rows_t=ref[4])
        m0 = plain.mesh(ref[3], tris, 0.2)
        for x, y in zip(c0 + m0, c1 + m1):
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
        assert reuse.collide(a[3], 0, a[3], 0.2, rows_t=a[4])[0].data_ptr() == c1[0].data_ptr()
    finally:
        torch.cuda.synchronize()
        ctx7.use_own_stream()
