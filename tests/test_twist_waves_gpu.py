"""The small-batch solve (solve_kernel_twist) at one, two and four waves per 8-drone tile: the multi-wave forms only
move where the same arithmetic runs, so coefficients, durations and status must be the one-wave form's byte for byte
-- every segment count the kernel serves, partial last tiles, the t[0] != 0 quirk and failed drones included.  Every
solve writes into fresh sentinel-filled device outputs: a store a form leaves out cannot hide behind another run's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 37, 256, 300)


def _inputs(order, m, n, shared):
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(9100 + 31 * m + order, n, m, shared_times=shared)
    if not shared:
        t[n - 1] += 0.25                                  # a drone with t[0] != 0 (the tile's last)
        if n >= 7:
            wp[3, m // 2, 1] = np.nan                    # non-finite waypoint
            t[5, m - 1] = t[5, m - 2]                    # zero-length segment: bad times
    return wp, t


def _solve(ctx, waves, wp, t):
    """One solve into FRESH sentinel-filled device outputs (solve_cases.solve_fresh: a piece, a duration or a status
    word that a form fails to store shows up as the sentinel instead of another run's value left in reused buffers)."""
    from solve_cases import solve_fresh
    ctx.set_option("twist_waves", waves)
    try:
        out = solve_fresh(ctx, wp, t)
    finally:
        ctx.set_option("twist_waves", 0)
    assert ctx.last_kernel().startswith("msnap::solve_kernel_twist<"), ctx.last_kernel()
    return out


def _same_bytes(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("order,m", [(7, m) for m in range(2, 25)] + [(9, m) for m in range(2, 13)])
def test_twist_waves_bitwise(order, m):
    from drone_path_planning_python_amd import Context
    with Context(order=order, max_segments=64) as ctx:
        for n in SIZES:
            for shared in ((False, True) if n == 37 else (False,)):
                wp, t = _inputs(order, m, n, shared)
                one = _solve(ctx, 1, wp, t)
                for waves in (2, 4):
                    other = _solve(ctx, waves, wp, t)
                    for x, y in zip(one, other):
                        _same_bytes(x, y)
                if not shared and n >= 7:
                    st = one[2]
                    assert st[3] != 0 and st[5] != 0 and np.isnan(one[0][3]).all() and np.isnan(one[0][5]).all()
                    keep = np.ones(n, bool)
                    keep[[3, 5]] = False
                    assert (st[keep] == 0).all()
                else:
                    assert (one[2] == 0).all()


@pytest.mark.parametrize("n", [256, 1000, 2048])
def test_twist_waves_default_is_bitwise_and_validated(n):
    """The launcher's choice (0; four, two or one wave by tile count on a 256-CU chip) gives the same bytes, through
    the device entry and through the host-pointer one; values other than 0, 1, 2, 4 are refused."""
    from drone_path_planning_python_amd import Context, MsnapError
    wp, t = _inputs(7, 10, n, False)
    with Context(order=7, max_segments=64) as ctx:
        assert ctx.get_option("twist_waves") == 0
        one = _solve(ctx, 1, wp, t)
        for dflt in (_solve(ctx, 0, wp, t), ctx.solve_batch(wp, t)):
            for x, y in zip(one, dflt):
                _same_bytes(x, y)
        for bad in (3, 5, 8):
            with pytest.raises(MsnapError):
                ctx.set_option("twist_waves", bad)
        assert ctx.get_option("twist_waves") == 0


@pytest.mark.parametrize("waves", [1, 4])
def test_twist_grid_ignores_grid_options(waves):
    """The twist grid is the tile count: a cap on the persistent grids (solve_grid_waves) or a twist_max_drones that
    still admits the batch must not change which tiles run."""
    from drone_path_planning_python_amd import Context
    n, m = 300, 10
    wp, t = _inputs(7, m, n, False)
    with Context(order=7, max_segments=64) as ctx:
        ref = _solve(ctx, waves, wp, t)
        for grid_waves, twist_max in ((1, 0), (3, 0), (0, n), (2, n + 1), (0, 4096)):
            ctx.set_option("solve_grid_waves", grid_waves)
            ctx.set_option("twist_max_drones", twist_max)
            try:
                got = _solve(ctx, waves, wp, t)
            finally:
                ctx.set_option("solve_grid_waves", 0)
                ctx.set_option("twist_max_drones", 0)
            for x, y in zip(ref, got):
                _same_bytes(x, y)
