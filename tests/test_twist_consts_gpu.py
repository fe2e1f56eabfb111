"""The small-batch solve (solve_kernel_twist) with its Hermite constants fetched from the constant-memory table
(msnap_twist_consts.h) on the lean instances and kept as literals on the long ones: both policies, both status paths.

Order 7 with 2, 3, 10 (table) and 11, 24 (literals) segments, order 9 with 2, 6 (table) and 7, 12 (literals); one
drone, a full tile, a tile and one mirrored drone, a tile and a partial one; one, two and four waves per tile; the
batch's last drone starts at t[0] = 0.25.  A second batch carries one failed drone of each kind -- NaN waypoint, time
running backwards, zero duration -- once in the half of the path that side 0 sweeps and once in side 1's.

Required: the three wave counts give the same bytes; the status words are the contract's (include/msnap.h: 3 for a
non-finite input, 2 for times out of order -- the oracles solve and have no status of their own), a failed drone's
coefficients are all NaN and no other drone holds one; the good drones agree with the C oracle within the bar
tests/test_solve_gpu.py holds the same instances to (1e-9 at ten segments and at order 9, 1e-8 for the other order-7
lengths); durations are the oracle's exactly; last_kernel() names the instance."""
import numpy as np
import pytest

from conftest import norm_rel
from solve_cases import khalf, solve_fresh

pytestmark = pytest.mark.gpu

SEGMENTS = {7: (2, 3, 10, 11, 24), 9: (2, 6, 7, 12)}
SIZES = (1, 8, 9, 13)
WAVES = (1, 2, 4)
KINDS = ("nan", "backwards", "zero")          # drones 1..6 of a faulted batch: kind k on side s is drone 1 + 2 k + s
ST_TIMES, ST_NONFINITE = 2, 3


def _bar(order, m):
    return 1e-9 if (order == 9 or m == 10) else 1e-8


def _clean(order, m, n):
    from drone_path_planning_python_amd.synthetic import swarm
    wp, t = swarm(47000 + 100 * order + m, n, m)
    t[n - 1] += 0.25
    return wp, t


def _faulted(wp, t, m):
    wp, t = wp.copy(), t.copy()
    expect = np.zeros(len(wp), dtype=np.int32)
    for k, kind in enumerate(KINDS):
        for side in (0, 1):
            d = 1 + 2 * k + side
            if kind == "nan":
                wp[d, m if side else 0, 1] = np.nan
            else:                               # the first segment of the path, or its last
                i = m if side else 1
                t[d, i] = t[d, i - 1] - (0.1 if kind == "backwards" else 0.0)
            expect[d] = ST_NONFINITE if kind == "nan" else ST_TIMES
    return wp, t, expect


@pytest.fixture(scope="module")
def contexts():
    from drone_path_planning_python_amd import Context
    ctxs = {order: Context(order=order, max_segments=64) for order in (7, 9)}
    yield ctxs
    for c in ctxs.values():
        c.close()


_REF = {}


def _oracle(order, m, n):
    """the C oracle on the clean batch, once per shape (the faulted batch changes only the drones it fails)"""
    if (order, m, n) not in _REF:
        import c_oracle
        wp, t = _clean(order, m, n)
        coef, dur, info, _ = c_oracle.solve_batch(wp, t, ncoef=order + 1, faithful=False, n_threads=4)
        assert (info == 0).all()
        _REF[(order, m, n)] = (coef, dur)
    return _REF[(order, m, n)]


def _solve_all_waves(ctx, order, m, wp, t):
    outs = []
    for waves in WAVES:
        ctx.set_option("twist_waves", waves)
        try:
            outs.append(solve_fresh(ctx, wp, t))
            assert ctx.get_option("twist_waves") == waves
        finally:
            ctx.set_option("twist_waves", 0)
        # (the name carries order, knots of the longer side and segments; the wave count is the option just set)
        want = "msnap::solve_kernel_twist<%d, %d, %d>" % (khalf(order), (m - 2) - (m - 2) // 2, m)
        assert ctx.last_kernel() == want, (ctx.last_kernel(), want)
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    return outs[0]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("order,m", [(o, m) for o in (7, 9) for m in SEGMENTS[o]])
def test_twist_constant_policies(contexts, order, m, n):
    ctx = contexts[order]
    ref, rdur = _oracle(order, m, n)
    wp, t = _clean(order, m, n)
    coef, dur, status = _solve_all_waves(ctx, order, m, wp, t)
    assert (status == 0).all() and not np.isnan(coef).any()
    err = norm_rel(coef, ref)
    print("order %d, %d segments, %d drones: norm-relative error %.3e (bar %.0e)" % (order, m, n, err, _bar(order, m)))
    assert err <= _bar(order, m)
    np.testing.assert_array_equal(dur, rdur)
    if n < 8:
        return
    fwp, ft, expect = _faulted(wp, t, m)
    coef, dur, status = _solve_all_waves(ctx, order, m, fwp, ft)
    np.testing.assert_array_equal(status, expect)
    failed = expect != 0
    assert np.isnan(coef[failed]).all() and not np.isnan(coef[~failed]).any()
    err = norm_rel(coef[~failed], ref[~failed])
    print("    with failed drones: %.3e" % err)
    assert err <= _bar(order, m)
    np.testing.assert_array_equal(dur[~failed], rdur[~failed])
    np.testing.assert_array_equal(dur, ft[:, 1:] - ft[:, :-1])
