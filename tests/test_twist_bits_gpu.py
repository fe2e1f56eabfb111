"""The small-batch solve (solve_kernel_twist) against recorded bits: tests/golden/twist_bits.npz holds coefficients,
durations and status of nine drones (one full 8-drone tile and one partial tile) per instance as the build before the
kernel's status reduction left the common path computed them (tests/golden/make_twist_bits_golden.py).  Changes to the
kernel that only move instructions, data or control flow must give the same bytes at one, two and four waves per
tile: clean batches, a healthy drone with t[0] != 0, failed drones next to healthy ones in a tile, and every failure in
one drone (NONFINITE wins over TIMES).  Each case is one launch of nine drones into sentinel-filled outputs."""
import numpy as np
import pytest

import twist_bits_cases as TB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def archive():
    with np.load(TB.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def contexts():
    from drone_path_planning_python_amd import Context
    ctxs = {o: Context(device_id=0, order=o, max_segments=64) for o in (7, 9)}
    yield ctxs
    for c in ctxs.values():
        c.close()


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.ascontiguousarray(got).view(np.uint8).tobytes() == np.ascontiguousarray(want).view(np.uint8).tobytes(), what


@pytest.mark.parametrize("waves", TB.WAVES)
@pytest.mark.parametrize("batch", list(TB.CHANGED))
@pytest.mark.parametrize("order,m", TB.INSTANCES)
def test_twist_bits(archive, contexts, order, m, batch, waves):
    wp, t = TB.inputs(order, m, batch)
    coef, dur, status = TB.solve(contexts[order], waves, wp, t)      # (asserts that the twist kernel ran)
    want = {f: archive[TB.key(order, m, batch, f)] for f in ("coef", "dur", "status")}
    _same_bytes(status, want["status"], "status")
    assert np.array_equal(status, TB.expected_status(batch))
    _same_bytes(dur, want["dur"], "durations")
    stored = list(TB.STORED[batch])
    _same_bytes(coef[stored], want["coef"], "coefficients of the drones this batch changes")
    # every other drone -- the healthy neighbours of a failed drone in the same tile among them -- as in the clean batch
    same = [d for d in range(TB.N) if d not in stored]
    _same_bytes(coef[same], archive[TB.key(order, m, "clean", "coef")][same], "coefficients of the untouched drones")
    for d in TB.CHANGED[batch]:
        assert np.isnan(coef[d]).all()
