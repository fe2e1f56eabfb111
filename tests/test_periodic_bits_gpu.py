"""The periodic solve against recorded bits: tests/golden/periodic_bits.npz holds coefficients, durations and status of
msnap_solve_periodic_device as the last build computed them in which periodic_solve_kernel<K> had an elimination text of
its own (tests/golden/make_periodic_bits_golden.py).  The kernel is a wrapper around ring_solve now
(csrc/msnap_ring.h), the text the time allocation on loops runs as its trial; a change to it that only moves
instructions, data or control flow must give the same bytes at every branch: two segments (knot 1 is knot M-1, no trip
of either backward loop), three (their first trip, and the refinement's first S_i from the stash), four, the cap of
each order (LDS above 64 KiB), per-drone and shared times, clean batches and failed drones next to healthy ones in a
tile.  Each launch is at most 17 drones into sentinel-filled outputs longer than the batch."""
import numpy as np
import pytest

import periodic_bits_cases as PB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def archive():
    with np.load(PB.GOLDEN) as z:
        return {k: z[k] for k in z.files if k != "csrc_sha"}


@pytest.fixture(scope="module")
def contexts():
    from drone_path_planning_python_amd import Context
    ctxs = {o: Context(device_id=0, order=o, max_segments=64) for o in (7, 9)}
    yield ctxs
    for c in ctxs.values():
        c.close()


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    as_int = np.int64 if got.dtype == np.float64 else got.dtype
    assert np.array_equal(np.ascontiguousarray(got).view(as_int), np.ascontiguousarray(want).view(as_int)), what


@pytest.mark.parametrize("case", PB.CASES, ids=PB.case_id)
def test_periodic_bits(archive, contexts, case):
    clean = archive[PB.key(case, "clean", "coef")]
    for batch in PB.batches(case):
        # (asserts that nothing was written behind the batch)
        coef, dur, status = PB.solve(contexts[case["order"]], case, *PB.inputs(case, batch))
        what = f"{PB.case_id(case)}/{batch}: "
        _same_bits(status, archive[PB.key(case, batch, "status")], what + "status")
        _same_bits(dur, archive[PB.key(case, batch, "dur")], what + "durations")
        stored = sorted(PB.changed(case, batch)) if batch != "clean" else list(range(case["n"]))
        _same_bits(coef[stored], archive[PB.key(case, batch, "coef")], what + "coefficients of the drones it changes")
        # expected status words, finite / NaN rows, and every untouched drone -- the healthy neighbours of a failed drone
        # in the same tile among them -- as in the recorded clean batch
        PB.check(case, batch, coef, dur, status, clean)
