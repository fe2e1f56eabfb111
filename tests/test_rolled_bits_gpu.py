"""The rolled solve kernels against recorded bits: tests/golden/rolled_bits_*.npz hold coefficients, durations and
status of solve_kernel<K, false> (LDS stash), solve_kernel<K, true> (global slab) and states_solve_kernel<K> as the last
build in which the two were separate texts computed them (tests/golden/make_rolled_bits_golden.py).  Both are wrappers
around one body now (csrc/msnap_rolled.h); a change to it that only moves instructions, data or control flow must give
the same bytes at every branch of the body: one segment, one knot, the longest paths of each stash, start and end
states given or not, per-drone and shared times, clean batches, a drone with t[0] != 0, and failed drones next to
healthy ones in a tile.  Each launch is at most 17 drones into sentinel-filled outputs longer than the batch."""
import numpy as np
import pytest

import rolled_bits_cases as RB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def archives():
    out = {}
    for path in sorted({RB.golden_path(c) for c in RB.CASES}):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files if k != "csrc_sha"})
    return out


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


@pytest.mark.parametrize("case", RB.CASES, ids=RB.case_id)
def test_rolled_bits(archives, contexts, case):
    clean = archives[RB.key(case, "clean", "coef")]
    for batch in RB.batches(case):
        # (asserts the kernel instance that ran, and that nothing was written behind the batch)
        coef, dur, status = RB.solve(contexts[case["order"]], case, *RB.inputs(case, batch))
        what = f"{RB.case_id(case)}/{batch}: "
        _same_bits(status, archives[RB.key(case, batch, "status")], what + "status")
        _same_bits(dur, archives[RB.key(case, batch, "dur")], what + "durations")
        stored = sorted(RB.changed(case, batch)) if batch != "clean" else list(range(case["n"]))
        _same_bits(coef[stored], archives[RB.key(case, batch, "coef")], what + "coefficients of the drones it changes")
        # expected status words, finite / NaN rows, and every untouched drone -- the healthy neighbours of a failed drone
        # in the same tile among them -- as in the recorded clean batch
        RB.check(case, batch, coef, dur, status, clean)
