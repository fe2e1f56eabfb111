"""The callers of the open-chain elimination that tests/test_rolled_bits_gpu.py does not reach, against recorded bits:
tests/golden/chain_bits_*.npz hold every output of gates_solve_kernel<K> (K21: coefficients, durations, status) and of
the rest, end-state and free-total modes of timeopt_kernel<K, MODE> (K8: also t_out, cost, pg, iters) as the last build
computed them in which the time allocation's trial wrote the elimination out a second time
(tests/golden/make_chain_bits_golden.py).  One changed unit in the last place of a trial's cost can change an Armijo
decision, so the allocator's outputs are held as 64-bit integers like the solves'.

K21: one gated knot, two knots and the segment caps; no knot gated, every bit at every knot, and knots gated by no
drone of the tile next to knots gated by some; an out-of-range mask and a non-finite prescribed value beside healthy
drones.  K8, each of the three modes at both orders: one segment (no knot, no stash), two (one knot takes both end
terms), three, and the first segment count with 8-drone tiles; max_iter 0 and 5, end states given and absent, shared
and per-drone times; a NaN waypoint and a backwards time beside healthy drones.  Where a case can move, the seeds are
such that the NumPy restatement takes an accepted and a rejected trial on a drone of every tile, and the kernel's iters
is asserted >= 1 there (chain_bits_cases.check): more than the start trial is pinned.  Each launch is at most 17 drones
into sentinel-filled outputs longer than the batch."""
import numpy as np
import pytest

import chain_bits_cases as CB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def archives():
    out = {}
    for path in sorted({CB.golden_path(c) for c in CB.CASES}):
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


@pytest.mark.parametrize("case", CB.CASES, ids=CB.case_id)
def test_chain_bits(archives, contexts, case):
    clean = {f: archives[CB.key(case, "clean", f)] for f in CB.fields(case)}
    for batch in CB.batches(case):
        got = CB.run(contexts[case["order"]], case, batch)      # (asserts that nothing was written behind the batch)
        for f in CB.fields(case):
            want = archives[CB.key(case, batch, f)]
            rows = got[f][CB.stored_rows(case, batch, f)]
            what = f"{CB.case_id(case)}/{batch}: {f}"
            assert rows.dtype == want.dtype and rows.shape == want.shape, what
            assert np.array_equal(CB.bits(rows), CB.bits(want)), what
        # expected status words, finite / NaN rows, every untouched drone as in the recorded clean batch, accepted steps
        CB.check(case, batch, got, clean)
