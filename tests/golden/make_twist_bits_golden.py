#!/usr/bin/env python3
"""Writes tests/golden/twist_bits.npz: coefficients, durations and status, bit for bit, of the small-batch solve
(solve_kernel_twist) as a given build of the library computes them on a GPU, for the batches of
tests/twist_bits_cases.py.  The archive committed with this file was recorded from the last commit before the kernel's
status reduction left the common path: tests/test_twist_bits_gpu.py holds every later build to those bits.

Select the library to record from with MSNAP_LIB_PATH and give the directory of the sources it was built from, whose
hash the archive carries as `csrc_sha`; an optional second argument is the archive to write:

    MSNAP_LIB_PATH=/elsewhere/csrc/libmsnap.so python tests/golden/make_twist_bits_golden.py /elsewhere/csrc [OUT.npz]

Before anything is written the recorder checks what the test relies on: one, two and four waves per tile give the same
bytes; every drone whose inputs a batch leaves alone comes out as in the clean batch; the status words are the expected
ones and a failed drone's coefficients are all NaN.  Keys: o<order>_m<segments>/<batch>/<coef|dur|status>; `coef` holds
the rows of twist_bits_cases.STORED[batch] only."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import twist_bits_cases as TB  # noqa: E402


def csrc_sha(d):
    """drone_path_planning_python_amd._lib.csrc_sha over the sources in `d`."""
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


def main():
    from drone_path_planning_python_amd import Context, _lib
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(_lib.LIB_PATH)
    out = sys.argv[2] if len(sys.argv) > 2 else TB.GOLDEN
    arc = {"csrc_sha": np.array(csrc_sha(src))}
    print("recording from", _lib.LIB_PATH, "built from csrc", arc["csrc_sha"])
    ctxs = {o: Context(device_id=0, order=o, max_segments=64) for o in (7, 9)}
    for order, m in TB.INSTANCES:
        clean = None
        for batch in TB.CHANGED:
            wp, t = TB.inputs(order, m, batch)
            coef, dur, status = TB.solve(ctxs[order], 1, wp, t)
            for waves in (2, 4):
                for x, y in zip((coef, dur, status), TB.solve(ctxs[order], waves, wp, t)):
                    assert x.tobytes() == y.tobytes(), (order, m, batch, waves)
            assert np.array_equal(status, TB.expected_status(batch)), (order, m, batch, status)
            if batch == "clean":
                clean = coef
            same = [d for d in range(TB.N) if d not in TB.STORED[batch]]
            assert coef[same].tobytes() == clean[same].tobytes(), (order, m, batch)
            assert all(np.isnan(coef[d]).all() for d in TB.CHANGED[batch]), (order, m, batch)
            arc[TB.key(order, m, batch, "coef")] = coef[list(TB.STORED[batch])]
            arc[TB.key(order, m, batch, "dur")] = dur
            arc[TB.key(order, m, batch, "status")] = status
            print(order, m, batch, "status", status.tolist())
    for c in ctxs.values():
        c.close()
    np.savez_compressed(out, **arc)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
