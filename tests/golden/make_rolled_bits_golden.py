#!/usr/bin/env python3
"""Writes tests/golden/rolled_bits_*.npz: coefficients, durations and status, bit for bit, of the rolled solve kernels
(solve_kernel<K, false | true> and states_solve_kernel<K>) as a given build of the library computes them on a GPU, for
the batches of tests/rolled_bits_cases.py.  The archives committed with this file were recorded from the last commit in
which the two kernels were separate texts: tests/test_rolled_bits_gpu.py holds every later build to those bits.

Select the library to record from with MSNAP_LIB_PATH and give the directory of the sources it was built from, whose
hash the archives carry as `csrc_sha`; an optional second argument is the directory to write into:

    MSNAP_LIB_PATH=/elsewhere/csrc/libmsnap.so python tests/golden/make_rolled_bits_golden.py /elsewhere/csrc [OUTDIR]

Before anything is written the recorder checks what the test relies on (rolled_bits_cases.check): the status words are
the expected ones, healthy drones have finite coefficients and failed ones NaN, every drone whose inputs a batch leaves
alone comes out as in the clean batch, and nothing is written behind the batch.  Keys:
<case>/<batch>/<coef|dur|status>; `coef` holds every drone of "clean" and elsewhere only the drones the batch changes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import rolled_bits_cases as RB  # noqa: E402
from make_twist_bits_golden import csrc_sha  # noqa: E402


def main():
    from drone_path_planning_python_amd import Context, _lib
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(_lib.LIB_PATH)
    outdir = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(RB.golden_path(RB.CASES[0]))
    sha = csrc_sha(src)
    print("recording from", _lib.LIB_PATH, "built from csrc", sha)
    ctxs = {o: Context(device_id=0, order=o, max_segments=64) for o in (7, 9)}
    arcs = {}
    for c in RB.CASES:
        arc = arcs.setdefault(os.path.basename(RB.golden_path(c)), {"csrc_sha": np.array(sha)})
        clean = None
        for batch in RB.batches(c):
            coef, dur, status = RB.solve(ctxs[c["order"]], c, *RB.inputs(c, batch))
            if batch == "clean":
                clean = coef
            RB.check(c, batch, coef, dur, status, clean)
            stored = sorted(RB.changed(c, batch)) if batch != "clean" else list(range(c["n"]))
            arc[RB.key(c, batch, "coef")] = coef[stored]
            arc[RB.key(c, batch, "dur")] = dur
            arc[RB.key(c, batch, "status")] = status
            print(RB.case_id(c), batch, "status", status.tolist())
    for ctx in ctxs.values():
        ctx.close()
    for name, arc in arcs.items():
        out = os.path.join(outdir, name)
        np.savez_compressed(out, **arc)
        print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
