#!/usr/bin/env python3
"""Writes tests/golden/chain_bits_*.npz: every output, bit for bit, of gates_solve_kernel<K> (msnap_solve_gates) and of
the rest, end-state and free-total modes of timeopt_kernel<K, MODE> (msnap_optimize_times, _states, _free) as a given
build of the library computes them on a GPU, for the batches of tests/chain_bits_cases.py.  The archives committed with
this file were recorded from the last commit in which the time allocation's trial carried an open-chain elimination of
its own beside rolled_solve_tile's: tests/test_chain_bits_gpu.py holds every later build to those bits.

Select the library to record from with MSNAP_LIB_PATH and give the directory of the sources it was built from, whose
hash the archives carry as `csrc_sha`; an optional second argument is the directory to write into:

    MSNAP_LIB_PATH=/elsewhere/csrc/libmsnap.so python tests/golden/make_chain_bits_golden.py /elsewhere/csrc [OUTDIR]

Before anything is written the recorder checks what the test relies on (chain_bits_cases.check).  Keys:
<case>/<batch>/<field>; coef, dur and t_out hold every drone of "clean" and elsewhere only the drones the batch changes.

    python tests/golden/make_chain_bits_golden.py --search

needs no GPU: it prints the SEEDS and MOVERS tables of chain_bits_cases.py, for every time-allocation case that can
move the first seed at which the NumPy restatement takes an accepted and a rejected trial, each decided by more than
1e-6 of the cost, on one drone of every tile."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import chain_bits_cases as CB  # noqa: E402
from make_twist_bits_golden import csrc_sha  # noqa: E402

def _moves(c, seed, d):
    """Does the restatement take a clear accepted and a clear rejected trial on drone d?"""
    import timeopt_free_ref as F
    import timeopt_ref as R
    import timeopt_states_ref as S
    wp, t, start, end, kT = CB.timeopt_inputs(c, "clean", seed)
    td = t if c["shared"] else t[d]
    s = None if start is None else start[d]
    e = None if end is None else end[d]
    trace, nc = [], c["order"] + 1
    if c["mode"] == "rest":
        R.optimize(wp[d], td, CB.W, CB.MIN_FRACTION, c["max_iter"], CB.TOL, nc, R.fast_cost, trace=trace)
    elif c["mode"] == "ends":
        S.optimize(wp[d], td, s, e, CB.W, CB.MIN_FRACTION, c["max_iter"], CB.TOL, nc, trace=trace)
    else:
        F.optimize(wp[d], td, s, e, CB.W, float(kT[d]), CB.MIN_FRACTION, c["max_iter"], CB.TOL, nc, trace=trace)
    return any(acc and mg > 1e-6 for _, acc, mg in trace) and any(not acc and mg > 1e-6 for _, acc, mg in trace)


def search():
    seeds, movers = {}, {}
    for c in CB.TIMEOPT:
        if not CB.can_move(c):
            continue
        td, n = CB.tile_drones(c), c["n"]
        tiles = [list(range(lo, min(lo + td, n))) for lo in range(0, n, td)]
        for seed in range(1000):
            found = []
            for tile in reversed(tiles):      # (the short tile first: it has the fewest candidates)
                d = next((d for d in tile if _moves(c, seed, d)), None)
                if d is None:
                    break
                found.append(d)
            if len(found) == len(tiles):
                seeds[CB.case_id(c)], movers[CB.case_id(c)] = seed, sorted(found)
                print("#", CB.case_id(c), "seed", seed, "drones", sorted(found), file=sys.stderr, flush=True)
                break
        else:
            raise SystemExit(f"no seed for {CB.case_id(c)}")
    for name, table in (("SEEDS", seeds), ("MOVERS", movers)):
        print(name + " = {")
        for k, v in table.items():
            print(f'    "{k}": {v},')
        print("}")


def main():
    if sys.argv[1:] == ["--search"]:
        return search()
    from drone_path_planning_python_amd import Context, _lib
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(_lib.LIB_PATH)
    outdir = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(CB.golden_path(CB.CASES[0]))
    sha = csrc_sha(src)
    print("recording from", _lib.LIB_PATH, "built from csrc", sha)
    ctxs = {o: Context(device_id=0, order=o, max_segments=64) for o in (7, 9)}
    arcs = {}
    for c in CB.CASES:
        arc = arcs.setdefault(os.path.basename(CB.golden_path(c)), {"csrc_sha": np.array(sha)})
        clean = None
        for batch in CB.batches(c):
            got = CB.run(ctxs[c["order"]], c, batch)
            if batch == "clean":
                clean = got
            CB.check(c, batch, got, clean)
            for f in CB.fields(c):
                arc[CB.key(c, batch, f)] = got[f][CB.stored_rows(c, batch, f)]
            print(CB.case_id(c), batch, "status", got["status"].tolist(),
                  "iters", got["iters"].tolist() if "iters" in got else "-")
    for ctx in ctxs.values():
        ctx.close()
    for name, arc in arcs.items():
        out = os.path.join(outdir, name)
        np.savez_compressed(out, **arc)
        print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
