#!/usr/bin/env python3
"""Records the exact solutions of the longest boundary-state cases (tests/states_exact.py: case(order, MAX_SEG[order]),
the three end-state combinations) with the 60-digit collocation of that module:

    python3 tests/golden/make_states_golden.py    -> tests/golden/states_golden.npz (order 7),
                                                     tests/golden/states_golden_order9.npz

The shorter cases are solved when the tests run; these two take about 8 s each.  Needs mpmath and NumPy only."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import states_exact as SE  # noqa: E402


def main():
    for order in (7, 9):
        K, M = (order + 1) // 2, SE.MAX_SEG[order]
        wp, t, start, end = SE.case(order, M)
        out = {"wp": wp, "t": t, "start": start, "end": end, "digits": np.int64(SE.mp.mp.dps)}
        coef = {c: np.empty((wp.shape[0], M, 4, 2 * K)) for c in SE.COMBOS}
        t0 = time.time()
        for d in range(wp.shape[0]):
            sols = SE.exact_solve(t[d], wp[d], [SE.combo_states(c, start[d], end[d]) for c in SE.COMBOS], K)
            for c, s in zip(SE.COMBOS, sols):
                coef[c][d] = s
        for c in SE.COMBOS:
            out["coef_" + c] = coef[c]
        np.savez_compressed(SE.golden_path(order), **out)
        print(f"order {order}: {wp.shape[0]} drones x {M} segments in {time.time() - t0:.1f} s -> {SE.golden_path(order)}")


if __name__ == "__main__":
    main()
