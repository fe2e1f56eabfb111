#!/usr/bin/env python3
"""Records the exact solutions of the longest periodic cases (tests/periodic_exact.py: case(order, MAX_SEG[order])) with
the 60-digit superposition of that module:

    python3 tests/golden/make_periodic_golden.py    -> tests/golden/periodic_golden.npz (order 7),
                                                       tests/golden/periodic_golden_order9.npz

The shorter cases are solved when the tests run.  Needs mpmath and NumPy only."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import periodic_exact as PE  # noqa: E402


def main():
    for order in (7, 9):
        K, M = (order + 1) // 2, PE.MAX_SEG[order]
        wp, t = PE.case(order, M)
        t0 = time.time()
        coef, seam = PE.exact_batch(wp, t, K)
        np.savez_compressed(PE.golden_path(order), wp=wp, t=t, coef=coef, seam=seam, digits=np.int64(PE.mp.mp.dps))
        print(f"order {order}: {wp.shape[0]} drones x {M} segments in {time.time() - t0:.1f} s -> {PE.golden_path(order)}")


if __name__ == "__main__":
    main()
