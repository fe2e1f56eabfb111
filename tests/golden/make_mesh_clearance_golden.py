#!/usr/bin/env python3
"""Writes tests/golden/mesh_clearance_golden.npz: the exact reference's D (tests/mesh_clearance_exact.py, Fractions
and mpmath at 60 digits) for the cases of tests/mesh_clearance_cases.py (CONTRACT and certify_case), rounded to fp64.  Minutes of CPU.

    python tests/golden/make_mesh_clearance_golden.py
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import mesh_clearance_cases as MC  # noqa: E402
import mesh_clearance_exact as ME  # noqa: E402


def one(job):
    name, d = job
    coef, dur, tris = MC.certify_case() if name == "certify_hole" else MC.contract_case(name)
    _, tm, _, _ = ME.fp64_mesh_clearance(coef[d:d + 1], dur[d:d + 1], tris)
    D, _ = ME.exact_mesh_clearance(coef[d], dur[d], tris, hint_t=[float(tm[0])])
    return name, d, float(D)


def main():
    sizes = {name: n for name, (_, _, n, _) in MC.CONTRACT.items()}
    sizes["certify_hole"] = 12
    jobs = [(name, d) for name, n in sizes.items() for d in range(n)]
    out = {name: np.zeros(n) for name, n in sizes.items()}
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for name, d, D in ex.map(one, jobs):
            out[name][d] = D
            print(name, d, repr(D), flush=True)
    np.savez(MC.GOLDEN, **out)


if __name__ == "__main__":
    main()
