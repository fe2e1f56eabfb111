#!/usr/bin/env python3
"""Writes tests/golden/mesh_clearance_edges_golden.npz: the exact reference's D (tests/mesh_clearance_exact.py,
Fractions and mpmath at 60 digits) for the solved paths of tests/mesh_clearance_cases.py::CURVED against the 12
triangles of its box, rounded to fp64, and per case the SHA-256 of the inputs it was computed for (coef, dur, tris as
fp64 bytes).  Minutes of CPU.

    python tests/golden/make_mesh_clearance_edges_golden.py
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
    coef, dur, tris = MC.curved_case(name)
    _, tm, _, _ = ME.fp64_mesh_clearance(coef[d:d + 1], dur[d:d + 1], tris)
    D, _ = ME.exact_mesh_clearance(coef[d], dur[d], tris, hint_t=[float(tm[0])])
    return name, d, float(D)


def main():
    jobs = [(name, d) for name, (_, _, n) in MC.CURVED.items() for d in range(n)]
    out = {name: np.zeros(n) for name, (_, _, n) in MC.CURVED.items()}
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for name, d, D in ex.map(one, jobs):
            out[name][d] = D
            print(name, d, repr(D), flush=True)
    for name in MC.CURVED:
        out[name + "_sha256"] = MC.inputs_sha256(*MC.curved_case(name))
    np.savez(MC.EDGES_GOLDEN, **out)


if __name__ == "__main__":
    main()
