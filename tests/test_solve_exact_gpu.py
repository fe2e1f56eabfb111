"""Every K1 solve instance (tests/solve_cases.py: one entry per kernel instance a small batch can launch) against the
60-digit solutions of tests/solve_exact.py, on two per-drone grids -- the suite's even draw and the uneven draw of
tools/solve_stress.py -- with one raised start each, plus one shared-grid launch per family at 10 segments.

Asserted: the instance the launcher reports, status, durations, the exact parts of the solution (c_0 = w_i on every
segment, the rest start's zeros), that every output word is stored, and the accuracy in conftest.norm_rel at the bars
the project already holds (solve_cases.bar).  Nothing tighter: the sharper figures -- a segment-scaled error, where the
worst element sits, the dense fp64 oracle's own error on the same inputs -- are printed and appended, one line per
launch set, to profiles/solve_accuracy.jsonl, from which tools/solve_accuracy_table.py builds
profiles/solve_accuracy.md."""
import json
import os

import numpy as np
import pytest

import solve_cases as SC
import solve_exact as SX
from conftest import ROOT, norm_rel

pytestmark = pytest.mark.gpu

RECORD = os.path.join(ROOT, "profiles", "solve_accuracy.jsonl")
_started = []
_dense = {}


def _record(line):
    """the first line of a process starts the file anew; a tree that cannot be written to loses the record only"""
    try:
        with open(RECORD, "a" if _started else "w") as f:
            f.write(json.dumps(line) + "\n")
        _started.append(1)
    except OSError:
        pass


def _dense_oracle(wp, t, order):
    """the dense fp64 solve on the same inputs (one per (order, M, grid), shared by the families)"""
    import msnap_oracle as O
    key = (order, wp.tobytes(), t.tobytes())
    if key not in _dense:
        tt = np.broadcast_to(t, (wp.shape[0], t.shape[0])) if t.ndim == 1 else t
        _dense[key] = O.solve_batch_fast(wp, tt, ncoef=order + 1)[0]
    return _dense[key]


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_instance_against_60_digits(case):
    from drone_path_planning_python_amd import Context
    K = SC.khalf(case.order)
    with Context(order=case.order, max_segments=64) as ctx:
        for o in case.opts:
            ctx.set_option(o, 1)
        for grid in (("shared",) if case.shared else ("even", "uneven")):
            wp, t = SC.inputs(case.order, case.M, grid, case.n)
            exact = SX.exact_batch_k1(wp, t, K)
            outs = []
            for waves in case.waves:
                if case.family == "twist":
                    ctx.set_option("twist_waves", waves)
                outs.append(SC.solve_fresh(ctx, wp, t))            # (no sentinel survives: asserted there)
                assert ctx.last_kernel() == case.kernel, (ctx.last_kernel(), waves)
            coef, dur, status = outs[0]
            for other in outs[1:]:                                  # the wave counts of one twist instance: same bytes
                for x, y in zip(outs[0], other):
                    assert x.tobytes() == y.tobytes()
            assert (status == 0).all(), status
            tt = np.broadcast_to(t, (case.n, case.M + 1)) if t.ndim == 1 else t
            T = np.diff(tt, axis=1)
            assert dur.tobytes() == np.ascontiguousarray(T).tobytes()
            keep = np.ones(case.n, bool)
            if grid != "shared":
                keep[SC.raised(case.n)] = False
                assert tt[SC.raised(case.n), 0] == 0.25
            assert (tt[keep, 0] == 0).all()
            assert np.array_equal(coef[keep][..., 0], wp[keep, :-1, :]), "c_0 != w_i"
            assert (coef[keep][:, 0, :, 1:K] == 0).all(), "rest start"

            err, at = SX.norm_rel_at(coef, exact)
            seg, sat = SX.seg_scaled(coef, exact, T)
            dense = _dense_oracle(wp, t, case.order)
            oerr, oat = SX.norm_rel_at(dense, exact)
            oseg, osat = SX.seg_scaled(dense, exact, T)
            limit, limit_name = SC.bar(case.order, case.M, grid)
            print(f"{SC.case_id(case)} {grid}: {case.kernel} norm_rel {err:.2e} at (drone, seg, axis, k) {at}, "
                  f"segment-scaled {seg:.2e} at {sat}; dense oracle {oerr:.2e} at {oat}, {oseg:.2e} at {osat}; "
                  f"bar {limit_name} {limit:g}")
            _record({"family": case.family, "order": case.order, "M": case.M, "grid": grid, "n": case.n,
                     "kernel": case.kernel, "waves": list(case.waves), "bar": limit, "bar_name": limit_name,
                     "norm_rel": err, "norm_rel_at": at, "seg_scaled": seg, "seg_scaled_at": sat,
                     "shortest_seg": [int(i) for i in T.argmin(axis=1)],
                     "oracle_norm_rel": oerr, "oracle_norm_rel_at": oat, "oracle_seg_scaled": oseg,
                     "oracle_seg_scaled_at": osat})
            assert err == norm_rel(coef, exact)
            assert err <= limit, (SC.case_id(case), grid, err, at, limit_name)
