#!/usr/bin/env python3
"""profiles/solve_accuracy.md from profiles/solve_accuracy.jsonl, the record tests/test_solve_exact_gpu.py writes while it
runs: per kernel family, order and grid the worst norm_rel and the worst segment-scaled error against the 60-digit
solutions, where they fall, and the dense fp64 oracle's figures on the same cases; then the order-9 families side by side
on the uneven grid at 13..20 segments.  usage: solve_accuracy_table.py [record.jsonl] > profiles/solve_accuracy.md.
No GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("twist", "twin", "reg", "generic", "generic-GS")
GRIDS = ("even", "uneven", "shared")


def where(r, key):
    d, s, a, k = r[key + "_at"]
    short = r["shortest_seg"][d]
    return "M %d drone %d seg %d%s c_%d" % (r["M"], d, s, " (its shortest)" if s == short else "", k)


def main(path):
    rows = [json.loads(line) for line in open(path)]
    out = ["# K1 solve instances against 60-digit solutions", "",
           "Built by `tools/solve_accuracy_table.py` from `profiles/solve_accuracy.jsonl`, which "
           "`tests/test_solve_exact_gpu.py` wrote on an MI355X in the run that passed (%d launch sets).  `norm_rel` is "
           "the suite's metric (per drone and axis, the largest coefficient error over the largest coefficient); the "
           "segment-scaled error is, per drone, segment and axis, max_k |c_k - ref_k| T^k / max_k |ref_k| T^k.  The "
           "oracle columns are the dense fp64 LU (`oracle/msnap_oracle.py::solve_batch_fast`) on the same cases against "
           "the same 60-digit solutions." % len(rows), "",
           "## Worst case per family, order and grid", "",
           "| family | order | grid | segments | cases | bar | worst norm_rel | at | worst segment-scaled | at | "
           "oracle norm_rel | oracle segment-scaled |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for fam in FAMILIES:
        for order in (7, 9):
            for grid in GRIDS:
                for bar in sorted({r["bar"] for r in rows}):
                    sel = [r for r in rows if (r["family"], r["order"], r["grid"], r["bar"]) == (fam, order, grid, bar)]
                    if not sel:
                        continue
                    a = max(sel, key=lambda r: r["norm_rel"])
                    b = max(sel, key=lambda r: r["seg_scaled"])
                    ms = sorted(r["M"] for r in sel)
                    out.append("| %s | %d | %s | %s | %d | %g | %.2e | %s | %.2e | %s | %.2e | %.2e |" % (
                        fam, order, grid, ("%d..%d" % (ms[0], ms[-1]) if len(ms) > 1 else str(ms[0])), len(sel), bar,
                        a["norm_rel"], where(a, "norm_rel"), b["seg_scaled"], where(b, "seg_scaled"),
                        max(r["oracle_norm_rel"] for r in sel), max(r["oracle_seg_scaled"] for r in sel)))
    out += ["", "## Largest value per bar", "", "| bar | order | grid | largest norm_rel | instance |", "|---|---|---|---|---|"]
    for name in sorted({r["bar_name"] for r in rows}):
        for order in (7, 9):
            for grid in GRIDS:
                sel = [r for r in rows if (r["bar_name"], r["order"], r["grid"]) == (name, order, grid)]
                if sel:
                    a = max(sel, key=lambda r: r["norm_rel"])
                    out.append("| %s = %g | %d | %s | %.2e | `%s` M %d |" % (name, a["bar"], order, grid, a["norm_rel"],
                                                                        a["kernel"], a["M"]))
    out += ["", "## Order 9, uneven grid, 13..20 segments: the families on identical inputs", "",
            "norm_rel / segment-scaled, and the (drone, segment, k) of the worst norm_rel element; `short` is the drone's "
            "shortest segment.", "", "| M | twin | reg | oracle | worst element: twin | reg |", "|---|---|---|---|---|---|"]
    ratios = []
    for M in range(13, 21):
        sel = {r["family"]: r for r in rows if r["order"] == 9 and r["grid"] == "uneven" and r["M"] == M}
        if "twin" not in sel or "reg" not in sel:
            continue
        tw, rg = sel["twin"], sel["reg"]
        ratios.append(max(tw["norm_rel"], rg["norm_rel"]) / min(tw["norm_rel"], rg["norm_rel"]))
        at = lambda r: "drone %d seg %d c_%d (short %d)" % (r["norm_rel_at"][0], r["norm_rel_at"][1], r["norm_rel_at"][3],  # noqa: E731
                                                            r["shortest_seg"][r["norm_rel_at"][0]])
        out.append("| %d | %.2e / %.2e | %.2e / %.2e | %.2e / %.2e | %s | %s |" % (
            M, tw["norm_rel"], tw["seg_scaled"], rg["norm_rel"], rg["seg_scaled"], tw["oracle_norm_rel"],
            tw["oracle_seg_scaled"], at(tw), at(rg)))
    if ratios:
        out += ["", "Largest ratio between the two families on one case: %.2f." % max(ratios)]
    out += ["", "## Order 9, every family, per segment count (norm_rel; even / uneven)", "",
            "| M | twist | twin | reg | generic | oracle |", "|---|---|---|---|---|---|"]
    for M in sorted({r["M"] for r in rows if r["order"] == 9}):
        cells = []
        for fam in ("twist", "twin", "reg", "generic"):
            sel = {r["grid"]: r for r in rows if r["order"] == 9 and r["M"] == M and
                   (r["family"] == fam or (fam == "generic" and r["family"] == "generic-GS"))}
            cells.append("%.1e / %.1e" % (sel["even"]["norm_rel"], sel["uneven"]["norm_rel"]) if "even" in sel else "")
        anyr = {r["grid"]: r for r in rows if r["order"] == 9 and r["M"] == M}
        cells.append("%.1e / %.1e" % (anyr["even"]["oracle_norm_rel"], anyr["uneven"]["oracle_norm_rel"]))
        out.append("| %d | %s |" % (M, " | ".join(cells)))
    print("\n".join(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "solve_accuracy.jsonl"))
