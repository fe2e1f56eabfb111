#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files instruction for instruction.

    hipcc <the Makefile's flags> --cuda-device-only -S file.hip -o old.s     (at one commit)
    hipcc <the Makefile's flags> --cuda-device-only -S file.hip -o new.s     (at another)
    python tools/kernel_isa_diff.py old.s new.s [--except REGEX]

Labels, comments, directives and blank lines are dropped; what is left of every function is its instruction stream
(branch targets are local labels: they are renumbered in order of first appearance, so that a kernel added or removed
in front does not show up as a difference).  Prints one line per kernel that differs, is missing or is new, and the
totals; exit status 1 if a kernel whose demangled name does not match --except differs.  Also prints, for the kernels
that match --except, the register counts of both files (`.sgpr_count`, `.vgpr_count`, `.agpr_count`, scratch).
"""
from __future__ import annotations

import re
import subprocess
import sys


def functions(path):
    """mangled name -> list of instruction lines"""
    out, cur = {}, None
    for ln in open(path):
        ln = ln.split(";")[0].rstrip()
        if not ln.strip():
            continue
        m = re.match(r"^(_Z\w+):\s*$", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        t = ln.strip()
        if t.startswith(".Lfunc_end") or t.startswith(".size"):      # (.size: the end of a data symbol)
            cur = None
            continue
        if t.startswith(".") or t.endswith(":"):      # directives and local labels
            continue
        out[cur].append(re.sub(r"\s+", " ", t))
    return out


def canonical(body):
    names = {}
    def ren(m):
        return names.setdefault(m.group(0), f".L{len(names)}")
    return [re.sub(r"\.LBB\d+_\d+", ren, ins) for ins in body]


def metadata(path):
    """mangled name -> dict of the register counts in the file's amdhsa.kernels note"""
    out, cur = {}, None
    for ln in open(path):
        if re.match(r"^  - \.", ln):                  # a new entry of the kernel list
            cur = {}
        m = re.match(r"^\s+(?:- )?\.(sgpr_count|sgpr_spill_count|vgpr_count|agpr_count|private_segment_fixed_size):\s+(\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
        m = re.match(r"^\s+(?:- )?\.symbol:\s+(\S+)\.kd", ln)
        if m and cur is not None:
            out[m.group(1)] = cur
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def compare(old, new, skip=None):
    """(number of kernels compared, [(demangled name, what)] that differ outside `skip`, [names matching skip])"""
    fo, fn = functions(old), functions(new)
    dm = demangle(sorted(set(fo) | set(fn)))
    bad, skipped, n = [], [], 0
    for k in sorted(set(fo) | set(fn)):
        if not fo.get(k) and not fn.get(k):         # a data symbol
            continue
        name = dm[k].split("(")[0].replace("void ", "")
        if skip and re.search(skip, name):
            skipped.append(k)
            continue
        n += 1
        if k not in fo or k not in fn:
            bad.append((name, "only in " + (new if k in fn else old)))
        elif canonical(fo[k]) != canonical(fn[k]):
            bad.append((name, f"{len(fo[k])} -> {len(fn[k])} instructions, streams differ"))
    return n, bad, skipped


def main():
    args = sys.argv[1:]
    skip = None
    if "--except" in args:
        i = args.index("--except")
        skip = args[i + 1]
        del args[i:i + 2]
    old, new = args
    n, bad, skipped = compare(old, new, skip)
    for name, what in bad:
        print(f"kernel_isa_diff: {name}: {what}")
    print(f"kernel_isa_diff: {n} functions compared, {len(bad)} differ" + (f", {len(skipped)} excepted" if skip else ""))
    if skipped:
        mo, mn, fo, fn = metadata(old), metadata(new), functions(old), functions(new)
        dm = demangle(skipped)
        for k in skipped:
            a, b = mo.get(k, {}), mn.get(k, {})
            row = ", ".join(f"{f.split('_count')[0].split('_segment')[0]} {a.get(f, '-')} -> {b.get(f, '-')}"
                            for f in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "agpr_count", "private_segment_fixed_size"))
            print(f"    {dm[k].split('(')[0].replace('void ', '')}: instructions {len(fo.get(k, []))} -> {len(fn.get(k, []))}, {row}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
