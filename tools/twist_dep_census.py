#!/usr/bin/env python3
"""Register-dependence census of the small-batch (twisted) solve kernel: where a lone in-order wave has to wait.

A wave that has its SIMD to itself issues in program order, one instruction per issue slot.  An instruction that
reads a vector register written fewer slots earlier than the producer's latency stalls the wave.  This tool reads the
device assembly of one kernel,

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on -mllvm -amdgpu-kernarg-preload-count=16 \
          --cuda-device-only -S msnap_solve.hip -o msnap_solve.s          (the line of profiles/twist_overhead_ab.md)
    python tools/twist_dep_census.py msnap_solve.s [--kernel 'solve_kernel_twist<4, 4, 10, 4>'] [--lat-fma S] ...

cuts it at `s_barrier`, at the first exchange of the merge (`v_mov_b32_dpp`) and at the status store
(`global_store_dword`), and reports per phase
  * how many instructions read a VGPR written 1, 2, .. slots earlier (nearest producer; "at distance d"),
  * the stall slots an in-order issue model implies: instruction i issues at max(issue[i-1] + 1, ready of its vector
    sources), a result is ready `latency` slots after its producer issued.  Latencies in issue slots come from
    tools/micro/dep_latency_micro.hip (profiles/twist_issue_slots_ab.md); everything that is not fp64 arithmetic or a
    reciprocal counts as one slot.
Register dependences only: memory waits (s_waitcnt), the barrier and branches are not modelled, scalar registers are
not tracked.  The out-of-line rare path behind `s_endpgm` is left out.
"""
from __future__ import annotations

import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_isa_diff  # noqa: E402

# measured on MI355X, one wave per SIMD (profiles/twist_issue_slots_ab.md)
LAT_FMA, LAT_MUL, LAT_RCP = 2.0, 2.0, 3.0
CYCLES_PER_SLOT = 4.2          # profiles/twist_overhead_ab.md: one instruction of any kind per ~4.2 shader cycles

NO_DEST = re.compile(r"^(global_store|ds_write|buffer_store|flat_store|scratch_store|s_waitcnt|s_barrier|s_nop|s_endpgm|"
                     r"s_cbranch|s_branch|s_sleep|s_setprio|v_cmpx|s_cmp|s_bitcmp)")
TWO_DEST = re.compile(r"^v_(add_co|sub_co|subrev_co|addc_co|subb_co|subbrev_co|div_scale|mad_u64_u32|mad_i64_i32)")
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def vregs(operand):
    out = set()
    for m in REG.finditer(operand):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def split_ops(ins):
    op, _, rest = ins.partition(" ")
    # operands are comma separated; modifiers (row_shl:4, offset:8, quad_perm:[..]) follow the last one after a space
    ops = [o.strip() for o in re.split(r",(?![^\[]*\])", rest)] if rest else []
    return op, ops


def defs_uses(ins):
    """(set of VGPRs written, set of VGPRs read)"""
    op, ops = split_ops(ins)
    if not ops:
        return set(), set()
    if NO_DEST.match(op):
        return set(), set().union(*[vregs(o) for o in ops])
    nd = 2 if TWO_DEST.match(op) else 1
    d = set().union(*[vregs(o) for o in ops[:nd]])
    u = set().union(*[vregs(o) for o in ops[nd:]]) if len(ops) > nd else set()
    if "_dpp" in op or op.startswith(("v_fmac", "v_mac", "v_writelane")):     # the destination is read as well
        u |= d
    return d, u


def latency(op, lat):
    if op.startswith("v_rcp_f64"):
        return lat["rcp"]
    if op.startswith("v_fma_f64"):
        return lat["fma"]
    if op.startswith(("v_mul_f64", "v_add_f64")):
        return lat["mul"]
    return 1.0


def phases(body):
    """[(name, first, end)] over the in-line part of the kernel"""
    end = next((i for i, s in enumerate(body) if s.startswith("s_endpgm")), len(body) - 1) + 1
    bar = next(i for i, s in enumerate(body) if s.startswith("s_barrier"))
    dpp = next(i for i in range(bar, end) if body[i].startswith("v_mov_b32_dpp"))
    st = next((i for i in range(dpp, end) if body[i].startswith("global_store_dword ")), end)
    return [("head, up to s_barrier", 0, bar + 1), ("sweeps", bar + 1, dpp), ("merge + status", dpp, st),
            ("back-substitution + recovery + stores", st, end)]


def census(body, lat, maxd=4):
    """per phase: instruction count, {distance: instructions whose nearest producer is that many slots in front},
    stall slots of the in-order model"""
    last_def = {}            # vgpr -> (index, ready time)
    t_prev, rows, issue = -1.0, [], []
    info = []
    for i, ins in enumerate(body):
        op, _ = split_ops(ins)
        d, u = defs_uses(ins)
        near = min((i - last_def[r][0] for r in u if r in last_def), default=None)
        ready = max((last_def[r][1] for r in u if r in last_def), default=0.0)
        t = max(t_prev + 1.0, ready)
        info.append((near, t - (t_prev + 1.0)))
        for r in d:
            last_def[r] = (i, t + latency(op, lat))
        t_prev = t
    for name, a, b in phases(body):
        dist = {k: sum(1 for n, _ in info[a:b] if n == k) for k in range(1, maxd + 1)}
        rows.append((name, b - a, dist, sum(s for _, s in info[a:b])))
    return rows


def pick(funcs, want):
    dm = kernel_isa_diff.demangle(sorted(funcs))
    hits = [k for k in funcs if want in dm[k] and funcs[k]]
    if len(hits) != 1:
        sys.exit(f"twist_dep_census: {len(hits)} kernels match {want!r}")
    return hits[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="solve_kernel_twist<4, 4, 10, 4>")
    ap.add_argument("--lat-fma", type=float, default=LAT_FMA)
    ap.add_argument("--lat-mul", type=float, default=LAT_MUL)
    ap.add_argument("--lat-rcp", type=float, default=LAT_RCP)
    args = ap.parse_args()
    funcs = kernel_isa_diff.functions(args.asm)
    body = funcs[pick(funcs, args.kernel)]
    lat = {"fma": args.lat_fma, "mul": args.lat_mul, "rcp": args.lat_rcp}
    print(f"{args.kernel}: latencies in slots fma {lat['fma']:g}, mul/add {lat['mul']:g}, rcp {lat['rcp']:g}")
    print(f"{'phase':40s} {'instr':>6s} {'d=1':>5s} {'d=2':>5s} {'d=3':>5s} {'d=4':>5s} {'stall slots':>12s} {'cycles':>8s}")
    for name, n, dist, stall in census(body, lat):
        print(f"{name:40s} {n:6d} {dist[1]:5d} {dist[2]:5d} {dist[3]:5d} {dist[4]:5d} {stall:12.0f} {stall * CYCLES_PER_SLOT:8.0f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
