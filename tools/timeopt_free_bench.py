#!/usr/bin/env python3
"""Times Context.optimize_times_free_device against Context.optimize_times_states_device in the same process: what a
free total duration costs per launch and per accepted step.  Appends one JSON line per size to
profiles/timeopt_free_bench.jsonl.

    python tools/timeopt_free_bench.py [--reps 7] [--out profiles/timeopt_free_bench.jsonl] [--small]
    python tools/timeopt_free_bench.py --static      (no GPU: registers and instruction counts of the built objects)

Inputs: synthetic.swarm waypoints and times, seeded end states within tests/states_exact.py's scale at both ends, the
time weight k_0 = (2k - 1) J(input times) / t[M] per drone.  The states entry gets the same waypoints and states and
the input knots stretched to the free result's total, so that both allocate comparable paths.  Kernel time as
tools/timeopt_bench.py takes it: events on the stream around the one launch; 3 warm-up calls of each entry, then
`reps` timed calls of each, alternating, and the median.  Per entry the row records ms per launch, the mean accepted
steps, us per accepted step (median ms / mean accepted steps) and the share of drones that met the tolerance.
--static appends a row of kind "static": VGPRs (the code object's metadata) and instruction counts (llvm-objdump) of
the free-total and the end-state instances, from csrc/*.o.  The timed rows need a GPU; there is no fallback."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE_SCALE = (2.0, 2.0, 4.0, 8.0)      # tests/states_exact.py


def static_row():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_isa as chk
    row = {"kind": "static"}
    for obj, mode in (("msnap_timeopt_free.o", "free"), ("msnap_timeopt.o", "states")):
        path = os.path.join(chk.CSRC, obj)
        count = {re.search(r"timeopt_kernel<(\d), (\d)>", k).groups(): len(v)
                 for k, v in chk.kernels_of(chk.disassemble(path)).items() if "timeopt_kernel<" in k}
        with tempfile.TemporaryDirectory() as tmp:
            fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
            subprocess.run([f"{chk.LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", path,
                            os.path.join(tmp, "copy.o")], check=True)
            subprocess.run([f"{chk.LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
            notes = subprocess.run([f"{chk.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True,
                                   check=True).stdout
        regs = {}
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            m = re.search(r"timeopt_kernelILi(\d)ELi(\d)E", name)
            if m:
                regs[m.groups()] = {"vgprs": int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                                    "agprs": int(blk.split()[0]),
                                    "scratch_bytes": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))}
        want = "3" if mode == "free" else "1"
        for (k, m), n in sorted(count.items()):
            if m == want:
                row[f"{mode}_order{2 * int(k) - 1}"] = dict(regs[(k, m)], instructions=n)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeopt_free_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="256 x 10 at order 7 only (a rehearsal)")
    ap.add_argument("--static", action="store_true", help="registers and instruction counts only (no GPU)")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.static:
        row = static_row()
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as out:
            out.write(json.dumps(row) + "\n")
        return
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.synthetic import swarm
    if not torch.cuda.is_available():
        raise SystemExit("timeopt_free_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sizes = [(7, 256, 10)] if args.small else [(7, 256, 10), (7, 4096, 10), (9, 256, 10), (9, 4096, 10)]
    mf, max_iter, tol, w = 0.1, 200, 1e-4, (1, 1, 1, 1)
    with open(args.out, "a") as out:
        for order, N, M in sizes:
            wp, t = swarm(2, N, M)
            nd = (order + 1) // 2 - 1
            rng = np.random.default_rng(1700 + order)
            scale = np.array(STATE_SCALE[:nd])
            start = rng.uniform(-1.0, 1.0, (N, 4, nd)) * scale
            end = rng.uniform(-1.0, 1.0, (N, 4, nd)) * scale
            with Context(device_id=0, order=order, max_segments=64) as ctx:
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                dwp, dt = torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev)
                ds, de = torch.from_numpy(start).to(dev), torch.from_numpy(end).to(dev)
                o_t = torch.empty((N, M + 1), dtype=torch.float64, device=dev)
                o_c = torch.empty((N, M, 4, order + 1), dtype=torch.float64, device=dev)
                o_d = torch.empty((N, M), dtype=torch.float64, device=dev)
                o_s = torch.empty((N,), dtype=torch.int32, device=dev)
                o_j = torch.empty((N, 2), dtype=torch.float64, device=dev)
                o_p = torch.empty((N,), dtype=torch.float64, device=dev)
                o_i = torch.empty((N,), dtype=torch.int32, device=dev)
                outs = (o_t, o_c, o_d, o_s, o_j, o_p, o_i)
                # k_0 from the cost at the input times, then the free result's totals for the states entry's knots
                ctx.optimize_times_states_device(N, M, dwp, dt, 0, ds, de, w, mf, 0, tol, *outs)
                dk = (order * o_j[:, 0] / dt[:, M]).contiguous()
                ctx.optimize_times_free_device(N, M, dwp, dt, 0, ds, de, w, dk, mf, max_iter, tol, *outs)
                total = o_t[:, M].clone()
                dt_states = (dt * (total / dt[:, M])[:, None]).contiguous()
                torch.cuda.synchronize()

                def free():
                    ctx.optimize_times_free_device(N, M, dwp, dt, 0, ds, de, w, dk, mf, max_iter, tol, *outs)

                def states():
                    ctx.optimize_times_states_device(N, M, dwp, dt_states, 0, ds, de, w, mf, max_iter, tol, *outs)

                calls = (("free", free), ("states", states))
                res = {name: {"ms": []} for name, _ in calls}
                for _ in range(3):
                    for _, call in calls:
                        call()
                torch.cuda.synchronize()
                for _ in range(args.reps):
                    for name, call in calls:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call()
                        e1.record()
                        torch.cuda.synchronize()
                        res[name]["ms"].append(e0.elapsed_time(e1))
                        res[name].update(ok=bool((o_s.cpu().numpy() == 0).all()), steps=float(o_i.cpu().numpy().mean()),
                                         converged=float((o_p.cpu().numpy() <= tol).mean()))
            row = {"kind": "timed", "order": order, "n_drones": N, "n_seg": M, "min_fraction": mf, "max_iter": max_iter,
                   "tol": tol, "reps": args.reps, "total_in_mean": float(t[:, M].mean()),
                   "total_free_mean": float(total.cpu().numpy().mean())}
            for name in ("free", "states"):
                r = res[name]
                med = float(np.median(r["ms"]))
                row.update({f"{name}_ms_median": med, f"{name}_ms_min": float(min(r["ms"])),
                            f"{name}_ms_max": float(max(r["ms"])), f"{name}_accepted_steps_mean": r["steps"],
                            f"{name}_us_per_accepted_step": 1e3 * med / r["steps"], f"{name}_share_converged": r["converged"],
                            f"{name}_statuses_ok": r["ok"]})
            row["per_step_free_over_states"] = row["free_us_per_accepted_step"] / row["states_us_per_accepted_step"]
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
