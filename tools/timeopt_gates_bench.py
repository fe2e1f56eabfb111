#!/usr/bin/env python3
"""Times Context.optimize_times_gates_device against Context.optimize_times_states_device in the same process: what
the gates mode costs per launch with no gate set, and per accepted step with gates.  Appends one JSON line per size to
profiles/timeopt_gates_bench.jsonl.

    python tools/timeopt_gates_bench.py [--reps 7] [--out profiles/timeopt_gates_bench.jsonl] [--small]

Inputs: synthetic.swarm waypoints and times, seeded end states within tests/states_exact.py's scale at both ends; the
same arrays for both entries.  Two gate settings per size:
  * "empty": fix all zero, via all NaN.  The iteration is the states entry's bit for bit (the same trial count), so the
    wall times compare directly: the ratio is what the mask and value fetches and the per-knot ballot cost.
  * "velocity": a velocity gate of up to 2 m/s per axis at every second interior knot (1, 3, ..).  The problem differs
    from the ungated one and so do the trip counts, so the comparison is time per accepted step.
Kernel time as tools/timeopt_free_bench.py takes it: events on the stream around the one launch; 3 warm-up calls of
each entry, then `reps` timed calls of each, alternating, and the median.  The rows need a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATE_SCALE = (2.0, 2.0, 4.0, 8.0)      # tests/states_exact.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeopt_gates_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="256 x 10 at order 7 only (a rehearsal)")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.synthetic import swarm
    if not torch.cuda.is_available():
        raise SystemExit("timeopt_gates_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sizes = [(7, 256, 10)] if args.small else [(7, 256, 10), (7, 4096, 10), (9, 256, 10), (9, 4096, 10)]
    mf, max_iter, tol, w = 0.1, 200, 1e-4, (1, 1, 1, 1)
    with open(args.out, "a") as out:
        for order, N, M in sizes:
            wp, t = swarm(2, N, M)
            nd = (order + 1) // 2 - 1
            rng = np.random.default_rng(2200 + order)
            scale = np.array(STATE_SCALE[:nd])
            start = rng.uniform(-1.0, 1.0, (N, 4, nd)) * scale
            end = rng.uniform(-1.0, 1.0, (N, 4, nd)) * scale
            fix0 = np.zeros((N, M - 1), dtype=np.int32)
            via0 = np.full((N, M - 1, 4, nd), np.nan)
            fix1, via1 = fix0.copy(), via0.copy()
            fix1[:, 0::2] = 1
            via1[:, 0::2, :, 0] = rng.uniform(-2.0, 2.0, (N, len(range(0, M - 1, 2)), 4))
            with Context(device_id=0, order=order, max_segments=64) as ctx:
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                to = lambda x: torch.from_numpy(x).to(dev)      # noqa: E731
                dwp, dt, ds, de = to(wp), to(t), to(start), to(end)
                gates = {"empty": (to(fix0), to(via0)), "velocity": (to(fix1), to(via1))}
                o_t = torch.empty((N, M + 1), dtype=torch.float64, device=dev)
                o_c = torch.empty((N, M, 4, order + 1), dtype=torch.float64, device=dev)
                o_d = torch.empty((N, M), dtype=torch.float64, device=dev)
                o_s = torch.empty((N,), dtype=torch.int32, device=dev)
                o_j = torch.empty((N, 2), dtype=torch.float64, device=dev)
                o_p = torch.empty((N,), dtype=torch.float64, device=dev)
                o_i = torch.empty((N,), dtype=torch.int32, device=dev)
                outs = (o_t, o_c, o_d, o_s, o_j, o_p, o_i)

                def states():
                    ctx.optimize_times_states_device(N, M, dwp, dt, 0, ds, de, w, mf, max_iter, tol, *outs)

                def gated(which):
                    f, v = gates[which]
                    return lambda: ctx.optimize_times_gates_device(N, M, dwp, dt, 0, ds, de, f, v, w, mf, max_iter, tol,
                                                                   *outs)

                calls = (("states", states), ("empty", gated("empty")), ("velocity", gated("velocity")))
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
                                         converged=float((o_p.cpu().numpy() <= tol).mean()),
                                         t_out=o_t.cpu().numpy().copy())
            row = {"kind": "timed", "order": order, "n_drones": N, "n_seg": M, "min_fraction": mf, "max_iter": max_iter,
                   "tol": tol, "reps": args.reps,
                   "empty_is_states_bit_for_bit": bool(np.array_equal(res["empty"]["t_out"], res["states"]["t_out"]))}
            for name in ("states", "empty", "velocity"):
                r = res[name]
                med = float(np.median(r["ms"]))
                row.update({f"{name}_ms_median": med, f"{name}_ms_min": float(min(r["ms"])),
                            f"{name}_ms_max": float(max(r["ms"])), f"{name}_accepted_steps_mean": r["steps"],
                            f"{name}_us_per_accepted_step": 1e3 * med / r["steps"], f"{name}_share_converged": r["converged"],
                            f"{name}_statuses_ok": r["ok"]})
            row["wall_empty_over_states"] = row["empty_ms_median"] / row["states_ms_median"]
            row["per_step_velocity_over_states"] = row["velocity_us_per_accepted_step"] / row["states_us_per_accepted_step"]
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
