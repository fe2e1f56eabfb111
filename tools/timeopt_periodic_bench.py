#!/usr/bin/env python3
"""Times Context.optimize_times_periodic_device against Context.optimize_times_states_device on the same waypoints, the
loop's own seam state (msnap_solve_periodic at the input times, msnap_eval_state at 0) given at both ends: what the ring
elimination in every trial (the seam coupling H, the backward pass over matrices, the seam block) costs over the open
chain's trial.  Appends one JSON line per size to profiles/timeopt_periodic_bench.jsonl.

    python tools/timeopt_periodic_bench.py [--reps 7] [--out profiles/timeopt_periodic_bench.jsonl] [--small]

Kernel time as tools/timeopt_states_bench.py takes it: events on the stream around the one launch, 3 warm-up calls, then
`reps` timed calls of each entry in turn (periodic, states, periodic, ..), the median of each.  The two problems are not
the same problem -- the open chain keeps the seam state the loop had at the INPUT times -- so they take different
numbers of steps; the row therefore records the accepted steps of both (mean and largest) and the time per step of the
slowest drone, which is what a launch waits for: a wave runs until its last drone is done and at these sizes no CU
holds more than a few tiles.  The entries do not report rejected trials; under the doubling / halving rule a run makes
about two trials per accepted step (tests/golden/make_timeopt_periodic_golden.py records solves4 and iters4), for both
entries alike, so the ratio of the times per step is the ratio of the times per trial.  Needs a GPU; there is no
fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def loops(n, m, seed):
    """Random loops as tests/periodic_exact.py::case draws them: durations U(0.5, 2), waypoint steps in [-2, 2]"""
    rng = np.random.default_rng(seed)
    t = np.concatenate([np.zeros((n, 1)), np.cumsum(rng.uniform(0.5, 2.0, (n, m)), axis=1)], axis=1)
    return np.cumsum(rng.uniform(-2.0, 2.0, (n, m + 1, 4)), axis=1), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeopt_periodic_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="256 x 10 at order 7 only (a rehearsal)")
    args = ap.parse_args()
    import torch
    from drone_path_planning_python_amd import Context
    if not torch.cuda.is_available():
        raise SystemExit("timeopt_periodic_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sizes = [(7, 256, 10)] if args.small else [(7, 256, 10), (7, 4096, 10), (9, 256, 10), (9, 4096, 10)]
    mf, max_iter, tol = 0.1, 500, 1e-4
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        for order, N, M in sizes:
            wp, t = loops(N, M, 160000 + order)
            nd = (order + 1) // 2 - 1
            with Context(device_id=0, order=order, max_segments=64) as ctx:
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                dwp, dt = torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev)
                o_t = torch.empty((N, M + 1), dtype=torch.float64, device=dev)
                o_c = torch.empty((N, M, 4, order + 1), dtype=torch.float64, device=dev)
                o_d = torch.empty((N, M), dtype=torch.float64, device=dev)
                o_s = torch.empty((N,), dtype=torch.int32, device=dev)
                o_j = torch.empty((N, 2), dtype=torch.float64, device=dev)
                o_p = torch.empty((N,), dtype=torch.float64, device=dev)
                o_i = torch.empty((N,), dtype=torch.int32, device=dev)
                outs = (o_t, o_c, o_d, o_s, o_j, o_p, o_i)
                # the loop's own seam state at the input times
                ctx.solve_periodic_device(N, M, dwp, dt, 0, o_c, o_d, o_s)
                pos = torch.empty((N, 4), dtype=torch.float64, device=dev)
                seam = torch.empty((N, 4, nd), dtype=torch.float64, device=dev)
                ctx.eval_state_device(N, M, o_c, o_d, torch.zeros((N,), dtype=torch.float64, device=dev), pos, seam)
                torch.cuda.synchronize()
                assert bool((o_s == 0).all())
                seam_end = seam.clone()

                def periodic():
                    ctx.optimize_times_periodic_device(N, M, dwp, dt, 0, (1, 1, 1, 1), mf, max_iter, tol, *outs)

                def states():
                    ctx.optimize_times_states_device(N, M, dwp, dt, 0, seam, seam_end, (1, 1, 1, 1), mf, max_iter, tol,
                                                     *outs)

                calls = {"periodic": periodic, "states": states}
                res = {k: {"ms": []} for k in calls}
                for _ in range(3):
                    for call in calls.values():
                        call()
                torch.cuda.synchronize()
                for _ in range(args.reps):
                    for name, call in calls.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call()
                        e1.record()
                        torch.cuda.synchronize()
                        res[name]["ms"].append(e0.elapsed_time(e1))
                        it = o_i.cpu().numpy()
                        res[name].update(ok=bool((o_s.cpu().numpy() == 0).all()), steps_mean=float(it.mean()),
                                         steps_max=int(it.max()),
                                         conv=float((o_p.cpu().numpy() <= tol).mean()),
                                         gain=float(np.median(o_j.cpu().numpy()[:, 1] / o_j.cpu().numpy()[:, 0])))
            row = {"order": order, "n_drones": N, "n_seg": M, "min_fraction": mf, "max_iter": max_iter, "tol": tol,
                   "reps": args.reps, "statuses_ok": res["periodic"]["ok"] and res["states"]["ok"]}
            for k, r in res.items():
                med = float(np.median(r["ms"]))
                row.update({f"{k}_ms_median": med, f"{k}_ms_min": float(min(r["ms"])), f"{k}_ms_max": float(max(r["ms"])),
                            f"{k}_accepted_steps_mean": r["steps_mean"], f"{k}_accepted_steps_max": r["steps_max"],
                            f"{k}_converged_fraction": r["conv"], f"{k}_median_cost_ratio": r["gain"],
                            f"{k}_us_per_step_of_slowest_drone": 1e3 * med / max(r["steps_max"], 1)})
            row["periodic_over_states_ms"] = row["periodic_ms_median"] / row["states_ms_median"]
            row["periodic_over_states_per_step"] = (row["periodic_us_per_step_of_slowest_drone"] /
                                                    row["states_us_per_step_of_slowest_drone"])
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
