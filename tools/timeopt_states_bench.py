#!/usr/bin/env python3
"""Times Context.optimize_times_states_device with zero-filled state blocks against Context.optimize_times_device on the
same inputs, in the same process: what the given-end-states form of the kernel (state images in LDS, the seed of the
carried term, the last knot's coupling block in every trial, one refinement step at the end) costs over the
rest-to-rest kernel on a problem both solve.  Appends one JSON line per size to profiles/timeopt_states_bench.jsonl.

    python tools/timeopt_states_bench.py [--reps 7] [--out profiles/timeopt_states_bench.jsonl] [--small]

Kernel time as tools/timeopt_bench.py takes it: events on the stream around the one launch, warm, median of `reps`
calls.  The two entries take the same accepted steps on these inputs (tests/test_timeopt_states_gpu.py holds them to
that on a small batch; the row records both means), so the ratio compares like with like.  Needs a GPU; there is no
fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeopt_states_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="256 x 10 at order 7 only (a rehearsal)")
    args = ap.parse_args()
    import torch
    from drone_path_planning_python_amd import Context
    from drone_path_planning_python_amd.synthetic import swarm
    if not torch.cuda.is_available():
        raise SystemExit("timeopt_states_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sizes = [(7, 256, 10)] if args.small else [(7, 256, 10), (7, 4096, 10), (9, 256, 10), (9, 4096, 10)]
    mf, max_iter, tol = 0.1, 200, 1e-4
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        for order, N, M in sizes:
            wp, t = swarm(2, N, M)
            nd = (order + 1) // 2 - 1
            with Context(device_id=0, order=order, max_segments=64) as ctx:
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                dwp, dt = torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev)
                zero0 = torch.zeros((N, 4, nd), dtype=torch.float64, device=dev)
                zero1 = torch.zeros((N, 4, nd), dtype=torch.float64, device=dev)
                o_t = torch.empty((N, M + 1), dtype=torch.float64, device=dev)
                o_c = torch.empty((N, M, 4, order + 1), dtype=torch.float64, device=dev)
                o_d = torch.empty((N, M), dtype=torch.float64, device=dev)
                o_s = torch.empty((N,), dtype=torch.int32, device=dev)
                o_j = torch.empty((N, 2), dtype=torch.float64, device=dev)
                o_p = torch.empty((N,), dtype=torch.float64, device=dev)
                o_i = torch.empty((N,), dtype=torch.int32, device=dev)
                outs = (o_t, o_c, o_d, o_s, o_j, o_p, o_i)

                def states():
                    ctx.optimize_times_states_device(N, M, dwp, dt, 0, zero0, zero1, (1, 1, 1, 1), mf, max_iter, tol, *outs)

                def rest():
                    ctx.optimize_times_device(N, M, dwp, dt, 0, (1, 1, 1, 1), mf, max_iter, tol, *outs)

                res = {}
                for name, call in (("rest", rest), ("states", states)):
                    call()
                    torch.cuda.synchronize()
                    ms = []
                    for _ in range(args.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call()
                        e1.record()
                        torch.cuda.synchronize()
                        ms.append(e0.elapsed_time(e1))
                    res[name] = {"ms": ms, "ok": bool((o_s.cpu().numpy() == 0).all()),
                                 "steps": float(o_i.cpu().numpy().mean()), "cost": o_j.cpu().numpy()[:, 1].copy()}
            med = {k: float(np.median(v["ms"])) for k, v in res.items()}
            row = {"order": order, "n_drones": N, "n_seg": M, "min_fraction": mf, "max_iter": max_iter, "tol": tol,
                   "reps": args.reps, "states_ms_median": med["states"], "states_ms_min": float(min(res["states"]["ms"])),
                   "states_ms_max": float(max(res["states"]["ms"])), "rest_ms_median": med["rest"],
                   "rest_ms_min": float(min(res["rest"]["ms"])), "rest_ms_max": float(max(res["rest"]["ms"])),
                   "states_over_rest": med["states"] / med["rest"],
                   "statuses_ok": res["states"]["ok"] and res["rest"]["ok"],
                   "accepted_steps_mean_states": res["states"]["steps"], "accepted_steps_mean_rest": res["rest"]["steps"],
                   "cost_rel_diff_max": float(np.max(np.abs(res["states"]["cost"] - res["rest"]["cost"]) /
                                                     res["rest"]["cost"]))}
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
