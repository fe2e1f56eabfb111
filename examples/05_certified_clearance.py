#!/usr/bin/env python3
"""Certified drone-vs-drone clearance: a head-on crossing the sampled pass misses, then a formation swarm.

1. Two rest-to-rest drones cross at right angles, 2 m in 1.1 s each, and pass through the same point at t = 0.55 s.
   On the 0.1 s sampling grid they are never closer than 0.28 m: the formation pass reports no hit at radius 0.1.
   msnap_pair_clearance finds the collision in continuous time.
2. swarm.certify_clearance on a 512-drone formation swarm: the samples and the certified speed peaks clear most drones,
   the exact kernel sees the pairs that are left -- listed on the GPU by msnap_formation_near_pairs, which the example
   then calls directly for the same pairs and times.

    python examples/05_certified_clearance.py        (needs an MI355X)
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_path_planning_python_amd import Context, synthetic  # noqa: E402
from drone_path_planning_python_amd.swarm import DeviceCompute, certify_clearance, default_sample_count  # noqa: E402

dev = torch.device("cuda", 0)
with Context(device_id=0, order=7, max_segments=16) as ctx:
    wp = np.zeros((2, 2, 4))
    wp[0, :, 0] = [-1.0, 1.0]
    wp[1, :, 1] = [-1.0, 1.0]
    coef, dur, status = ctx.solve_batch(wp, np.array([0.0, 1.1]))
    S = default_sample_count(1.1, synthetic.SAMPLE_DT)
    pos = ctx.sample(coef, dur, synthetic.SAMPLE_DT, S, 3)
    smd, _, shit = ctx.formation_collide(pos, pos, 0.1)
    md, tm, lower, st = ctx.pair_clearance(coef, dur, np.array([[0, 1]], dtype=np.int32))
    print(f"crossing pair: sampled minimum {smd[0]:.3f} m, hit {bool(shit[0])};  "
          f"certified: min_dist {md[0]:.3e} m at t = {tm[0]:.4f} s, lower bound {lower[0]:.3e} m")

    rb, off, t = synthetic.formation_config(2)
    G, m, _ = rb.shape
    poses = ctx.formation_transform(rb.reshape(G * m, 7), off)
    wp = synthetic.formation_waypoints(poses, G)[:512]
    comp = DeviceCompute(ctx, torch)
    coef, dur, status = comp.solve(torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev))
    res = certify_clearance(comp, coef, dur, synthetic.DRONE_RADIUS, synthetic.SAMPLE_DT,
                            synthetic.formation_sample_count(t), status=status)
    torch.cuda.synchronize()
    print(f"formation swarm, 512 drones: {int(res.cleared_by_sampling.sum())} cleared by sampling, "
          f"{res.n_uncertain} uncertain, {res.pairs.shape[0]} pairs certified exactly;  sampled hits "
          f"{int(res.sampled_hit.sum())}, certified hits {int(res.hit.sum())}, undecided {int(res.undecided.sum())};  "
          f"smallest certified lower bound {float(res.certified_lower.min()):.4f} m")
    # the filter of step 4 on its own: the pairs of the uncertain drones closer than 2 radius + (V_i + V_j) gap
    from drone_path_planning_python_amd.swarm import COMPARE_MARGIN, PEAK_MARGIN  # noqa: E402
    idx = torch.nonzero(~res.cleared_by_sampling, as_tuple=True)[0]
    pos = comp.sample(coef, dur, synthetic.SAMPLE_DT, synthetic.formation_sample_count(t))[idx].contiguous()
    v = (comp.dynamic_peaks(coef, dur)[0][:, 0] * (1.0 + PEAK_MARGIN))[idx].contiguous()
    comp.near_pairs(pos, 2.0 * synthetic.DRONE_RADIUS, v, res.gap, COMPARE_MARGIN)      # (sizes the scratch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pairs, dist = comp.near_pairs(pos, 2.0 * synthetic.DRONE_RADIUS, v, res.gap, COMPARE_MARGIN)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert torch.equal(idx[pairs.to(torch.int64)].to(torch.int32), res.pairs)
    print(f"near pairs among the {idx.numel()} uncertain drones: {pairs.shape[0]} pairs in {ms:.2f} ms "
          f"(closest {float(dist.min()) if pairs.shape[0] else float('nan'):.4f} m)")
    ctx.use_own_stream()
