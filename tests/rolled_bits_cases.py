"""Inputs of tests/golden/rolled_bits_*.npz, shared by their recorder (tests/golden/make_rolled_bits_golden.py) and
tests/test_rolled_bits_gpu.py: every instance of the rolled solve -- solve_kernel<K, false> (LDS stash),
solve_kernel<K, true> (global slab) and states_solve_kernel<K> -- at the smallest shapes that reach every branch of the
body they share (csrc/msnap_rolled.h), clean and with failed drones injected."""
import os

import numpy as np

ST_TIMES, ST_NONFINITE = 2, 3      # MSNAP_ST_* of include/msnap.h
GUARD = 2                          # drone rows behind the batch that a launch must leave alone
BATCHES = ("clean", "raised", "faults_a", "faults_b")
SHARED_BATCHES = ("clean", "faults_a")      # (one time grid for the batch: a bad time would fail every drone)
COMBOS = ("start", "end", "both", "neither")


def _case(kind, order, m, n, shared=False, combo="rest"):
    return {"kind": kind, "order": order, "m": m, "n": n, "shared": shared, "combo": combo}


# rest to rest: the LDS stash on a full tile and a one-drone tile, one segment (no knot, no stash), and the first segment
# count of each order whose stash no longer fits LDS; shared times once per kernel
REST = [_case("rest", 7, 25, 17), _case("rest", 9, 21, 17), _case("rest", 7, 1, 5), _case("rest", 9, 1, 5),
        _case("rest", 7, 49, 3), _case("rest", 9, 34, 3), _case("rest", 7, 25, 17, True), _case("rest", 9, 34, 3, True)]
# boundary states: one segment, one knot that takes both end terms, two knots, and the entry's segment limit
STATES = [_case("states", o, m, n, False, c)
          for o, lim in ((7, 47), (9, 32)) for m, n in ((1, 17), (2, 17), (3, 17), (lim, 3)) for c in COMBOS]
STATES += [_case("states", 7, 3, 17, True, c) for c in COMBOS]
CASES = REST + STATES


def case_id(c):
    return f"{c['kind']}_o{c['order']}_m{c['m']}_n{c['n']}" + ("_shared" if c["shared"] else "") + f"_{c['combo']}"


def key(c, batch, field):
    return f"{case_id(c)}/{batch}/{field}"


def golden_path(c):
    """One archive per kernel, the boundary-state one per order as well: each stays below the largest fixture."""
    name = "rolled_bits_rest.npz" if c["kind"] == "rest" else f"rolled_bits_states_o{c['order']}.npz"
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)


def batches(c):
    return SHARED_BATCHES if c["shared"] else BATCHES


def kernel_name(c):
    """msnap_last_kernel after the launch (the boundary-state entry does not note its kernel)."""
    if c["kind"] != "rest":
        return None
    slab = c["m"] >= (49 if c["order"] == 7 else 34)
    return f"msnap::solve_kernel<{(c['order'] + 1) // 2}, {'true' if slab else 'false'}>"


def changed(c, batch):
    """{drone: status} of the drones whose inputs `batch` changes; every other drone must come out as in "clean"."""
    n, states = c["n"], c["kind"] == "states"
    if batch == "clean":
        return {}
    if batch == "raised":          # t[0] = 0.25: the Taylor shift of a healthy rest-to-rest path, refused with end states
        return {d: (ST_TIMES if states else 0) for d in {2, n - 1}}
    if batch == "faults_a":        # a NaN waypoint; a segment that runs backwards (shared times: an infinite waypoint)
        return {1: ST_NONFINITE, n - 1: ST_NONFINITE if c["shared"] else ST_TIMES}
    if batch == "faults_b":        # an infinite time; t[0] < 0 (rest to rest) or a non-finite state entry
        return {0: ST_NONFINITE, n - 2: ST_NONFINITE if states else ST_TIMES}
    raise ValueError(batch)


def expected_status(c, batch):
    st = np.zeros(c["n"], np.int32)
    for d, s in changed(c, batch).items():
        st[d] = s
    return st


def inputs(c, batch):
    """(wp [n, m+1, 4], t [n, m+1] or [m+1], start, end [n, 4, K-1] or None) of one batch; "clean" is synthetic.swarm's
    own with seeded end states."""
    from drone_path_planning_python_amd.synthetic import swarm
    order, m, n = c["order"], c["m"], c["n"]
    wp, t = swarm(5300 + 31 * m + order, n, m, shared_times=c["shared"])
    start = end = None
    if c["kind"] == "states":
        nu = (order + 1) // 2 - 1
        rng = np.random.default_rng(7700 + 31 * m + order)
        scale = np.array((2.0, 2.0, 4.0, 8.0)[:nu])
        both = rng.uniform(-1.0, 1.0, (2, n, 4, nu)) * scale
        start = both[0] if c["combo"] in ("start", "both") else None
        end = both[1] if c["combo"] in ("end", "both") else None
    if batch == "raised":
        for d in changed(c, batch):
            t[d] += 0.25
    elif batch == "faults_a":
        wp[1, m // 2, 1] = np.nan
        if c["shared"]:
            wp[n - 1, m, 3] = np.inf
        else:
            j = max(m - 2, 0)
            t[n - 1, j + 1] = t[n - 1, j] - 0.125
    elif batch == "faults_b":
        t[0, m] = np.inf
        if c["kind"] == "rest":
            t[n - 2] -= 0.5 + t[n - 2, 0]           # t[0] = -0.5
        elif start is not None:
            start[n - 2, 2, 1] = np.nan
        elif end is not None:
            end[n - 2, 0, 0] = np.inf
        else:
            wp[n - 2, 0, 3] = np.inf                # (no state given: the start waypoint instead)
    elif batch != "clean":
        raise ValueError(batch)
    return wp, t, start, end


def solve(ctx, c, wp, t, start, end):
    """One launch into sentinel-filled device outputs that are GUARD drones longer than the batch; returns
    (coef, dur, status) of the batch as numpy arrays after checking that the rows behind it kept the sentinel."""
    import torch
    n, m = c["n"], c["m"]
    dev = torch.device("cuda", ctx.device_id)
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    dwp, dt, ds, de = up(wp), up(t), up(start), up(end)
    sentinel = np.array([0x7FF8DEADBEEF0001], dtype=np.int64).view(np.float64)[0]
    coef = torch.full((n + GUARD, m, 4, ctx.order + 1), sentinel, dtype=torch.float64, device=dev)
    dur = torch.full((n + GUARD, m), sentinel, dtype=torch.float64, device=dev)
    status = torch.full((n + GUARD,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    if c["kind"] == "rest":
        ctx.solve_batch_device(n, m, dwp, dt, c["shared"], coef, dur, status)
        assert ctx.last_kernel() == kernel_name(c), ctx.last_kernel()
    else:
        ctx.solve_states_device(n, m, dwp, dt, c["shared"], ds, de, coef, dur, status)
    ctx.sync()
    coef, dur, status = coef.cpu().numpy(), dur.cpu().numpy(), status.cpu().numpy()
    want = np.array([sentinel]).view(np.int64)[0]
    assert (coef[n:].view(np.int64) == want).all() and (dur[n:].view(np.int64) == want).all(), "written past the batch"
    assert (status[n:] == -7).all(), "status written past the batch"
    return coef[:n], dur[:n], status[:n]


def check(c, batch, coef, dur, status, clean_coef):
    """What keeps the archive from hiding a failure: the expected status words, finite coefficients for every healthy
    drone and NaN for every failed one, and the untouched drones bit for bit as in the clean batch."""
    want = expected_status(c, batch)
    assert np.array_equal(status, want), (case_id(c), batch, status.tolist())
    assert np.isfinite(coef[want == 0]).all(), (case_id(c), batch)
    assert np.isnan(coef[want != 0]).all(), (case_id(c), batch)
    same = [d for d in range(c["n"]) if d not in changed(c, batch)]
    assert np.array_equal(coef[same].view(np.int64), clean_coef[same].view(np.int64)), (case_id(c), batch)
