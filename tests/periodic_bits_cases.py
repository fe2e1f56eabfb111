"""Inputs of tests/golden/periodic_bits.npz, shared by its recorder (tests/golden/make_periodic_bits_golden.py) and
tests/test_periodic_bits_gpu.py: msnap_solve_periodic_device at the smallest shapes that reach every branch of the ring
elimination (csrc/msnap_ring.h), clean and with failed drones injected as tests/test_periodic_gpu.py builds them."""
import os

import numpy as np

import periodic_exact as PE

ST_TIMES, ST_NONFINITE = 2, 3      # MSNAP_ST_* of include/msnap.h
GUARD = 2                          # drone rows behind the batch that a launch must leave alone
BATCHES = ("clean", "nan_waypoint", "flat_time", "raised")
SHARED_BATCHES = ("clean", "nan_waypoint")      # (one time grid for the batch: a bad time would fail every drone)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "periodic_bits.npz")


def _case(order, m, n, shared=False):
    return {"order": order, "m": m, "n": n, "shared": shared}


# two segments (knot 1 is knot M-1: both backward loops run zero trips, the refinement never reads a stashed G), three
# (the first trip of each), four, and the cap (LDS above 64 KiB, the function attribute); 17 drones are a full tile and
# a one-drone tile whose other lanes replay it; shared times once per order
CASES = [_case(o, m, n) for o in (7, 9) for m, n in ((2, 17), (3, 17), (4, 17), (PE.MAX_SEG[o], 3))]
CASES += [_case(o, 3, 17, True) for o in (7, 9)]


def case_id(c):
    return f"o{c['order']}_m{c['m']}_n{c['n']}" + ("_shared" if c["shared"] else "")


def key(c, batch, field):
    return f"{case_id(c)}/{batch}/{field}"


def batches(c):
    return SHARED_BATCHES if c["shared"] else BATCHES


def changed(c, batch):
    """{drone: status} of the drones whose inputs `batch` changes; every other drone must come out as in "clean"."""
    if batch == "clean":
        return {}
    if batch == "nan_waypoint":    # the last waypoint is read too
        return {1: ST_NONFINITE}
    if batch == "flat_time":       # a duration of zero, on the drone that ends the batch (alone in its tile at 17)
        return {c["n"] - 1: ST_TIMES}
    if batch == "raised":          # t[0] = 0.1
        return {0: ST_TIMES}
    raise ValueError(batch)


def expected_status(c, batch):
    st = np.zeros(c["n"], np.int32)
    for d, s in changed(c, batch).items():
        st[d] = s
    return st


def inputs(c, batch):
    """(wp [n, m+1, 4], t [n, m+1] or [m+1]) of one batch; "clean" is periodic_exact.case's own."""
    m, n = c["m"], c["n"]
    wp, t = PE.case(c["order"], m, N=n, kind="shared" if c["shared"] else "offset")
    if batch == "nan_waypoint":
        wp[1, m, 2] = np.nan
    elif batch == "flat_time":
        t[n - 1, m - 1] = t[n - 1, m - 2]
    elif batch == "raised":
        t[0] += 0.1
    elif batch != "clean":
        raise ValueError(batch)
    return wp, t


def solve(ctx, c, wp, t):
    """One launch into sentinel-filled device outputs that are GUARD drones longer than the batch; returns
    (coef, dur, status) of the batch as numpy arrays after checking that the rows behind it kept the sentinel."""
    import torch
    n, m = c["n"], c["m"]
    dev = torch.device("cuda", ctx.device_id)
    dwp, dt = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (wp, t))
    sentinel = np.array([0x7FF8DEADBEEF0001], dtype=np.int64).view(np.float64)[0]
    coef = torch.full((n + GUARD, m, 4, ctx.order + 1), sentinel, dtype=torch.float64, device=dev)
    dur = torch.full((n + GUARD, m), sentinel, dtype=torch.float64, device=dev)
    status = torch.full((n + GUARD,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.solve_periodic_device(n, m, dwp, dt, c["shared"], coef, dur, status)
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
