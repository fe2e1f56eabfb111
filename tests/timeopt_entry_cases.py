"""The host entry of a time-allocation mode called without its optional outputs (cost, pg, iters all NULL), against the
mode's device entry: the case the ..._entries_... tests of tests/test_timeopt*_gpu.py share.  Context's host methods
always pass the three optional outputs, so the host entry is called through the library directly; which of its staged
regions reach the launcher, and which stay NULL, is decided per pointer in the one entry body of csrc/msnap_timeopt.hip."""
import ctypes

import numpy as np

W1 = (1.0, 1.0, 1.0, 1.0)


def assert_host_entry_without_optionals_is_the_device_entry(ctx, mode, wp, t, states=(), time_weight=()):
    """`mode`: "", "_states", "_periodic" or "_free", the suffix of msnap_optimize_times; `states`: (start, end) where
    the mode takes them, each an array or None; `time_weight`: (array [n],) where the mode takes one.  t_out, coef, dur
    and status of the two entries must be the same bits, every drone must succeed and some knot must have moved."""
    import torch
    wp, t = np.ascontiguousarray(wp, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)
    n, m, _ = wp.shape
    M = m - 1
    w = np.array(W1)

    def vp(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    host = (np.empty((n, m)), np.empty((n, M, 4, ctx.ncoef)), np.empty((n, M)), np.empty((n,), dtype=np.int32))
    rc = getattr(ctx._lib, "msnap_optimize_times" + mode)(
        ctx._h, n, M, vp(wp), vp(t), 0, *map(vp, states), vp(w), *map(vp, time_weight), 0.1, 200, 1e-4, *map(vp, host),
        None, None, None)
    assert rc == 0, rc
    assert (host[3] == 0).all() and not np.array_equal(host[0], t)

    dev = torch.device("cuda", ctx.device_id)

    def to(a):
        return None if a is None else torch.from_numpy(a).to(dev)

    d_in = (to(wp), to(t), tuple(map(to, states)), tuple(map(to, time_weight)))
    outs = tuple(torch.empty(x.shape, dtype=torch.int32 if x.dtype == np.int32 else torch.float64, device=dev)
                 for x in host)
    torch.cuda.synchronize()
    getattr(ctx, "optimize_times" + mode + "_device")(n, M, d_in[0], d_in[1], 0, *d_in[2], W1, *d_in[3], 0.1, 200, 1e-4,
                                                      *outs)
    ctx.sync()
    for name, a, b in zip(("t_out", "coef", "dur", "status"), host, outs):
        assert np.array_equal(a, b.cpu().numpy()), (mode, name, [x is not None for x in states])
