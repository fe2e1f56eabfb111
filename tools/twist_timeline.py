#!/usr/bin/env python3
"""Phase timeline of the small-batch (twisted) solve kernel on the headline shape.
Needs a library built with -DMSNAP_TOOLS_TIMELINE (MSNAP_LIB_PATH points at it, tools/build_timeline_lib.sh):
every WAVE records s_memrealtime (100 MHz) and s_memtime at 5 points, one row per wave (tile * waves + wave).

    MSNAP_LIB_PATH=$PWD/tools/libmsnap_tl.so python3 tools/twist_timeline.py [waves per tile: 0 (launcher), 1, 2, 4]"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_path_planning_python_amd import Context, _lib  # noqa: E402
from drone_path_planning_python_amd.synthetic import swarm  # noqa: E402

N, M = 256, 10
WAVES = int(sys.argv[1]) if len(sys.argv) > 1 else 0
wp, t = swarm(2, N, M)
dev = torch.device("cuda:0")
dwp, dt = torch.from_numpy(wp).to(dev), torch.from_numpy(t).to(dev)
coef = torch.empty((N, M, 4, 8), dtype=torch.float64, device=dev)
dur = torch.empty((N, M), dtype=torch.float64, device=dev)
st = torch.empty((N,), dtype=torch.int32, device=dev)
lib = _lib.load()
lib.msnap_debug_read_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int]
tiles = (N + 7) // 8
with Context(0, 7, 64) as ctx:
    ctx.set_option("twist_waves", WAVES)
    for _ in range(20):
        ctx.solve_batch_device(N, M, dwp, dt, False, coef, dur, st)
    ctx.sync()
    print(ctx.last_kernel(), " twist_waves option", WAVES)
    buf = np.zeros((1024, 32), dtype=np.uint64)
    assert lib.msnap_debug_read_timeline(buf.ctypes.data_as(ctypes.c_void_p), buf.size) == 0
rows = int((buf[:, 0] != 0).sum())
nw = rows // tiles
assert rows == nw * tiles and nw in (1, 2, 4), (rows, tiles)
buf = buf[:rows]
real = buf[:, 0:10:2].astype(np.int64)
shad = buf[:, 1:10:2].astype(np.int64)
names = ["stage inputs (load + LDS + barrier)", "forward sweep", "status + merge", "backward + recovery + stores"]
print("tiles", tiles, " waves per tile", nw, " start skew between waves: %.2f us" % ((real[:, 0].max() - real[:, 0].min()) / 100.0))
print("kernel span first start -> last end: %.2f us" % ((real[:, 4].max() - real[:, 0].min()) / 100.0))
for w in range(nw):
    r, sh = real[w::nw], shad[w::nw]
    if nw > 1:
        print("wave %d of each tile:" % w)
    for k, nm in enumerate(names):
        d_real = (r[:, k + 1] - r[:, k]) / 100.0
        d_sh = sh[:, k + 1] - sh[:, k]
        print("  %-40s %.2f us (median; min %.2f max %.2f)   %d shader-clock ticks" %
              (nm, np.median(d_real), d_real.min(), d_real.max(), int(np.median(d_sh))))
    print("  per-wave total %.2f us median" % np.median((r[:, 4] - r[:, 0]) / 100.0))
end = real[:, 4].reshape(tiles, nw).max(axis=1) - real[:, 0].reshape(tiles, nw).min(axis=1)
print("per-tile span (first wave start -> last wave end) %.2f us median" % (np.median(end) / 100.0))
