"""Sharding a swarm over the GPUs of one node (one process per GPU).

The solve needs no communication: drones are split into contiguous blocks, one
per rank.  The formation (drone-vs-drone) pass exchanges twice: every rank samples
its own shard and the sampled positions are all-gathered (RCCL over xGMI when the
process group is "nccl"; "gloo" on CPU for the tests); then the swarm's unordered
pairs -- one triangular line of (row block, column) units -- are split into `world`
equal contiguous parts, rank r evaluates part r (every pair on exactly ONE rank,
both drones credited), the per-drone partial minima (12 bytes per drone and rank)
are all-gathered and every rank folds them for the rows it owns.  The mesh sweep
replicates the (tiny) mesh and shards the drones; it depends on the rank's own
samples only, so with a second context (`side_ctx`) it runs on a side stream next
to the exchanges and the pairwise pass.

torch / torch.distributed are plumbing here (device memory + the collective);
all arithmetic happens in libmsnap through the `compute` object, by default a
`DeviceCompute` around a Context.  The CPU tests plug in a stand-in with the
same three methods to exercise the exchange logic under gloo.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np


@functools.lru_cache(maxsize=None)
def _output_names(method: str) -> tuple:
    """The names DeviceCompute._out keys a method's outputs by -- "<method>.coef", .dur, .status and, for an allocator,
    .t_out, .cost, .pg, .iters -- built once per method: the same string objects on every call keep their hash."""
    return tuple(f"{method}.{x}" for x in ("coef", "dur", "status", "t_out", "cost", "pg", "iters"))


def shard_bounds(n: int, world: int, rank: int) -> tuple:
    """Contiguous block partition: the first n % world ranks get one extra drone."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError("bad world/rank")
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    hi = lo + base + (1 if rank < extra else 0)
    return lo, hi


def shard_sizes(n: int, world: int) -> list:
    return [shard_bounds(n, world, r)[1] - shard_bounds(n, world, r)[0] for r in range(world)]


class DeviceCompute:
    """The device operations of the formation pipeline, on torch CUDA tensors.

    `side_ctx`: a second Context on the same device.  When given, `mesh_begin` launches the mesh sweep
    on a side stream (ordered after what the main stream holds at that moment) and `mesh_end` makes the
    main stream wait for it: the sweep overlaps the all-gather and the pairwise pass, whose launch ends
    with SIMDs running out of shares."""

    _reuse = None      # (class default: no output reuse)

    def __init__(self, ctx, torch_module, side_ctx=None, reuse_outputs=False):
        """`reuse_outputs`: every method hands back the SAME output tensors on each call with the same shapes (valid
        until its next call) instead of allocating new ones -- for a loop that consumes a pass's results before it
        starts the next: eleven `torch.empty` per formation pipeline are ~30 us of host time, as much as the host has
        to spare beside 80 us of kernels."""
        self.ctx = ctx
        self.torch = torch_module
        self._reuse = {} if reuse_outputs else None
        self.device = torch_module.device("cuda", ctx.device_id)
        # run on torch's current stream so the collective and the kernels order naturally
        self.main = torch_module.cuda.current_stream(self.device)
        ctx.set_stream(self.main.cuda_stream)
        self.side_ctx = side_ctx
        self.side = None
        if side_ctx is not None:
            if side_ctx.device_id != ctx.device_id:
                raise ValueError("side_ctx must live on the same device")
            # the side context's own stream at the lowest priority: the sweep's workgroups are dispatched
            # when the main stream's kernels have none waiting, i.e. into the end of the pairwise launch
            side_ctx.set_option("own_stream_priority", 1)
            # ... and as a grid of 12 waves per CU that walks the drones: one workgroup per drone holds every wave slot
            # of the chip for the sweep's whole run, and the main stream's next kernel waits for its end
            if side_ctx.get_option("mesh_waves_per_cu") == 0:
                side_ctx.set_option("mesh_waves_per_cu", 12)
            side_ctx.use_own_stream()
            self.side = torch_module.cuda.ExternalStream(side_ctx.stream(), device=self.device)
        self._mesh_pending = None
        self._whole_ok = {}      # (n_total, n_samples, world) -> {"ok": the whole-swarm pass pays, "since": passes since decided}

    def _out(self, name, shape, dtype):
        if self._reuse is None:
            return self.torch.empty(shape, dtype=dtype, device=self.device)
        key = (name, tuple(shape), dtype)
        buf = self._reuse.get(key)
        if buf is None:
            buf = self._reuse[key] = self.torch.empty(shape, dtype=dtype, device=self.device)
        return buf

    def solve(self, wp, t):
        torch = self.torch
        n, m, _ = wp.shape
        M = m - 1
        coef = self._out("solve.coef", (n, M, 4, self.ctx.ncoef), torch.float64)
        dur = self._out("solve.dur", (n, M), torch.float64)
        status = self._out("solve.status", (n,), torch.int32)
        if n:
            self.ctx.solve_batch_device(n, M, wp, t, t.dim() == 1, coef, dur, status)
        return coef, dur, status

    def solve_grid(self, wp):
        """The same solve on the shared time grid the context was prepared for (`Context.prepare_grid`): one
        fp64 MFMA GEMM against the grid's operator instead of the per-drone recurrence."""
        torch = self.torch
        n, m, _ = wp.shape
        M = m - 1
        # (the library refuses a segment count that is not the prepared grid's; the tensor's shape is checked here)
        if wp.dim() != 3 or wp.shape[2] != 4 or m != self.ctx.grid_waypoints():
            raise ValueError(f"solve_grid: wp must be [n, {self.ctx.grid_waypoints()}, 4] for the prepared grid, got {tuple(wp.shape)}")
        coef = self._out("solve_grid.coef", (n, M, 4, self.ctx.ncoef), torch.float64)
        dur = self._out("solve_grid.dur", (n, M), torch.float64)
        status = self._out("solve_grid.status", (n,), torch.int32)
        if n:
            self.ctx.solve_grid_device(n, M, wp, coef, dur, status)
        return coef, dur, status

    def sample(self, coef, dur, dt, n_samples):
        torch = self.torch
        n, M = dur.shape
        pos = self._out("sample.pos", (n, n_samples, 3), torch.float64)
        if n:
            self.ctx.sample_device(n, M, coef, dur, dt, n_samples, 3, pos)
        return pos

    def sample_rows_t(self, coef, dur, dt, n_samples, n_cols=None):
        """(pos [n, S, 3], pos_t): the sampler's second output is what the pairwise pass over these drones would
        otherwise compute in a launch of its own -- the transposed row image [S][3][pitch], or (a whole swarm behind the
        exact broad phase) the drones' path boxes and sort keys; `collide(..., rows_t=pos_t)` hands it over.  With
        `n_cols` (the columns these rows, as a shard at offset 0, will meet) the library is asked first whether that
        pass reads a hand-over at all (paths shorter than 6 samples do not), and pos_t is None if not."""
        torch = self.torch
        n, M = dur.shape
        if n_cols is not None and not self.ctx.collide_reads_rows_t(n, 0, n_cols, n_samples):
            return self.sample(coef, dur, dt, n_samples), None
        pos = self._out("sample_rows_t.pos", (n, n_samples, 3), torch.float64)
        pos_t = self._out("sample_rows_t.pos_t", (self.ctx.collide_rows_t_doubles(n, n_samples),), torch.float64)
        if n:
            self.ctx.sample_collide_device(n, M, coef, dur, dt, n_samples, pos, pos_t)
        return pos, pos_t

    def solve_grid_sample(self, wp, dt, n_samples, n_cols=None):
        """solve_grid and the sampler as one launch (msnap_solve_grid_sample_device): (coef, dur, status, pos, pos_t),
        the same tensors, bit for bit, as `solve_grid` followed by `sample_rows_t` (pos_t is None where that would
        return None, or when `n_cols` is None and no hand-over is wanted)."""
        torch = self.torch
        n, m, _ = wp.shape
        M = m - 1
        if wp.dim() != 3 or wp.shape[2] != 4 or m != self.ctx.grid_waypoints():
            raise ValueError(f"solve_grid_sample: wp must be [n, {self.ctx.grid_waypoints()}, 4] for the prepared grid, got {tuple(wp.shape)}")
        coef = self._out("solve_grid_sample.coef", (n, M, 4, self.ctx.ncoef), torch.float64)
        dur = self._out("solve_grid_sample.dur", (n, M), torch.float64)
        status = self._out("solve_grid_sample.status", (n,), torch.int32)
        pos = self._out("solve_grid_sample.pos", (n, n_samples, 3), torch.float64)
        pos_t = None
        if n_cols is not None and self.ctx.collide_reads_rows_t(n, 0, n_cols, n_samples):
            pos_t = self._out("solve_grid_sample.pos_t", (self.ctx.collide_rows_t_doubles(n, n_samples),), torch.float64)
        if n:
            self.ctx.solve_grid_sample_device(n, M, wp, dt, n_samples, coef, dur, status, pos, pos_t)
        return coef, dur, status, pos, pos_t

    # ---- dynamic limits (include/msnap.h) --------------------------------------------------------------------------
    def dynamic_peaks(self, coef, dur):
        """(peak [n, 4], t_peak [n, 4], status [n] int32): certified speed, acceleration, jerk and yaw-rate peaks."""
        torch = self.torch
        n, M = dur.shape
        peak = self._out("dynamic_peaks.peak", (n, 4), torch.float64)
        t_peak = self._out("dynamic_peaks.t_peak", (n, 4), torch.float64)
        status = self._out("dynamic_peaks.status", (n,), torch.int32)
        if n:
            self.ctx.dynamic_peaks_device(n, M, coef, dur, peak, t_peak, status)
        return peak, t_peak, status

    def retime_to_limits(self, coef, dur, limits, fit=False, common=False):
        """(coef, dur, scale [n]): the drones run uniformly slower (or, with `fit`, faster) so that the limits
        (speed, acceleration, jerk, yaw rate; 0 = none) hold; `common`: one scale for the batch."""
        torch = self.torch
        n, M = dur.shape
        coef_out = self._out("retime.coef", tuple(coef.shape), torch.float64)
        dur_out = self._out("retime.dur", (n, M), torch.float64)
        scale = self._out("retime.scale", (n,), torch.float64)
        flags = self.ctx.retime_flags(fit, common)
        if n:
            self.ctx.retime_to_limits_device(n, M, coef, dur, limits, flags, coef_out, dur_out, scale)
        return coef_out, dur_out, scale

    def time_scale(self, coef, dur, scale):
        """(coef, dur) of the drones run `scale[d]` times slower (a scale that is not finite and > 0 copies)."""
        torch = self.torch
        n, M = dur.shape
        coef_out = self._out("time_scale.coef", tuple(coef.shape), torch.float64)
        dur_out = self._out("time_scale.dur", (n, M), torch.float64)
        if n:
            self.ctx.time_scale_device(n, M, coef, dur, scale, coef_out, dur_out)
        return coef_out, dur_out

    # ---- pairwise clearance in continuous time (include/msnap.h) -----------------------------------------------------
    def pair_clearance(self, coef, dur, pairs):
        """(min_dist [P], t_min [P], lower [P], status [P] int32) of the listed pairs (int32 [P, 2], drone indices into
        the batch): the certified distance while both fly, lower <= infimum <= min_dist."""
        torch = self.torch
        n, M = dur.shape
        P = pairs.shape[0]
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32:
            raise ValueError("pair_clearance: pairs must be an int32 tensor [P, 2]")
        md = self._out("pair_clearance.md", (P,), torch.float64)
        tm = self._out("pair_clearance.tm", (P,), torch.float64)
        lower = self._out("pair_clearance.lower", (P,), torch.float64)
        status = self._out("pair_clearance.status", (P,), torch.int32)
        if P:
            self.ctx.pair_clearance_device(n, M, coef, dur, P, pairs.contiguous(), md, tm, lower, status)
        return md, tm, lower, status

    # ---- cross clearance: two path sets on shifted clocks (include/msnap.h) ------------------------------------------
    def cross_clearance(self, coef_a, dur_a, coef_b, dur_b, pairs, t0_a=None, t0_b=None):
        """(min_dist [P], t_min [P], lower [P], status [P] int32) of the listed pairs (int32 [P, 2]: index in set A,
        index in set B), drone a flying P_a(t - t0_a[a]) on the common clock; t0_a [Na] / t0_b [Nb] float64 or None
        (zeros).  The sets have their own segment counts."""
        torch = self.torch
        (na, Ma), (nb, Mb) = dur_a.shape, dur_b.shape
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32:
            raise ValueError("cross_clearance: pairs must be an int32 tensor [P, 2]")
        for name, x, n in (("t0_a", t0_a, na), ("t0_b", t0_b, nb)):
            if x is not None and (tuple(x.shape) != (n,) or x.dtype != torch.float64):
                raise ValueError(f"cross_clearance: {name} must be a float64 tensor [{n}]")
        P = pairs.shape[0]
        md = self._out("cross_clearance.md", (P,), torch.float64)
        tm = self._out("cross_clearance.tm", (P,), torch.float64)
        lower = self._out("cross_clearance.lower", (P,), torch.float64)
        status = self._out("cross_clearance.status", (P,), torch.int32)
        if P:
            self.ctx.cross_clearance_device(na, Ma, coef_a.contiguous(), dur_a.contiguous(),
                                            None if t0_a is None else t0_a.contiguous(), nb, Mb, coef_b.contiguous(),
                                            dur_b.contiguous(), None if t0_b is None else t0_b.contiguous(), P,
                                            pairs.contiguous(), md, tm, lower, status)
        return md, tm, lower, status

    # ---- conflict windows: from when until when a pair is too close (include/msnap.h) -------------------------------
    _WINDOW_OUTPUTS = ("t_clear_until", "t_first", "d_first", "t_last", "d_last", "t_clear_from")

    def _window_out(self, name, P):
        torch = self.torch
        return ([self._out(f"{name}.{k}", (P,), torch.float64) for k in self._WINDOW_OUTPUTS]
                + [self._out(f"{name}.status", (P,), torch.int32)])

    def conflict_window(self, coef, dur, pairs, threshold, t_res=1e-6):
        """(t_clear_until, t_first, d_first, t_last, d_last, t_clear_from, status int32), each [P], of the listed pairs
        (int32 [P, 2], drone indices into the batch): from when until when the pair is closer than `threshold`, the
        crossings located to `t_res` seconds (msnap_pair_conflict_window_device)."""
        torch = self.torch
        n, M = dur.shape
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32:
            raise ValueError("conflict_window: pairs must be an int32 tensor [P, 2]")
        P = pairs.shape[0]
        outs = self._window_out("conflict_window", P)
        if P:
            self.ctx.pair_conflict_window_device(n, M, coef, dur, P, pairs.contiguous(), threshold, t_res, *outs)
        return tuple(outs)

    def cross_conflict_window(self, coef_a, dur_a, coef_b, dur_b, pairs, threshold, t_res=1e-6, t0_a=None, t0_b=None):
        """conflict_window of drone a of set A against drone b of set B (int32 [P, 2]: index in A, index in B) on
        shifted clocks, as cross_clearance; the times are on the common clock."""
        torch = self.torch
        (na, Ma), (nb, Mb) = dur_a.shape, dur_b.shape
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32:
            raise ValueError("cross_conflict_window: pairs must be an int32 tensor [P, 2]")
        for name, x, n in (("t0_a", t0_a, na), ("t0_b", t0_b, nb)):
            if x is not None and (tuple(x.shape) != (n,) or x.dtype != torch.float64):
                raise ValueError(f"cross_conflict_window: {name} must be a float64 tensor [{n}]")
        P = pairs.shape[0]
        outs = self._window_out("cross_conflict_window", P)
        if P:
            self.ctx.cross_conflict_window_device(na, Ma, coef_a.contiguous(), dur_a.contiguous(),
                                                  None if t0_a is None else t0_a.contiguous(), nb, Mb,
                                                  coef_b.contiguous(), dur_b.contiguous(),
                                                  None if t0_b is None else t0_b.contiguous(), P, pairs.contiguous(),
                                                  threshold, t_res, *outs)
        return tuple(outs)

    # ---- mesh clearance in continuous time (include/msnap.h) --------------------------------------------------------
    def mesh_clearance(self, coef, dur, tris):
        """(min_dist [n], t_min [n], tri_min [n] int32, lower [n], status [n] int32): the certified distance of each
        drone's whole path to the mesh `tris` [T, 3, 3], lower <= infimum <= min_dist."""
        torch = self.torch
        n, M = dur.shape
        if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3) or tris.dtype != torch.float64:
            raise ValueError("mesh_clearance: tris must be a float64 tensor [T, 3, 3]")
        md = self._out("mesh_clearance.md", (n,), torch.float64)
        tm = self._out("mesh_clearance.tm", (n,), torch.float64)
        tri = self._out("mesh_clearance.tri", (n,), torch.int32)
        lower = self._out("mesh_clearance.lower", (n,), torch.float64)
        status = self._out("mesh_clearance.status", (n,), torch.int32)
        if n:
            self.ctx.mesh_clearance_device(n, M, coef, dur, tris.shape[0], tris.contiguous(), md, tm, tri, lower, status)
        return md, tm, tri, lower, status

    # ---- mesh conflict windows: from when until when a path is too close to a mesh (include/msnap.h) ---------------
    _MESH_WINDOW_OUTPUTS = (("t_clear_until", "float64"), ("t_first", "float64"), ("d_first", "float64"),
                            ("tri_first", "int32"), ("t_last", "float64"), ("d_last", "float64"),
                            ("tri_last", "int32"), ("t_clear_from", "float64"), ("status", "int32"))

    def mesh_conflict_window(self, coef, dur, tris, threshold, t_res=1e-6):
        """(t_clear_until, t_first, d_first, tri_first int32, t_last, d_last, tri_last int32, t_clear_from, status
        int32), each [n]: from when until when each drone is closer than `threshold` to the mesh `tris` [T, 3, 3], the
        crossings located to `t_res` seconds (msnap_mesh_conflict_window_device)."""
        torch = self.torch
        n, M = dur.shape
        if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3) or tris.dtype != torch.float64:
            raise ValueError("mesh_conflict_window: tris must be a float64 tensor [T, 3, 3]")
        outs = [self._out(f"mesh_conflict_window.{k}", (n,), getattr(torch, kind))
                for k, kind in self._MESH_WINDOW_OUTPUTS]
        if n:
            self.ctx.mesh_conflict_window_device(n, M, coef, dur, tris.shape[0], tris.contiguous(), threshold, t_res,
                                                 *outs)
        return tuple(outs)

    # ---- path extent in continuous time (include/msnap.h) ------------------------------------------------------------
    def path_extent(self, coef, dur, dirs):
        """(ext [n, K], t_ext [n, K], upper [n, K], status [n] int32): the certified reach of each drone's whole path in
        the directions `dirs` [K, 3], ext <= sup_t n.p(t) <= upper.  With K == 0 the call does nothing (status too)."""
        torch = self.torch
        n, M = dur.shape
        if dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.dtype != torch.float64:
            raise ValueError("path_extent: dirs must be a float64 tensor [K, 3]")
        K = dirs.shape[0]
        ext = self._out("path_extent.ext", (n, K), torch.float64)
        t_ext = self._out("path_extent.t_ext", (n, K), torch.float64)
        upper = self._out("path_extent.upper", (n, K), torch.float64)
        status = self._out("path_extent.status", (n,), torch.int32)
        if n and K:
            self.ctx.path_extent_device(n, M, coef, dur, K, dirs.contiguous(), ext, t_ext, upper, status)
        return ext, t_ext, upper, status

    # ---- half-space windows: from when until when a path is outside a half-space (include/msnap.h) -------------------
    _HALFSPACE_OUTPUTS = ("t_inside_until", "t_first", "v_first", "t_last", "v_last", "t_inside_from")

    def halfspace_window(self, coef, dur, planes, queries, t_res=1e-6, t_from=None, t_to=None):
        """(t_inside_until, t_first, v_first, t_last, v_last, t_inside_from, status int32), each [Q], of the queries
        (int32 [Q, 2]: drone, plane) against `planes` [K, 4] = (n, b), inside being n.x <= b, each on its range
        [t_from, t_to] ([Q] float64 each, or None: 0 / the whole flight), the crossings located to `t_res` seconds
        (msnap_halfspace_window_device)."""
        torch = self.torch
        n, M = dur.shape
        if planes.dim() != 2 or planes.shape[1] != 4 or planes.dtype != torch.float64:
            raise ValueError("halfspace_window: planes must be a float64 tensor [K, 4]")
        if queries.dim() != 2 or queries.shape[1] != 2 or queries.dtype != torch.int32:
            raise ValueError("halfspace_window: queries must be an int32 tensor [Q, 2]")
        Q = queries.shape[0]
        for name, x in (("t_from", t_from), ("t_to", t_to)):
            if x is not None and (tuple(x.shape) != (Q,) or x.dtype != torch.float64):
                raise ValueError(f"halfspace_window: {name} must be a float64 tensor [{Q}]")
        outs = ([self._out(f"halfspace_window.{k}", (Q,), torch.float64) for k in self._HALFSPACE_OUTPUTS]
                + [self._out("halfspace_window.status", (Q,), torch.int32)])
        if Q:
            self.ctx.halfspace_window_device(n, M, coef.contiguous(), dur.contiguous(), planes.shape[0],
                                             planes.contiguous(), Q, queries.contiguous(),
                                             None if t_from is None else t_from.contiguous(),
                                             None if t_to is None else t_to.contiguous(), t_res, *outs)
        return tuple(outs)

    # ---- replanning in flight (include/msnap.h) ----------------------------------------------------------------------
    def solve_states(self, wp, t, start=None, end=None):
        """(coef, dur, status) of the solve from and to given end states: `start` / `end` [n, 4, K-1] float64 -- entry
        q-1 the q-th derivative at the first / last waypoint -- or None for rest; t[0] must be 0."""
        n, m, _ = wp.shape
        M = m - 1
        start, end = self._end_states("solve_states", n, start, end)
        coef, dur, status = self._solve_outs("solve_states", n, M)
        if n:
            self.ctx.solve_states_device(n, M, wp.contiguous(), t.contiguous(), t.dim() == 1, start, end, coef, dur,
                                         status)
        return coef, dur, status

    def solve_gates(self, wp, t, start=None, end=None, fix=None, via=None):
        """(coef, dur, status) of solve_states with prescribed derivatives at interior waypoints: `fix` [n, M-1] int32
        -- bit q-1 of entry i-1: the q-th derivative at waypoint i is prescribed, on all four axes -- and `via`
        [n, M-1, 4, K-1] float64 the values (entries under a clear bit are not used).  fix None: no gates."""
        n, m, _ = wp.shape
        M = m - 1
        start, end = self._end_states("solve_gates", n, start, end)
        fix, via = self._gates("solve_gates", n, M, fix, via)
        coef, dur, status = self._solve_outs("solve_gates", n, M)
        if n:
            self.ctx.solve_gates_device(n, M, wp.contiguous(), t.contiguous(), t.dim() == 1, start, end, fix, via, coef,
                                        dur, status)
        return coef, dur, status

    def solve_periodic(self, wp, t):
        """(coef, dur, status) of the closed-loop solve: the last waypoint is joined to the first, the period is t[-1],
        wp[:, -1] - wp[:, 0] the lap offset; t[0] must be 0."""
        n, m, _ = wp.shape
        M = m - 1
        coef, dur, status = self._solve_outs("solve_periodic", n, M)
        if n:
            self.ctx.solve_periodic_device(n, M, wp.contiguous(), t.contiguous(), t.dim() == 1, coef, dur, status)
        return coef, dur, status

    def optimize_times_periodic(self, wp, t, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200, tol=1e-4):
        """(t_out, coef, dur, status, info) of the time allocation on closed loops: wp, t as solve_periodic takes them
        (the period t[-1] is kept), the rest as Context.optimize_times; info = {"cost": [n, 2], "pg": [n],
        "iters": [n] int32}."""
        return self._optimize_times("optimize_times_periodic", self.ctx.optimize_times_periodic_device, wp, t, (),
                                    weights, (), min_fraction, max_iter, tol)

    def optimize_times_states(self, wp, t, start=None, end=None, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200,
                              tol=1e-4):
        """(t_out, coef, dur, status, info) of the time allocation from and to given end states: arguments as
        solve_states plus the four of Context.optimize_times; info = {"cost": [n, 2], "pg": [n], "iters": [n] int32}."""
        n, _, _ = wp.shape
        states = self._end_states("optimize_times_states", n, start, end)
        return self._optimize_times("optimize_times_states", self.ctx.optimize_times_states_device, wp, t, states,
                                    weights, (), min_fraction, max_iter, tol)

    def optimize_times_free(self, wp, t, start=None, end=None, weights=(1, 1, 1, 1), time_weight=1.0, min_fraction=0.1,
                            max_iter=200, tol=1e-4):
        """(t_out, coef, dur, status, info) of the time allocation with a free total duration: arguments as
        optimize_times_states plus `time_weight` > 0, a number or a float64 tensor [n] (one per drone); t[-1] is a
        starting guess.  info as there, with "cost" the objective, time term included."""
        torch = self.torch
        n, _, _ = wp.shape
        states = self._end_states("optimize_times_free", n, start, end)
        if torch.is_tensor(time_weight):
            if tuple(time_weight.shape) != (n,) or time_weight.dtype != torch.float64:
                raise ValueError("optimize_times_free: time_weight must be a number or a float64 tensor [n]")
            kt = time_weight.to(self.device).contiguous()
        else:
            kt = torch.full((n,), float(time_weight), dtype=torch.float64, device=self.device)
        return self._optimize_times("optimize_times_free", self.ctx.optimize_times_free_device, wp, t, states, weights,
                                    (kt,), min_fraction, max_iter, tol)

    def optimize_times_gates(self, wp, t, start=None, end=None, fix=None, via=None, weights=(1, 1, 1, 1),
                             min_fraction=0.1, max_iter=200, tol=1e-4):
        """(t_out, coef, dur, status, info) of the time allocation through gates: arguments as solve_gates plus the
        four of Context.optimize_times.  The gate values are kept in physical units while the knots move; coef is
        solve_gates' at t_out; fix None is optimize_times_states.  info as there."""
        n, m, _ = wp.shape
        states = self._end_states("optimize_times_gates", n, start, end)
        gates = self._gates("optimize_times_gates", n, m - 1, fix, via)
        return self._optimize_times("optimize_times_gates", self.ctx.optimize_times_gates_device, wp, t,
                                    states + gates, weights, (), min_fraction, max_iter, tol)

    def _gates(self, method, n, M, fix, via):
        """`fix` / `via` of `method` checked -- None, or an int32 tensor [n, M-1] with a float64 tensor
        [n, M-1, 4, K-1] -- and contiguous."""
        torch = self.torch
        if fix is not None:
            if tuple(fix.shape) != (n, max(M - 1, 0)) or fix.dtype != torch.int32:
                raise ValueError(f"{method}: fix must be an int32 tensor [n, M-1]")
            if via is None:
                raise ValueError(f"{method}: fix needs via")
            fix = fix.contiguous()
        if via is not None:
            nd = self.ctx.ncoef // 2 - 1
            if tuple(via.shape) != (n, max(M - 1, 0), 4, nd) or via.dtype != torch.float64:
                raise ValueError(f"{method}: via must be a float64 tensor [n, M-1, 4, {nd}]")
            via = via.contiguous()
        return fix, via

    def _end_states(self, method, n, start, end):
        """`start` / `end` of `method` checked -- None, or a float64 tensor [n, 4, K-1] -- and contiguous."""
        nd = self.ctx.ncoef // 2 - 1
        for name, x in (("start", start), ("end", end)):
            if x is not None and (tuple(x.shape) != (n, 4, nd) or x.dtype != self.torch.float64):
                raise ValueError(f"{method}: {name} must be a float64 tensor [n, 4, {nd}]")
        return None if start is None else start.contiguous(), None if end is None else end.contiguous()

    def _solve_outs(self, method, n, M):
        """coef, dur, status of `method` for n paths of M segments."""
        torch = self.torch
        coef, dur, status = _output_names(method)[:3]
        return (self._out(coef, (n, M, 4, self.ctx.ncoef), torch.float64),
                self._out(dur, (n, M), torch.float64), self._out(status, (n,), torch.int32))

    def _optimize_times(self, method, device_entry, wp, t, states, weights, time_weight, min_fraction, max_iter, tol):
        """The allocators' one body: `device_entry` is Context's `<method>_device`; `states` its checked (start, end)
        -- with (fix, via) behind them for the gates mode -- and `time_weight` its (tensor [n],); () where it takes
        none."""
        torch, out = self.torch, self._out
        n, m, _ = wp.shape
        M = m - 1
        coef, dur, status, t_out, cost, pg, iters = _output_names(method)
        t_out = out(t_out, (n, m), torch.float64)
        coef = out(coef, (n, M, 4, self.ctx.ncoef), torch.float64)
        dur = out(dur, (n, M), torch.float64)
        status = out(status, (n,), torch.int32)
        cost = out(cost, (n, 2), torch.float64)
        pg = out(pg, (n,), torch.float64)
        iters = out(iters, (n,), torch.int32)
        if n:
            device_entry(n, M, wp.contiguous(), t.contiguous(), t.dim() == 1, *states, weights, *time_weight,
                         min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters)
        return t_out, coef, dur, status, {"cost": cost, "pg": pg, "iters": iters}

    def eval_state(self, coef, dur, tq):
        """(pos [n, 4], deriv [n, 4, K-1]) of each drone at its own time tq [n]: NaN outside its path."""
        torch = self.torch
        n, M = dur.shape
        if tuple(tq.shape) != (n,) or tq.dtype != torch.float64:
            raise ValueError("eval_state: tq must be a float64 tensor [n]")
        pos = self._out("eval_state.pos", (n, 4), torch.float64)
        deriv = self._out("eval_state.deriv", (n, 4, self.ctx.ncoef // 2 - 1), torch.float64)
        if n:
            self.ctx.eval_state_device(n, M, coef, dur, tq.contiguous(), pos, deriv)
        return pos, deriv

    # ---- near pairs (include/msnap.h) -------------------------------------------------------------------------------
    _near_pairs_first_capacity = None      # (tests force a tiny first capacity through this)

    def near_pairs(self, pos, base, speed=None, gap=0.0, margin=0.0):
        """(pairs int32 [P, 2], dist [P]): the pairs i < j of `pos` [n, S, 3] whose sampled distance is below
        (base + (speed[i] + speed[j]) gap) (1 + margin), ascending, with that distance (msnap_formation_near_pairs_device).
        The count is read back once; a list that outgrew the first capacity max(4096, 8 n) is fetched by a second call."""
        torch = self.torch
        n, S = pos.shape[0], pos.shape[1]
        if pos.dim() != 3 or pos.shape[2] != 3 or pos.dtype != torch.float64:
            raise ValueError("near_pairs: pos must be a float64 tensor [n, S, 3]")
        if speed is not None and (tuple(speed.shape) != (n,) or speed.dtype != torch.float64):
            raise ValueError("near_pairs: speed must be a float64 tensor [n]")
        if n < 2:
            return (torch.zeros((0, 2), dtype=torch.int32, device=pos.device),
                    torch.zeros((0,), dtype=torch.float64, device=pos.device))
        pos = pos.contiguous()
        speed = None if speed is None else speed.contiguous()
        cap = self._near_pairs_first_capacity or max(4096, 8 * n)
        found = self._out("near_pairs.found", (1,), torch.int64)
        while True:
            pairs = torch.empty((cap, 2), dtype=torch.int32, device=self.device)
            dist = torch.empty((cap,), dtype=torch.float64, device=self.device)
            self.ctx.near_pairs_device(n, S, pos, base, speed, gap, margin, cap, pairs, dist, found)
            P = int(found.item())
            if P <= cap:
                return pairs[:P], dist[:P]
            cap = P

    def collide(self, pos_rows, row_offset, pos_all, radius, rows_t=None):
        torch = self.torch
        r = pos_rows.shape[0]
        md = self._out("collide.md", (r,), torch.float64)
        partner = self._out("collide.partner", (r,), torch.int32)
        hit = self._out("collide.hit", (r,), torch.int32)
        if r and rows_t is not None:
            self.ctx.formation_collide_t_device(r, row_offset, pos_all.shape[0], pos_rows.shape[1], rows_t, pos_rows,
                                                pos_all, radius, md, partner, hit)
        elif r:
            self.ctx.formation_collide_device(r, row_offset, pos_all.shape[0], pos_rows.shape[1], pos_rows,
                                              pos_all, radius, md, partner, hit)
        return md, partner, hit

    # ---- several ranks: who evaluates which pairs -------------------------------------------------------------
    # "parts": every unordered pair on exactly one rank (collide_part), a second small all-gather, the fold -- the
    # arithmetic is divided by the number of ranks.  "whole": every rank runs the pass over the WHOLE gathered swarm
    # behind the exact broad phase and keeps its rows -- no second collective, and on swarms where the broad phase culls
    # (4096-drone formation fixture: 3 % of the pairs are evaluated, 68 us) that is less than a rank's part of all pairs
    # plus its collective.  Both inputs of the choice are the library's: whether a whole pass of this shape would run
    # behind the broad phase (msnap_formation_collide_takes_broad_phase) and whether, by the counts a whole pass left,
    # it pays against the parts (msnap_formation_whole_pass_pays) -- no threshold or cost constant lives here.  Every
    # rank ran the pass on the same positions and gets the same counts; they still agree through one MIN all-reduce.
    REPROBE_EVERY = 256      # passes after which a shape that went to the parts tries one whole pass again

    def pairwise_mode(self, n_total, n_samples, world):
        key = (int(n_total), int(n_samples), int(world))
        if world == 1:
            return "parts"
        st = self._whole_ok.get(key)
        if st is not None and not st["ok"] and st["since"] < self.REPROBE_EVERY:
            return "parts"
        return "whole" if self.ctx.collide_takes_broad_phase(n_total, 0, n_total, n_samples) else "parts"

    def note_parts_pass(self, n_total, n_samples, world):
        """After a pass in parts: counts towards the next re-probe of the whole-swarm mode (a swarm that was dense
        when the decision was taken may have spread out since)."""
        st = self._whole_ok.get((int(n_total), int(n_samples), int(world)))
        if st is not None and not st["ok"]:
            st["since"] += 1

    def note_whole_pass(self, n_total, n_samples, world, dist=None):
        """After a whole-swarm pass: decide whether it pays against the parts -- on the first pass of a swarm shape,
        on a re-probe, and every REPROBE_EVERY whole passes (a sparse swarm may have contracted).  Reads the pass's
        survivor counts (one stream synchronisation).  With `dist` the ranks take the decision together (a MIN
        all-reduce of one flag): a split decision would leave them in different collectives, so the all-reduce is
        entered whatever happened locally -- a rank whose query failed contributes 0 (parts) and re-raises after it."""
        key = (int(n_total), int(n_samples), int(world))
        st = self._whole_ok.get(key)
        if st is not None and st["ok"]:
            st["since"] += 1
            if st["since"] < self.REPROBE_EVERY:
                return
        err = None
        try:
            ok = bool(self.ctx.whole_pass_pays(n_total, world))
        except Exception as e:      # (e.g. MSNAP_ECAPTURE: the query synchronises, the stream is being captured)
            ok, err = False, e
        if dist is not None and world > 1:
            flag = self.torch.tensor([1 if ok else 0], dtype=self.torch.int32,
                                     device=self.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            ok = bool(int(flag.item()))
        self._whole_ok[key] = {"ok": ok, "since": 0}
        if err is not None:
            raise err

    def collide_part(self, pos_all, part, n_parts):
        """This rank's part of the pass over the whole swarm: uint8 [formation_part_bytes(N)] (squared minima
        of every drone over the pairs of this part, then the partners)."""
        n = pos_all.shape[0]
        out = self._out("collide_part.out", (self.ctx.formation_part_bytes(n),), self.torch.uint8)
        if n:
            self.ctx.formation_collide_part_device(n, pos_all.shape[1], pos_all, part, n_parts, out)
        return out

    def collide_finish(self, parts, n_total, row_offset, n_rows, radius):
        """Fold the gathered parts (uint8 [P, formation_part_bytes(N)]) for the rows this rank owns."""
        torch = self.torch
        md = self._out("collide_finish.md", (n_rows,), torch.float64)
        partner = self._out("collide_finish.partner", (n_rows,), torch.int32)
        hit = self._out("collide_finish.hit", (n_rows,), torch.int32)
        if n_rows:
            self.ctx.formation_collide_finish_device(n_total, parts.shape[0], parts, row_offset, n_rows, radius,
                                                     md, partner, hit)
        return md, partner, hit

    def _mesh_on(self, ctx, pos, tris, radius, md=None, hit=None):
        torch = self.torch
        n = pos.shape[0]
        if md is None:
            md = self._out("mesh.md", (n,), torch.float64)
            hit = self._out("mesh.hit", (n,), torch.int32)
        if n:
            ctx.mesh_sweep_device(n, pos.shape[1], pos, tris.shape[0], tris, radius, md, hit)
        return md, hit

    def mesh(self, pos, tris, radius):
        return self._mesh_on(self.ctx, pos, tris, radius)

    def mesh_begin(self, pos, tris, radius):
        """Start the mesh sweep; with a side context it runs next to whatever the main stream does until
        `mesh_end`, otherwise it is an ordinary launch on the main stream.

        All buffers are main-stream allocations: the side stream starts after everything the main stream
        holds now (so a recycled output block is quiet), the inputs are kept referenced until `mesh_end`,
        and `mesh_end` orders the main stream behind the sweep before anything can be recycled."""
        if self._mesh_pending is not None:
            raise RuntimeError("mesh_begin: a sweep is already pending")
        if self.side is None:
            self._mesh_pending = (self.mesh(pos, tris, radius), None)
            return
        n = pos.shape[0]
        md = self._out("mesh.md", (n,), self.torch.float64)
        hit = self._out("mesh.hit", (n,), self.torch.int32)
        self.side.wait_stream(self.main)            # the samples (and the mesh) are ready
        self._mesh_pending = (self._mesh_on(self.side_ctx, pos, tris, radius, md, hit), (pos, tris))

    def mesh_end(self):
        """(min_dist, hit) of the pending sweep, ordered into the main stream."""
        if self._mesh_pending is None:
            raise RuntimeError("mesh_end without mesh_begin")
        (out, _keep), self._mesh_pending = self._mesh_pending, None
        if self.side is not None:
            self.main.wait_stream(self.side)
        return out

    def mesh_abort(self):
        """Join a pending sweep and forget it: what a caller's `finally` runs when something between
        `mesh_begin` and `mesh_end` raised, so that the main stream is ordered behind the side stream before
        the sweep's buffers can be recycled and the next `mesh_begin` is not refused."""
        if self._mesh_pending is not None:
            self.mesh_end()

    def close(self):
        """Drop the wrapper of the side context's stream (call before closing `side_ctx`)."""
        self.mesh_abort()
        self.side = None


@dataclass
class FormationResult:
    lo: int              # first global drone index owned by this rank
    hi: int
    min_dist: object     # [hi-lo]
    partner: object      # [hi-lo] global index
    hit: object          # [hi-lo]
    positions_all: object  # [N, S, 3] after the all-gather
    mesh_min_dist: object = None   # [hi-lo] when a mesh was given
    mesh_hit: object = None


def all_gather_positions(pos_local, n_total: int, world: int, rank: int, dist, torch, force: bool = False):
    """All-gather the ranks' [n_r, S, 3] position blocks into [N, S, 3].  `force`: issue the collective on a
    one-rank group too (a one-GPU box then runs the same RCCL call a multi-GPU job makes).

    Shards may differ by one drone, so every rank pads to the largest shard, one
    `all_gather_into_tensor` moves the padded blocks (a single collective: RCCL
    picks a direct all-gather on the xGMI full mesh; the message is latency bound,
    SURVEY.md 8e) and the padding is dropped afterwards."""
    sizes = shard_sizes(n_total, world)
    if world == 1 and not force:
        return pos_local
    S = pos_local.shape[1]
    nmax = max(sizes)
    gathered = torch.empty((world * nmax, S, 3), dtype=pos_local.dtype, device=pos_local.device)
    if all(s == nmax for s in sizes):
        # even shards (4096 drones on 2, 4 or 8 GPUs): the shard itself is the send buffer
        dist.all_gather_into_tensor(gathered, pos_local.contiguous())
        return gathered
    padded = torch.zeros((nmax, S, 3), dtype=pos_local.dtype, device=pos_local.device)
    padded[:pos_local.shape[0]] = pos_local
    dist.all_gather_into_tensor(gathered, padded)
    parts = [gathered[r * nmax:r * nmax + sizes[r]] for r in range(world)]
    return torch.cat(parts, dim=0)


def all_gather_parts(part_local, world: int, dist, torch, force: bool = False):
    """All-gather the ranks' part blocks (uint8 [B] each) into [world, B]: the second, small collective of the
    formation pass (12 bytes per drone and rank).  `force` as in all_gather_positions."""
    if world == 1 and not force:
        return part_local.reshape(1, -1)
    gathered = torch.empty((world * part_local.shape[0],), dtype=part_local.dtype, device=part_local.device)
    dist.all_gather_into_tensor(gathered, part_local.contiguous())
    return gathered.reshape(world, -1)


def formation_pass(compute, coef_local, dur_local, n_total: int, world: int, rank: int, dt: float,
                   n_samples: int, radius: float, dist=None, torch=None, status_local=None,
                   mesh_tris=None, force_collectives: bool = False, force_mode: str = None,
                   _sampled=None) -> FormationResult:
    """Sample the local shard, exchange, evaluate this rank's part of the swarm's pairs, exchange the
    partial minima and fold them for the own rows (one rank: one symmetric launch, no exchange); with
    `mesh_tris` ([T, 3, 3]) also sweep the local shard against the mesh, started right behind the sampler
    so that a compute object with a side stream overlaps it with the exchanges and the pairwise pass.

    `status_local` (the solve's per-drone status of this shard): a failed solve leaves NaN
    coefficients, and NaN samples never win a minimum (include/msnap.h) -- such a drone would
    read as collision-free and be invisible to the others, so it is refused here.

    `force_collectives`: take the several-rank route -- both collectives, parts and fold, or the whole-swarm mode --
    on a one-rank group as well (what a one-GPU box can execute of the multi-GPU path); `force_mode` ("parts" /
    "whole") pins the pairwise mode instead of asking `compute.pairwise_mode`."""
    lo, hi = shard_bounds(n_total, world, rank)
    if status_local is not None and int(abs(status_local).sum()) != 0:
        raise ValueError("formation_pass: the solve reported failed drones (status != 0) in rows "
                         f"[{lo}, {hi}); their samples are NaN and cannot be collision-checked")
    multi = world > 1 or force_collectives
    if multi:
        mode = force_mode or (compute.pairwise_mode(n_total, n_samples, world) if hasattr(compute, "pairwise_mode") else "parts")
        # checked before the first collective: a compute object without the calls this mode needs must not leave
        # the other ranks waiting in an all-gather this rank never enters
        if mode == "parts" and not (hasattr(compute, "collide_part") and hasattr(compute, "collide_finish")):
            raise TypeError("formation_pass on several ranks needs compute.collide_part / collide_finish "
                            "(every pair on exactly one rank); this compute object only has collide()")
    rows_t = None
    if _sampled is not None:      # (formation_pass_from_waypoints: solve and sampler were one launch)
        pos_local, rows_t = _sampled
    elif not multi and hasattr(compute, "sample_rows_t"):
        pos_local, rows_t = compute.sample_rows_t(coef_local, dur_local, dt, n_samples, n_cols=n_total)
    else:
        pos_local = compute.sample(coef_local, dur_local, dt, n_samples)
    overlapped = mesh_tris is not None and hasattr(compute, "mesh_begin")
    if overlapped:
        compute.mesh_begin(pos_local, mesh_tris, radius)
    try:
        if multi:
            pos_all = all_gather_positions(pos_local, n_total, world, rank, dist, torch, force=force_collectives)
            if mode == "whole":
                md, partner, hit = (x[lo:hi] for x in compute.collide(pos_all, 0, pos_all, radius))
                if hasattr(compute, "note_whole_pass"):
                    compute.note_whole_pass(n_total, n_samples, world, dist if hasattr(dist, "get_backend") else None)
            else:
                part = compute.collide_part(pos_all, rank, world)
                parts = all_gather_parts(part, world, dist, torch, force=force_collectives)
                md, partner, hit = compute.collide_finish(parts, n_total, lo, hi - lo, radius)
                if hasattr(compute, "note_parts_pass"):
                    compute.note_parts_pass(n_total, n_samples, world)
        else:
            pos_all = pos_local
            if rows_t is not None:
                md, partner, hit = compute.collide(pos_local, lo, pos_all, radius, rows_t=rows_t)
            else:
                md, partner, hit = compute.collide(pos_local, lo, pos_all, radius)
        mmd = mhit = None
        if overlapped:
            mmd, mhit = compute.mesh_end()
        elif mesh_tris is not None:
            mmd, mhit = compute.mesh(pos_local, mesh_tris, radius)
    except BaseException as first:
        # join the side stream before the sweep's buffers can be recycled -- and keep the FIRST exception: after a
        # HIP error the join will most likely fail too and would otherwise replace the cause
        if overlapped and hasattr(compute, "mesh_abort"):
            try:
                compute.mesh_abort()
            except Exception as second:
                first.__context__ = second
        raise
    return FormationResult(lo, hi, md, partner, hit, pos_all, mmd, mhit)


def formation_pass_from_waypoints(compute, wp_local, n_total: int, world: int, rank: int, dt: float, n_samples: int,
                                  radius: float, dist=None, torch=None, mesh_tris=None, check_status: bool = True,
                                  force_collectives: bool = False, force_mode: str = None):
    """`formation_pass` for a swarm on the context's prepared time grid, from the waypoints: the solve and the sampler
    are ONE launch (`compute.solve_grid_sample`, msnap_solve_grid_sample_device), the rest is `formation_pass`.
    Returns (FormationResult, coef, dur, status).  `check_status` reads the solve's status back before the pairwise
    pass (one synchronisation) and refuses failed drones as `formation_pass` does; a caller that checks `status`
    itself later passes False and keeps the stream running."""
    lo, hi = shard_bounds(n_total, world, rank)
    multi = world > 1 or force_collectives
    coef, dur, status, pos, rows_t = compute.solve_grid_sample(wp_local, dt, n_samples, n_cols=None if multi else n_total)
    res = formation_pass(compute, coef, dur, n_total, world, rank, dt, n_samples, radius, dist=dist, torch=torch,
                         status_local=status if check_status else None, mesh_tris=mesh_tris,
                         force_collectives=force_collectives, force_mode=force_mode, _sampled=(pos, rows_t))
    return res, coef, dur, status


def check_limits(limits):
    """The host-side check of msnap_retime_to_limits' limits: 4 values, none negative or NaN (0 / inf: no limit)."""
    lim = np.asarray(limits, dtype=np.float64)
    if lim.shape != (4,) or not bool(np.all(lim >= 0.0)):
        raise ValueError(f"limits must be 4 values (speed, acceleration, jerk, yaw rate), none negative or NaN: {limits}")
    return lim


def retime_swarm(compute, coef_local, dur_local, limits, world: int, rank: int, dist=None, fit: bool = False,
                 common: bool = True):
    """Retime a swarm sharded over `world` ranks to the dynamic limits (speed, acceleration, jerk, yaw rate; 0 = none).

    `common` (the default: a formation stays in step): every rank computes its drones' factors, one MAX all-reduce of a
    single value gives the swarm's factor and `compute.time_scale` applies it -- the result equals one
    `retime_to_limits(..., common=True)` over the whole swarm.  A rank without drones, or whose drones all failed,
    contributes a neutral 0; failed drones (NaN coefficients) pass through with scale NaN.  Every rank enters the
    collective whatever happened locally (a rank that raised would leave the others waiting); an error is re-raised
    after it.  Returns (coef, dur, scale) of the local drones."""
    if not common:
        check_limits(limits)
        return compute.retime_to_limits(coef_local, dur_local, limits, fit=fit, common=False)
    import torch
    n = dur_local.shape[0]
    err, scale, k_local = None, None, None
    try:
        check_limits(limits)
        if n:
            _, _, scale = compute.retime_to_limits(coef_local, dur_local, limits, fit=fit, common=True)
            k_local = torch.nan_to_num(scale, nan=0.0).amax().reshape(1)
    except Exception as e:      # (entered the collective below all the same)
        err = e
    if k_local is None or err is not None:
        k_local = torch.zeros(1, dtype=torch.float64)
    if dist is not None and world > 1:
        on_device = dist.get_backend() == "nccl"
        k = k_local.to(dur_local.device) if on_device else k_local.cpu()
        dist.all_reduce(k, op=dist.ReduceOp.MAX)
    else:
        k = k_local
    if err is not None:
        raise err
    if not n:
        return coef_local, dur_local, torch.zeros((0,), dtype=torch.float64, device=dur_local.device)
    scale = torch.where(torch.isnan(scale), scale, k.to(scale.device).expand_as(scale)).contiguous()
    coef_out, dur_out = compute.time_scale(coef_local, dur_local, scale)
    return coef_out, dur_out, scale


def default_sample_count(total_duration: float, dt: float) -> int:
    """len(np.arange(0, duration, dt)) -- the reference's sampling loop
    (src/trajectory_visualising/visualization.py:53)."""
    return int(len(np.arange(0.0, total_duration, dt)))


# ---- certified clearance of a swarm: the sampled pass decides what it can, the exact kernel sees the rest ------------
# V_i = peak (1 + 2e-9) exceeds the true speed S by the peaks' contract (include/msnap.h: S (1 - 1e-9) <= peak + 1e-12
# + r_0) wherever 1e-12 + r_0 <= 9e-10 peak: then S <= peak (1 + 9e-10) / (1 - 1e-9) < peak (1 + 2e-9).  That is a speed
# of at least 2e-3 m/s (1e-12 <= 5e-10 peak) with r_0 <= 4e-10 peak.  A solved path has r_0 around 1e-14 of its peak;
# hand-made coefficients that cancel to 1e-5 of their size do not qualify.
PEAK_MARGIN = 2e-9
COMPARE_MARGIN = 1e-9    # relative margin of the fp64 compares against 2 radius + (V_i + V_j) gap


def sample_gap(dt: float, n_samples: int, totals) -> float:
    """The largest distance from a time at which a drone flies to the nearest sample at which it still flies: dt / 2
    inside the grid, more at the end of a path the grid stops short of (`default_sample_count` stops one step early: a
    10 s path sampled at 0.1 s ends at 9.9 s, gap 0.1 s).  Per drone with total duration T the samples are s dt,
    s < n_samples, s dt <= T (a sample beyond T reads the extrapolated last piece, which the certified speed does not
    bound); the result is the maximum over the drones (`totals`: their total durations)."""
    totals = np.asarray(totals, dtype=np.float64).reshape(-1)
    if n_samples < 1 or not dt > 0.0:
        raise ValueError("sample_gap: n_samples >= 1 and dt > 0")
    if totals.size == 0:
        return 0.5 * dt
    k = np.minimum(np.floor(totals / dt), n_samples - 1)
    k = np.where(k * dt > totals, k - 1, k)
    tail = totals - k * dt
    inner = np.where(k >= 1, 0.5 * dt, 0.0)
    return float(np.maximum(inner, tail).max())


@dataclass
class ClearanceResult:
    # [N] a proven lower bound of the drone's distance to every other drone while both fly, up to the rounding allowance
    # of msnap_pair_clearance (include/msnap.h): certified_lower <= D (1 + 1e-13) + 1e-13 + C_ROUND 2^-52 R for the
    # exact infimum D of each of the drone's pairs, R the largest sum_k |c_k| T_i^k over x, y, z, the two drones and
    # the segments that meet the pair's window -- an ulp of the coordinates, which far from the origin exceeds 1e-13 m
    certified_lower: object
    hit: object               # [N] bool: some pair of the drone ATTAINS a distance below 2 radius (definite)
    undecided: object         # [N] bool: no hit, but a pair with lower < 2 radius <= min_dist (a search that met its caps)
    cleared_by_sampling: object   # [N] bool: the sampled pass and the speed peaks alone prove >= 2 radius
    sampled_min_dist: object  # [N] the sampled pass, for comparison
    sampled_partner: object
    sampled_hit: object
    pairs: object             # [P, 2] int32: the pairs that went through msnap_pair_clearance
    pair_min_dist: object     # [P]
    pair_t_min: object
    pair_lower: object
    gap: float
    n_uncertain: int          # |U|: drones the sampled pass could not clear


def uncertain_pairs(pos_u, idx_u, v_u, radius: float, gap: float, torch, budget: int = 1 << 22):
    """Among the drones idx_u (positions pos_u [U, S, 3], speeds v_u [U]) the pairs (i < j, global indices, int32
    [P, 2]) whose sampled distance is below (2 radius + (V_i + V_j) gap) (1 + COMPARE_MARGIN)."""
    U, S = pos_u.shape[0], pos_u.shape[1]
    out = []
    rows = max(1, budget // max(1, U * S))
    for r0 in range(0, U, rows):
        r1 = min(U, r0 + rows)
        d = pos_u[r0:r1, None] - pos_u[None]                       # [rows, U, S, 3]
        dist = (d * d).sum(dim=-1).amin(dim=-1).sqrt()             # [rows, U]
        lim = (2.0 * radius + (v_u[r0:r1, None] + v_u[None, :]) * gap) * (1.0 + COMPARE_MARGIN)
        keep = dist < lim
        ii, jj = torch.nonzero(keep, as_tuple=True)
        ii = ii + r0
        sel = ii < jj
        out.append(torch.stack([idx_u[ii[sel]], idx_u[jj[sel]]], dim=1))
    if not out:
        return torch.zeros((0, 2), dtype=torch.int32, device=pos_u.device)
    return torch.cat(out, dim=0).to(torch.int32).contiguous()


def certify_clearance(compute, coef, dur, radius: float, dt: float, n_samples: int, status=None, world: int = 1,
                      rank: int = 0, pair_filter: str = "auto") -> ClearanceResult:
    """Certify the drone-vs-drone clearance of a swarm in continuous time.

    1. the sampled pass as `formation_pass` runs it, and the certified speed peaks V_i = peak (1 + 2e-9);
    2. gap = `sample_gap`;
    3. a drone whose sampled minimum distance d_i is at least 2 radius + (V_i + V_max) gap is cleared by sampling: a
       pair that truly comes within 2 radius has a sample within gap of that moment, at which both of its drones fail
       this test;
    4. among the other drones U, the pairs whose sampled distance is below 2 radius + (V_i + V_j) gap -- listed by
       `compute.near_pairs` (msnap_formation_near_pairs_device) where the compute object has it, by `uncertain_pairs`
       (torch) where it has not or with `pair_filter="torch"`: the same list, in the same order --
    5. go through `compute.pair_clearance` (msnap_pair_clearance_device).

    One rank only: several ranks would need a gather of the uncertain drones' coefficients, which is not built --
    `world > 1` raises.  Drones whose solve failed (`status` != 0) are refused, as `formation_pass` does."""
    import torch
    if world != 1 or rank != 0:
        raise NotImplementedError("certify_clearance runs on one rank: the gather of the uncertain drones' "
                                  "coefficients over several ranks is not built")
    if not (radius >= 0.0):
        raise ValueError("certify_clearance: radius >= 0")
    if pair_filter not in ("auto", "torch"):
        raise ValueError('certify_clearance: pair_filter is "auto" or "torch"')
    n = dur.shape[0]
    res = formation_pass(compute, coef, dur, n, 1, 0, dt, n_samples, radius, status_local=status)
    peak, _, pst = compute.dynamic_peaks(coef, dur)
    if int(pst.abs().sum()) != 0:
        raise ValueError("certify_clearance: drones with non-finite coefficients or durations <= 0 cannot be certified")
    d = res.min_dist
    v = peak[:, 0] * (1.0 + PEAK_MARGIN)
    gap = sample_gap(dt, n_samples, dur.sum(dim=1).cpu().numpy())
    v_max = v.max() if n else 0.0
    reach = (v + v_max) * gap
    cleared = d >= (2.0 * radius + reach) * (1.0 + COMPARE_MARGIN)
    idx_u = torch.nonzero(~cleared, as_tuple=True)[0]
    if pair_filter == "auto" and hasattr(compute, "near_pairs"):
        local, _ = compute.near_pairs(res.positions_all[idx_u], 2.0 * radius, v[idx_u], gap, COMPARE_MARGIN)
        pairs = idx_u[local.to(torch.int64)].to(torch.int32).reshape(-1, 2).contiguous()
    else:
        pairs = uncertain_pairs(res.positions_all[idx_u], idx_u, v[idx_u], radius, gap, torch)
    # everything that is not a kept pair is at least 2 radius apart: a cleared drone by its own bound d_i - reach_i
    # (which covers all of its pairs), a pair of U that was not kept by d_ij - (V_i + V_j) gap >= 2 radius
    lip = torch.where(cleared, (d - reach) * (1.0 - COMPARE_MARGIN), torch.full_like(d, 2.0 * radius))
    certified = lip.clone()
    hit = torch.zeros((n,), dtype=torch.bool, device=d.device)
    undecided = torch.zeros((n,), dtype=torch.bool, device=d.device)
    P = pairs.shape[0]
    if P:
        md, tm, lower, pstat = compute.pair_clearance(coef, dur, pairs)
        if int(pstat.abs().sum()) != 0:
            raise ValueError("certify_clearance: msnap_pair_clearance reported failed pairs")
        md, tm, lower = md.clone(), tm.clone(), lower.clone()
        both = pairs.to(torch.int64).reshape(-1)                      # a0 b0 a1 b1 ...
        certified.scatter_reduce_(0, both, lower.repeat_interleave(2), reduce="amin", include_self=True)
        p_hit = md < 2.0 * radius
        p_und = (~p_hit) & (lower < 2.0 * radius)
        hit[both[p_hit.repeat_interleave(2)]] = True
        undecided[both[p_und.repeat_interleave(2)]] = True
        undecided &= ~hit
    else:
        md = tm = lower = torch.zeros((0,), dtype=torch.float64, device=d.device)
    return ClearanceResult(certified, hit, undecided, cleared, d, res.partner, res.hit, pairs, md, tm, lower, gap,
                           int(idx_u.numel()))


# ---- certified clearance of a swarm against a mesh: the sampled sweep decides what it can, the kernel sees the rest --
@dataclass
class MeshClearanceResult:
    min_dist: object          # [N] a distance the drone attains to the mesh (a cleared drone: its sampled minimum)
    t_min: object             # [N] the absolute time of min_dist (NaN for a drone cleared by sampling)
    triangle: object          # [N] int32: the triangle of min_dist (-1 for a drone cleared by sampling)
    # [N] a proven lower bound of the drone's distance to the mesh over its whole path, up to the rounding allowance of
    # msnap_mesh_clearance (include/msnap.h); for a drone cleared by sampling (d_i - V_i gap) (1 - COMPARE_MARGIN)
    certified_lower: object
    hit: object               # [N] bool: min_dist < radius, the sweep's rule (definite: the distance is attained)
    undecided: object         # [N] bool: no hit, but certified_lower < radius (a search that met its caps)
    cleared_by_sampling: object   # [N] bool: the sampled sweep and the speed peak alone prove >= radius
    sampled_min_dist: object  # [N] the sampled sweep, for comparison
    sampled_hit: object
    gap: float
    n_uncertain: int          # drones that went through msnap_mesh_clearance


def certify_mesh_clearance(compute, coef, dur, tris, radius: float, dt: float, n_samples: int,
                           status=None) -> MeshClearanceResult:
    """Certify the drone-vs-mesh clearance of a swarm in continuous time.

    1. the sampled sweep as `formation_pass` runs it (`compute.sample`, `compute.mesh`), and the certified speed peaks
       V_i = peak (1 + 2e-9);
    2. gap = `sample_gap`;
    3. a drone whose sampled minimum distance d_i is at least (radius + V_i gap) (1 + COMPARE_MARGIN) is cleared by
       sampling: every moment of its flight is within gap of a sample, and the distance to the mesh changes by at most
       V_i gap in between;
    4. the other drones go through `compute.mesh_clearance` (msnap_mesh_clearance_device).

    One rank: every drone is checked on its own, so a sharded swarm calls this per shard.  Drones whose solve failed
    (`status` != 0) are refused, as `formation_pass` does."""
    import torch
    if not (radius >= 0.0):
        raise ValueError("certify_mesh_clearance: radius >= 0")
    if status is not None and int(abs(status).sum()) != 0:
        raise ValueError("certify_mesh_clearance: the solve reported failed drones (status != 0); their samples are "
                         "NaN and cannot be checked")
    n = dur.shape[0]
    pos = compute.sample(coef, dur, dt, n_samples)
    d, shit = compute.mesh(pos, tris, radius)
    d, shit = d.clone(), shit.clone().to(torch.bool)
    peak, _, pst = compute.dynamic_peaks(coef, dur)
    if int(pst.abs().sum()) != 0:
        raise ValueError("certify_mesh_clearance: drones with non-finite coefficients or durations <= 0 cannot be certified")
    v = peak[:, 0] * (1.0 + PEAK_MARGIN)
    gap = sample_gap(dt, n_samples, dur.sum(dim=1).cpu().numpy())
    reach = v * gap
    cleared = d >= (radius + reach) * (1.0 + COMPARE_MARGIN)
    idx_u = torch.nonzero(~cleared, as_tuple=True)[0]
    min_dist = d.clone()
    t_min = torch.full_like(d, float("nan"))
    triangle = torch.full((n,), -1, dtype=torch.int32, device=d.device)
    certified = (d - reach) * (1.0 - COMPARE_MARGIN)
    if idx_u.numel():
        md, tm, tri, lower, mst = compute.mesh_clearance(coef[idx_u].contiguous(), dur[idx_u].contiguous(), tris)
        if int(mst.abs().sum()) != 0:
            raise ValueError("certify_mesh_clearance: msnap_mesh_clearance reported failed drones")
        min_dist[idx_u], t_min[idx_u], triangle[idx_u], certified[idx_u] = md, tm, tri, lower
    hit = min_dist < radius
    undecided = (~hit) & (certified < radius)
    return MeshClearanceResult(min_dist, t_min, triangle, certified, hit, undecided, cleared, d, shit, gap,
                               int(idx_u.numel()))


# ---- certified geofence: a box and / or half-spaces against the support function of every path ----------------------
GEOFENCE_INSIDE, GEOFENCE_OUTSIDE, GEOFENCE_UNDECIDED, GEOFENCE_FAILED = 0, 1, 2, 3


@dataclass
class GeofenceResult:
    verdict: object           # [N] int8: GEOFENCE_INSIDE / _OUTSIDE / _UNDECIDED / _FAILED
    inside: object            # [N] bool: every upper is below its limit (certified)
    outside: object           # [N] bool: some ext exceeds its limit (definite: the value is attained)
    undecided: object         # [N] bool: neither -- only possible within the closing gap of msnap_path_extent
    failed: object            # [N] bool: status != 0, the solve's or msnap_path_extent's: nothing is certified
    worst: object             # [N] int64: the constraint with the largest ext - limit (index into `normals`; -1: failed)
    t_worst: object           # [N] the absolute time of that constraint's ext (NaN: failed)
    excess: object            # [N] ext - limit of that constraint: > 0 for an `outside` drone (NaN: failed)
    normals: object           # [C, 3] the constraints' directions: the box's finite sides (+x, -x, +y, -y, +z, -z order), then the planes
    limits: object            # [C] their limits, the drone's radius taken off: n.p <= limit
    ext: object               # [N, C] msnap_path_extent's outputs for `normals`
    t_ext: object
    upper: object
    box_lo: object            # [N, 3] the certified box of each path, [-upper(-e_a), upper(+e_a)] (None: no box given)
    box_hi: object


def certify_geofence(compute, coef, dur, lo=None, hi=None, planes=None, radius: float = 0.0,
                     status=None) -> GeofenceResult:
    """Certify in continuous time that every drone of `coef`, `dur` stays inside a convex geofence.

    The fence is a box `lo` / `hi` (each [3]; -inf / +inf: that side is unconstrained) and / or half-spaces `planes`
    [P, 4] = (n, b) meaning n.x <= b; a drone is a sphere of `radius`, which moves each limit by radius |n|.  The
    directions go through `compute.path_extent` (msnap_path_extent_device).  Per drone, the first that applies:
      failed     status != 0 (`status`: the solve's; or this call's): such a drone is refused, nothing is certified;
      outside    some ext exceeds its limit: an attained violation -- `worst`, `t_worst`, `excess` name it;
      inside     every upper is below its limit (strictly: a path that only touches a limit is not certified);
      undecided  neither: a limit inside the closing gap between ext and upper.
    When a box is given the certified box of every path comes back as well (all six axes are evaluated then).

    One rank: every drone is checked on its own, so a sharded swarm calls this per shard."""
    import torch
    if not (radius >= 0.0):
        raise ValueError("certify_geofence: radius >= 0")
    dev = dur.device
    n = dur.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    axes = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], **f64)
    have_box = lo is not None or hi is not None
    box_lim = torch.full((6,), float("inf"), **f64)
    if have_box:
        lo_t = torch.full((3,), -float("inf"), **f64) if lo is None else torch.as_tensor(lo, dtype=torch.float64).to(dev)
        hi_t = torch.full((3,), float("inf"), **f64) if hi is None else torch.as_tensor(hi, dtype=torch.float64).to(dev)
        if tuple(lo_t.shape) != (3,) or tuple(hi_t.shape) != (3,) or bool(torch.isnan(lo_t).any() | torch.isnan(hi_t).any()):
            raise ValueError("certify_geofence: lo and hi are [3], without NaN")
        box_lim[0::2], box_lim[1::2] = hi_t, -lo_t
    if planes is not None:
        pl = torch.as_tensor(planes, dtype=torch.float64).to(dev).reshape(-1, 4)
        if not bool(torch.isfinite(pl).all()):
            raise ValueError("certify_geofence: planes must be finite")
    else:
        pl = torch.zeros((0, 4), **f64)
    # what is sent: all six axes when a box is given (the certified box), then the planes; what is judged: the finite ones
    dirs = torch.cat([axes if have_box else axes[:0], pl[:, :3]]).contiguous()
    lim_all = torch.cat([box_lim if have_box else box_lim[:0], pl[:, 3]])
    lim_all = lim_all - radius * torch.linalg.vector_norm(dirs, dim=1)
    bad = torch.zeros((n,), dtype=torch.bool, device=dev)
    if status is not None:
        bad |= torch.as_tensor(status).to(dev) != 0
    ext, t_ext, upper, st = compute.path_extent(coef, dur, dirs)
    if dirs.shape[0]:
        bad |= st != 0
    ext, t_ext, upper = ext.clone(), t_ext.clone(), upper.clone()
    box_lo = box_hi = None
    if have_box:
        box_hi, box_lo = upper[:, 0:6:2].clone(), -upper[:, 1:6:2]
    keep = torch.isfinite(lim_all)
    normals, limits = dirs[keep], lim_all[keep]
    ext, t_ext, upper = ext[:, keep], t_ext[:, keep], upper[:, keep]
    C = int(keep.sum())
    nan = torch.full((n,), float("nan"), **f64)
    if C:
        over = ext - limits[None, :]
        over = torch.where(torch.isnan(over), torch.full_like(over, -float("inf")), over)
        excess, worst = over.max(dim=1)
        t_worst = t_ext.gather(1, worst[:, None])[:, 0]
        outside = ~bad & (ext > limits[None, :]).any(dim=1)
        inside = ~bad & ~outside & (upper < limits[None, :]).all(dim=1)
    else:
        excess, worst, t_worst = nan.clone(), torch.full((n,), -1, dtype=torch.int64, device=dev), nan.clone()
        outside = torch.zeros_like(bad)
        inside = ~bad
    undecided = ~bad & ~outside & ~inside
    worst = torch.where(bad, torch.full_like(worst, -1), worst)
    t_worst, excess = torch.where(bad, nan, t_worst), torch.where(bad, nan, excess)
    verdict = torch.full((n,), GEOFENCE_UNDECIDED, dtype=torch.int8, device=dev)
    verdict[inside], verdict[outside], verdict[bad] = GEOFENCE_INSIDE, GEOFENCE_OUTSIDE, GEOFENCE_FAILED
    return GeofenceResult(verdict, inside, outside, undecided, bad, worst, t_worst, excess, normals, limits, ext, t_ext,
                          upper, box_lo, box_hi)


def replan(compute, coef, dur, t_r, wp_new, t_new, end=None, optimize=None, gates=None):
    """Replan a flying swarm: leave the paths `coef`, `dur` at time `t_r` and fly through new waypoints.

    `t_r` is a number or a tensor [N] (per drone, on the current paths' clock); `wp_new` [N, M', 4] are the waypoints
    after the current position, `t_new` [N, M'] or [M'] their times counted from `t_r`, strictly positive and
    increasing; `end` [N, 4, K-1] the state to arrive in (None: rest).  The state at `t_r` comes from
    `compute.eval_state`, its position becomes the waypoint at time 0, its derivatives the start state of
    `compute.solve_states`.  Returns (coef, dur, status, (pos, deriv)) -- the new paths on a clock that starts at `t_r`,
    and the state they start from.  A drone whose `t_r` lies outside its path has a NaN state and comes back with
    status 3 and NaN coefficients, as does one with bad times (status 2): nothing raises per drone.

    `optimize`: None solves at `t_new` as given.  A dict with any of weights / min_fraction / max_iter / tol lets
    `compute.optimize_times_states` move the interior times first (the state at `t_r`, the waypoints, `end` and the
    last time are kept); the knots it chose are the running sum of the returned `dur`.  With "time_weight" in the dict
    (a number or a tensor [N], > 0) `compute.optimize_times_free` moves every time, the last one too: `t_new[-1]` is
    then a starting guess, and a larger weight buys a shorter path at a higher cost.

    `gates`: (fix, via) as `compute.solve_gates` takes them -- fix [N, M' - 1] int32, via [N, M' - 1, 4, K-1], entry
    i-1 for `wp_new[:, i-1]`, the new path's interior waypoint i; the last new waypoint takes `end`.  `gates`
    together with `optimize` raises ValueError here: time allocation through gates is `replan_gated`."""
    if gates is not None and optimize is not None:
        raise ValueError("replan: gates and optimize do not combine here; replan_gated allocates times through gates")
    wp, t, pos, deriv = _replan_inputs(compute, coef, dur, t_r, wp_new, t_new)
    if gates is not None:
        fix, via = gates
        new_coef, new_dur, status = compute.solve_gates(wp, t, start=deriv, end=end, fix=fix, via=via)
    elif optimize is None:
        new_coef, new_dur, status = compute.solve_states(wp, t, start=deriv, end=end)
    else:
        unknown = set(optimize) - {"weights", "min_fraction", "max_iter", "tol", "time_weight"}
        if unknown:
            raise ValueError("replan: optimize takes weights, min_fraction, max_iter, tol, time_weight, not "
                             f"{sorted(unknown)}")
        entry = compute.optimize_times_free if "time_weight" in optimize else compute.optimize_times_states
        _, new_coef, new_dur, status, _ = entry(wp, t, start=deriv, end=end, **optimize)
    return new_coef, new_dur, status, (pos, deriv)


def replan_gated(compute, coef, dur, t_r, wp_new, t_new, gates, end=None, optimize=None):
    """`replan` through gates, with or without time allocation: arguments and the returned tuple as `replan`, `gates`
    = (fix, via) as described there.  `optimize` None: `compute.solve_gates` at `t_new` as given.  A dict with any of
    weights / min_fraction / max_iter / tol: `compute.optimize_times_gates` moves the interior times first -- the state
    at `t_r`, the waypoints, `end`, the last time and the gate values in physical units are kept.  "time_weight" raises
    ValueError: a free total duration through gates is not built."""
    fix, via = gates
    if optimize is not None:
        if "time_weight" in optimize:
            raise ValueError("replan_gated: time_weight (a free total duration) does not combine with gates: not built")
        unknown = set(optimize) - {"weights", "min_fraction", "max_iter", "tol"}
        if unknown:
            raise ValueError(f"replan_gated: optimize takes weights, min_fraction, max_iter, tol, not {sorted(unknown)}")
    wp, t, pos, deriv = _replan_inputs(compute, coef, dur, t_r, wp_new, t_new)
    if optimize is None:
        new_coef, new_dur, status = compute.solve_gates(wp, t, start=deriv, end=end, fix=fix, via=via)
    else:
        _, new_coef, new_dur, status, _ = compute.optimize_times_gates(wp, t, start=deriv, end=end, fix=fix, via=via,
                                                                        **optimize)
    return new_coef, new_dur, status, (pos, deriv)


def _replan_inputs(compute, coef, dur, t_r, wp_new, t_new):
    """(wp [N, M' + 1, 4], t [N, M' + 1] or [M' + 1], pos, deriv) of a replan: the state at `t_r` in front of the new
    waypoints, 0 in front of their times."""
    import torch
    n = dur.shape[0]
    dev = dur.device
    if wp_new.dim() != 3 or wp_new.shape[0] != n or wp_new.shape[2] != 4 or wp_new.shape[1] < 1:
        raise ValueError("replan: wp_new must be [N, M', 4] with M' >= 1")
    mp_ = wp_new.shape[1]
    if tuple(t_new.shape) not in ((mp_,), (n, mp_)):
        raise ValueError("replan: t_new must be [N, M'] or [M']")
    tq = torch.as_tensor(t_r, dtype=torch.float64).to(dev)
    tq = tq.expand(n).contiguous() if tq.dim() == 0 else tq.contiguous()
    pos, deriv = compute.eval_state(coef, dur, tq)
    wp = torch.cat([pos[:, None, :], wp_new.to(torch.float64)], dim=1).contiguous()
    t = torch.cat([torch.zeros(t_new.shape[:-1] + (1,), dtype=torch.float64, device=dev), t_new.to(torch.float64)],
                  dim=-1).contiguous()
    return wp, t, pos, deriv


def replan_within_limits(compute, coef, dur, t_r, wp_new, t_new, limits, end=None, rounds=8, optimize=None):
    """`replan` with the total duration chosen per drone so that the new path keeps the dynamic `limits` (speed,
    acceleration, jerk, yaw rate; 0 or inf: none) and is no slower than they ask: a search over the time weight of
    `compute.optimize_times_free`.  A replanned path cannot be stretched afterwards (its start state is in physical
    units), so the limits are met by the choice of the weight instead.

    Each of the `rounds` rounds is one `optimize_times_free` launch, one `dynamic_peaks` launch and one synchronising
    read.  Every drone starts at k_0 = (2k - 1) J(t_new) / t_new[-1], the weight at which the caller's total would be
    stationary if the cost were homogeneous.  A drone whose certified peak upper bounds peak (1 + 2e-9) are all within
    `limits` has its weight multiplied by 4, any other divided by 4; once a drone has both a feasible and a violating
    weight, the next one is their geometric mean.  `optimize`: weights / min_fraction / max_iter / tol as `replan`.

    Returns (coef, dur, status, (pos, deriv), info): per drone the path of the largest feasible weight tried, and info =
    {"time_weight": [N] that weight, "violating_weight": [N] the smallest weight found to violate (inf: none),
    "feasible": [N] bool (host arrays), "peaks": [N, 4] the kept path's peaks (device)}.  A drone with no feasible
    weight in `rounds` rounds -- one whose start speed already exceeds the speed limit, say -- keeps feasible = False
    and the path of the smallest weight tried."""
    import torch
    lim = check_limits(limits)
    if rounds < 1:
        raise ValueError("replan_within_limits: rounds must be at least 1")
    opt = dict(optimize or {})
    unknown = set(opt) - {"weights", "min_fraction", "max_iter", "tol"}
    if unknown:
        raise ValueError(f"replan_within_limits: optimize takes weights, min_fraction, max_iter, tol, not {sorted(unknown)}")
    wp, t, pos, deriv = _replan_inputs(compute, coef, dur, t_r, wp_new, t_new)
    n, dev = wp.shape[0], wp.device
    order = compute.ctx.order                                  # 2k - 1
    bound = torch.from_numpy(np.where((lim > 0.0) & np.isfinite(lim), lim, np.inf)).to(dev)
    # J at the input times: the states entry at max_iter 0 (no synchronisation; a failed drone's NaN travels on)
    rest = {k: v for k, v in opt.items() if k in ("weights", "min_fraction")}
    _, _, _, _, at_input = compute.optimize_times_states(wp, t, start=deriv, end=end, max_iter=0, **rest)
    k = (order * at_input["cost"][:, 0] / t[..., -1]).cpu().numpy()
    k_feas, k_viol, k_low = np.zeros(n), np.full(n, np.inf), np.full(n, np.inf)
    kept = None
    for _ in range(rounds):
        _, c, d, st, _ = compute.optimize_times_free(wp, t, start=deriv, end=end,
                                                     time_weight=torch.from_numpy(k).to(dev), **opt)
        peak, _, pst = compute.dynamic_peaks(c, d)
        ok = ((st == 0) & (pst == 0) & (peak * (1.0 + PEAK_MARGIN) <= bound[None, :]).all(dim=1)).cpu().numpy()
        # this round's path is kept by a drone it is the best feasible one of, or the slowest one of while none is
        take = (ok & (k > k_feas)) | (~ok & (k_feas == 0.0) & (k < k_low))
        k_feas = np.where(ok, np.maximum(k_feas, k), k_feas)
        k_viol = np.where(ok, k_viol, np.minimum(k_viol, k))
        k_low = np.minimum(k_low, k)
        if kept is None:
            kept = [c.clone(), d.clone(), st.clone(), peak.clone()]
        else:
            m = torch.from_numpy(take).to(dev)
            for dst, src in zip(kept, (c, d, st, peak)):
                dst.copy_(torch.where(m.reshape((n,) + (1,) * (src.dim() - 1)), src, dst))
        both = (k_feas > 0.0) & np.isfinite(k_viol)
        k = np.where(both, np.sqrt(k_feas * k_viol), np.where(k_feas > 0.0, 4.0 * k_feas, 0.25 * k_low))
    feasible = k_feas > 0.0
    info = {"time_weight": np.where(feasible, k_feas, k_low), "violating_weight": k_viol, "feasible": feasible,
            "peaks": kept[3]}
    return kept[0], kept[1], kept[2], (pos, deriv), info


def join_loop(compute, coef, dur, t_r, loop_coef, loop_dur, wp_via, t_via, optimize=None):
    """Park a flying swarm on holding loops: leave the paths `coef`, `dur` at time `t_r` and arrive on the loops
    `loop_coef`, `loop_dur` (what `compute.solve_periodic` returned) at their first waypoint, in the loops' own state.

    `wp_via` [N, V, 4] are waypoints to pass on the way (V may be 0); `t_via` [N, V + 1] or [V + 1] holds their times
    and, last, the arrival time on the loop, all counted from `t_r`.  This is `replan` with the loop's first waypoint
    appended as the last one and `end` taken from `compute.eval_state` of the loop at 0: positions and derivatives
    1 .. K-1 are continuous at both hand-overs.  Returns what `replan` returns; `optimize` as there."""
    import torch
    n = dur.shape[0]
    if loop_dur.shape[0] != n or loop_coef.shape[0] != n:
        raise ValueError("join_loop: loop_coef, loop_dur hold one loop per drone")
    if wp_via.dim() != 3 or wp_via.shape[0] != n or wp_via.shape[2] != 4:
        raise ValueError("join_loop: wp_via must be [N, V, 4]")
    zero = torch.zeros((n,), dtype=torch.float64, device=dur.device)
    pos, deriv = compute.eval_state(loop_coef, loop_dur, zero)
    # (replan evaluates too: with reuse_outputs the same tensors would come back)
    wp_new = torch.cat([wp_via.to(torch.float64), pos[:, None, :]], dim=1)
    return replan(compute, coef, dur, t_r, wp_new, t_via, end=deriv.clone(), optimize=optimize)


# ---- certified clearance of replanned paths against the paths that stay, and against each other ---------------------
@dataclass
class ReplanClearanceResult:
    # per replanned drone [K], in the order of `idx`: a proven lower bound of its distance, on the new path, to every
    # drone that keeps its path and to every other replanned drone while both fly, up to the rounding allowance of
    # msnap_cross_clearance (include/msnap.h): certified_lower <= D (1 + 1e-13) + r for the exact infimum D of each pair
    certified_lower: object
    hit: object               # [K] bool: some pair of the drone ATTAINS a distance below 2 radius (definite)
    undecided: object         # [K] bool: no hit, but a pair with lower < 2 radius <= min_dist (a search that met its caps)
    pairs: object             # [P, 2] int32, swarm indices: (replanned drone, the other drone); new-old pairs first
    pair_new_new: object      # [P] bool: the other drone is replanned too (both on their new paths)
    pair_min_dist: object     # [P]
    pair_t_min: object        # [P] on the swarm's clock
    pair_lower: object        # [P]


def _replan_pairs(who, dur, idx, t_r, new_coef, new_dur):
    """The pair lists of a replan, shared by certify_replan and replan_conflict_windows: (idx [K] int64, t0 [K], no
    [K (N - K), 2] int32 = (new i, old j) with j not in idx, nn [K (K - 1) / 2, 2] int32 = (new i, new j), i < j)."""
    import torch
    n, dev = dur.shape[0], dur.device
    idx = torch.as_tensor(idx, dtype=torch.int64).to(dev).reshape(-1)
    K = int(idx.numel())
    if new_dur.shape[0] != K or new_coef.shape[0] != K:
        raise ValueError(f"{who}: new_coef, new_dur hold one path per entry of idx")
    if K and (int(idx.min()) < 0 or int(idx.max()) >= n or int(torch.unique(idx).numel()) != K):
        raise ValueError(f"{who}: idx holds distinct drone indices of the swarm")
    t0 = torch.as_tensor(t_r, dtype=torch.float64).to(dev)
    t0 = t0.expand(K).contiguous() if t0.dim() == 0 else t0.contiguous()
    if tuple(t0.shape) != (K,):
        raise ValueError(f"{who}: t_r is a number or one value per replanned drone")
    stays = torch.ones((n,), dtype=torch.bool, device=dev)
    stays[idx] = False
    old = torch.nonzero(stays, as_tuple=True)[0]
    loc = torch.arange(K, device=dev)
    no = torch.stack([loc.repeat_interleave(old.numel()), old.repeat(K)], dim=1).to(torch.int32).contiguous()
    ii, jj = torch.triu_indices(K, K, offset=1, device=dev)
    nn = torch.stack([ii, jj], dim=1).to(torch.int32).contiguous()
    return idx, t0, no, nn


def certify_replan(compute, coef, dur, idx, t_r, new_coef, new_dur, radius: float, new_status=None) -> ReplanClearanceResult:
    """Certify replanned paths next to the paths that stay, in continuous time.

    The drones `idx` [K] (distinct swarm indices) leave the swarm's paths `coef`, `dur` at `t_r` -- a number, or one
    value per replanned drone [K], on the swarm's clock -- for `new_coef` [K, M', 4, nc], `new_dur` [K, M'], whose clock
    starts at `t_r` (what `replan` returns for those drones).  Every (new i, old j) pair with j not in `idx` and every
    (new i, new j) pair with i < j goes through `compute.cross_clearance` (msnap_cross_clearance_device) with the
    offsets `t_r`: the window of a pair is the time both fly, from the later start.  A drone that keeps its path is
    certified against the new path only; its own pairs with other such drones are `certify_clearance`'s.

    There is no sampled pre-filter: the pair count is K x N (K (N - K) + K (K - 1) / 2), which is small for the few
    drones a replan touches and grows with the swarm.  One rank only.  Raises on failed drones (`new_status` != 0,
    non-finite coefficients, durations <= 0), as `certify_clearance` does."""
    import torch
    if not (radius >= 0.0):
        raise ValueError("certify_replan: radius >= 0")
    if new_status is not None and int(new_status.abs().sum()) != 0:
        raise ValueError("certify_replan: the replan reported failed drones (status != 0)")
    idx, t0, no, nn = _replan_pairs("certify_replan", dur, idx, t_r, new_coef, new_dur)
    K, dev = int(idx.numel()), dur.device
    outs = []
    if no.shape[0]:
        outs.append(tuple(x.clone() for x in compute.cross_clearance(new_coef, new_dur, coef, dur, no, t0_a=t0)))
    if nn.shape[0]:
        outs.append(tuple(x.clone() for x in compute.cross_clearance(new_coef, new_dur, new_coef, new_dur, nn, t0_a=t0,
                                                                     t0_b=t0)))
    certified = torch.full((K,), float("inf"), dtype=torch.float64, device=dev)
    hit = torch.zeros((K,), dtype=torch.bool, device=dev)
    undecided = torch.zeros((K,), dtype=torch.bool, device=dev)
    if not outs:
        empty = torch.zeros((0,), dtype=torch.float64, device=dev)
        return ReplanClearanceResult(certified, hit, undecided, torch.zeros((0, 2), dtype=torch.int32, device=dev),
                                     torch.zeros((0,), dtype=torch.bool, device=dev), empty, empty, empty)
    md, tm, lower, pstat = (torch.cat([o[k] for o in outs]) for k in range(4))
    if int(pstat.abs().sum()) != 0:
        raise ValueError("certify_replan: msnap_cross_clearance reported failed pairs")
    p_hit = md < 2.0 * radius
    p_und = (~p_hit) & (lower < 2.0 * radius)
    # the replanned drones a pair counts for: its first member, and its second where that one is replanned too
    who = torch.cat([no[:, 0], nn[:, 0], nn[:, 1]]).to(torch.int64)
    P0 = no.shape[0]
    take = lambda x: torch.cat([x, x[P0:]])      # noqa: E731
    certified.scatter_reduce_(0, who, take(lower), reduce="amin", include_self=True)
    hit[who[take(p_hit)]] = True
    undecided[who[take(p_und)]] = True
    undecided &= ~hit
    pairs = torch.cat([torch.stack([idx[no[:, 0].to(torch.int64)], no[:, 1].to(torch.int64)], dim=1),
                       idx[nn.to(torch.int64)].reshape(-1, 2)]).to(torch.int32)
    new_new = torch.arange(pairs.shape[0], device=dev) >= P0
    return ReplanClearanceResult(certified, hit, undecided, pairs, new_new, md, tm, lower)


# ---- conflict windows: from when a pair is too close, and the hand-over time of a replan that still avoids it --------
@dataclass
class ConflictWindowResult:
    pairs: object             # [P, 2] int32, swarm indices: the pairs that went through the conflict-window entry
    # per pair [P], msnap_pair_conflict_window's outputs (include/msnap.h): clear is proven on [S, t_clear_until) and
    # (t_clear_from, W]; t_first / t_last are the earliest / latest conflict found (+inf / -inf: none)
    t_clear_until: object
    t_first: object
    d_first: object
    t_last: object
    d_last: object
    t_clear_from: object
    # per drone (conflict_windows: [N]; replan_conflict_windows: [K], in the order of `idx`): the earliest t_clear_until
    # over the drone's pairs -- until then the drone is proven clear of every listed partner --, +inf for a drone
    # without a pair that is in conflict or undecided
    first_conflict: object


def _window_result(pairs, outs, who, n_who):
    """ConflictWindowResult from the entry's outputs; `who` [Q] int64 indices into the per-drone array of length n_who
    and the positions `take` [Q] of their pairs in the list."""
    import torch
    idx, take = who
    cu = outs[0]
    first = torch.full((n_who,), float("inf"), dtype=torch.float64, device=cu.device)
    if idx.numel():
        first.scatter_reduce_(0, idx, cu[take], reduce="amin", include_self=True)
    return ConflictWindowResult(pairs, *outs[:6], first)


def conflict_windows(compute, clearance_result, coef, dur, radius: float, t_res: float = 1e-6) -> ConflictWindowResult:
    """From when the pairs that `certify_clearance` could not clear are closer than 2 radius.

    The pairs of `clearance_result` (a ClearanceResult) whose `pair_lower` < 2 radius -- hits and undecided ones -- go
    through `compute.conflict_window` (msnap_pair_conflict_window_device) with threshold = 2 radius.  `first_conflict`
    [N] is per drone the earliest `t_clear_until` over its pairs: `latest_replan_time` turns it into a hand-over time."""
    import torch
    if not (radius >= 0.0):
        raise ValueError("conflict_windows: radius >= 0")
    n = dur.shape[0]
    keep = clearance_result.pair_lower < 2.0 * radius
    pairs = clearance_result.pairs[keep].to(torch.int32).contiguous()
    outs = tuple(x.clone() for x in compute.conflict_window(coef, dur, pairs, 2.0 * radius, t_res))
    if pairs.shape[0] and int(outs[6].abs().sum()) != 0:
        raise ValueError("conflict_windows: msnap_pair_conflict_window reported failed pairs")
    both = pairs.to(torch.int64).reshape(-1)                          # a0 b0 a1 b1 ...
    take = torch.arange(pairs.shape[0], device=both.device).repeat_interleave(2)
    return _window_result(pairs, outs, (both, take), n)


def latest_replan_time(result, margin: float):
    """Per drone the latest hand-over time t_r of a replan that starts `margin` seconds before the drone's first
    conflict: first_conflict - margin, not below 0 (+inf for a drone without a conflict).  Hand it to `replan`.
    `result`: a ConflictWindowResult, a MeshConflictWindowResult or a GeofenceWindowResult (`geofence_windows`: there
    first_conflict is the earliest time FOUND outside the fence, to within t_res of the proven `inside_until` when the
    search closed; an undecided graze has +inf here and a finite `inside_until`)."""
    if not (margin >= 0.0):
        raise ValueError("latest_replan_time: margin >= 0")
    return (result.first_conflict - margin).clamp(min=0.0)


def replan_conflict_windows(compute, coef, dur, idx, t_r, new_coef, new_dur, radius: float,
                            t_res: float = 1e-6) -> ConflictWindowResult:
    """`conflict_windows` beside `certify_replan`: the pairs of `certify_replan` (every (new i, old j), then every (new
    i, new j) with i < j; swarm indices in `pairs`) through `compute.cross_conflict_window`
    (msnap_cross_conflict_window_device) with the offsets `t_r` and threshold = 2 radius.  `first_conflict` [K] is per
    replanned drone, on the swarm's clock."""
    import torch
    if not (radius >= 0.0):
        raise ValueError("replan_conflict_windows: radius >= 0")
    idx, t0, no, nn = _replan_pairs("replan_conflict_windows", dur, idx, t_r, new_coef, new_dur)
    K, dev = int(idx.numel()), dur.device
    outs = []
    if no.shape[0]:
        outs.append(tuple(x.clone() for x in compute.cross_conflict_window(new_coef, new_dur, coef, dur, no,
                                                                           2.0 * radius, t_res, t0_a=t0)))
    if nn.shape[0]:
        outs.append(tuple(x.clone() for x in compute.cross_conflict_window(new_coef, new_dur, new_coef, new_dur, nn,
                                                                           2.0 * radius, t_res, t0_a=t0, t0_b=t0)))
    if not outs:
        empty = torch.zeros((0,), dtype=torch.float64, device=dev)
        return ConflictWindowResult(torch.zeros((0, 2), dtype=torch.int32, device=dev), *([empty] * 6),
                                    torch.full((K,), float("inf"), dtype=torch.float64, device=dev))
    cat = tuple(torch.cat([o[k] for o in outs]) for k in range(7))
    if int(cat[6].abs().sum()) != 0:
        raise ValueError("replan_conflict_windows: msnap_cross_conflict_window reported failed pairs")
    P0, P = no.shape[0], no.shape[0] + nn.shape[0]
    who = torch.cat([no[:, 0], nn[:, 0], nn[:, 1]]).to(torch.int64)
    take = torch.cat([torch.arange(P, device=dev), torch.arange(P0, P, device=dev)])
    pairs = torch.cat([torch.stack([idx[no[:, 0].to(torch.int64)], no[:, 1].to(torch.int64)], dim=1),
                       idx[nn.to(torch.int64)].reshape(-1, 2)]).to(torch.int32)
    return _window_result(pairs, cat, (who, take), K)


# ---- mesh conflict windows: from when a drone is too close to the mesh, for the same hand-over time --------------------
@dataclass
class MeshConflictWindowResult:
    idx: object               # [K] int64: the drones that went through the mesh conflict-window entry
    # per drone [N], msnap_mesh_conflict_window's outputs (include/msnap.h): clear is proven on [0, t_clear_until) and
    # (t_clear_from, W]; t_first / t_last are the earliest / latest conflict found, d_* and tri_* the sweep's distance
    # and triangle there.  A drone that did not go through the entry has the certified-clear values
    # (+inf, +inf, +inf, -1, -inf, +inf, -1, -inf)
    t_clear_until: object
    t_first: object
    d_first: object
    tri_first: object
    t_last: object
    d_last: object
    tri_last: object
    t_clear_from: object
    # [N]: t_clear_until -- until then the drone is proven clear of the mesh --, +inf for a drone without a conflict
    # or an undecided graze.  `latest_replan_time` reads this field alone
    first_conflict: object


def mesh_conflict_windows(compute, mesh_result, coef, dur, tris, radius: float,
                          t_res: float = 1e-6) -> MeshConflictWindowResult:
    """From when until when the drones that `certify_mesh_clearance` could not clear are closer than radius to the mesh.

    The drones of `mesh_result` (a MeshClearanceResult) whose `certified_lower` < radius -- hits and undecided ones -- go
    through `compute.mesh_conflict_window` (msnap_mesh_conflict_window_device) with threshold = radius.
    `first_conflict` [N] is the drone's `t_clear_until`: `latest_replan_time` turns it into a hand-over time."""
    import torch
    if not (radius >= 0.0):
        raise ValueError("mesh_conflict_windows: radius >= 0")
    n, dev = dur.shape[0], dur.device
    idx = torch.nonzero(mesh_result.certified_lower < radius, as_tuple=True)[0]
    inf = float("inf")
    fills = (inf, inf, inf, -1, -inf, inf, -1, -inf)
    full = [torch.full((n,), f, dtype=torch.int32 if isinstance(f, int) else torch.float64, device=dev) for f in fills]
    if idx.numel():
        outs = compute.mesh_conflict_window(coef[idx].contiguous(), dur[idx].contiguous(), tris, radius, t_res)
        if int(outs[8].abs().sum()) != 0:
            raise ValueError("mesh_conflict_windows: msnap_mesh_conflict_window reported failed drones")
        for dst, src in zip(full, outs[:8]):
            dst[idx] = src
    return MeshConflictWindowResult(idx, *full, full[0].clone())


# ---- half-space windows: when a path leaves a geofence, and a safe flight corridor as a chain of polytopes -------------
@dataclass
class GeofenceWindowResult:
    idx: object               # [K] int64: the drones that went through the half-space window entry
    queries: object           # [Q, 2] int32: (drone, constraint -- an index into the GeofenceResult's `normals`)
    # per query [Q], msnap_halfspace_window's outputs (include/msnap.h): inside is proven on [0, t_inside_until) and
    # (t_inside_from, total]; t_first / t_last are the earliest / latest time found outside (+inf / -inf: none), v_*
    # the constraint's n.p there
    t_inside_until: object
    t_first: object
    v_first: object
    t_last: object
    v_last: object
    t_inside_from: object
    # per drone [N]; a drone that did not go through the entry has (+inf, -inf, +inf, -inf, -1)
    first_conflict: object    # the earliest t_first over the drone's constraints (+inf: none found): `latest_replan_time`
    last_conflict: object     # the latest t_last (-inf: none found)
    inside_until: object      # the earliest t_inside_until: until then the drone is proven inside every constraint
    inside_from: object       # the latest t_inside_from: after it the drone is proven inside every constraint
    first_broken: object      # int64: the constraint whose t_first is first_conflict (-1: none)


def _drone_plane_queries(idx, first, count):
    """int64 (row [Q], plane [Q]): for row r of `idx`, the `count[r]` planes from `first[r]` on; row indexes `idx`."""
    import torch
    total = int(count.sum())
    row = torch.repeat_interleave(torch.arange(idx.numel(), device=idx.device), count, output_size=total)
    within = torch.arange(total, device=idx.device) - (torch.cumsum(count, 0) - count)[row]
    return row, first[row] + within


def _earliest(values, row, n_rows, fill, largest=False):
    """Per row the smallest (largest) of `values` [Q] and the first query that attains it (-1: the row has none)."""
    import torch
    Q = values.numel()
    best = torch.full((n_rows,), fill, dtype=values.dtype, device=values.device)
    arg = torch.full((n_rows,), -1, dtype=torch.int64, device=values.device)
    if Q:
        best.scatter_reduce_(0, row, values, reduce="amax" if largest else "amin", include_self=True)
        at = torch.where(values == best[row], torch.arange(Q, device=values.device), torch.full_like(row, Q))
        first = torch.full((n_rows,), Q, dtype=torch.int64, device=values.device)
        first.scatter_reduce_(0, row, at, reduce="amin", include_self=True)
        arg = torch.where(first < Q, first, arg)
    return best, arg


def geofence_windows(compute, geofence_result, coef, dur, t_res: float = 1e-6) -> GeofenceWindowResult:
    """From when until when the drones that `certify_geofence` could not certify are outside the fence.

    The `outside` and `undecided` drones of `geofence_result` (a GeofenceResult) go against every finite constraint of it
    -- `normals` / `limits`, which carry the radius already -- through `compute.halfspace_window`
    (msnap_halfspace_window_device) over their whole flight.  Per drone: `first_conflict` / `last_conflict`, the earliest
    and latest time found outside any constraint; `inside_until` / `inside_from`, the proven ranges; `first_broken`, the
    constraint that is broken first.  `latest_replan_time` turns `first_conflict` into a hand-over time."""
    import torch
    n, dev = dur.shape[0], dur.device
    idx = torch.nonzero(geofence_result.outside | geofence_result.undecided, as_tuple=True)[0]
    C = int(geofence_result.limits.numel())
    planes = torch.cat([geofence_result.normals.reshape(-1, 3), geofence_result.limits.reshape(-1, 1)], dim=1).contiguous()
    row, con = _drone_plane_queries(idx, torch.zeros_like(idx), torch.full_like(idx, C))
    queries = torch.stack([idx[row], con], dim=1).to(torch.int32).contiguous()
    outs = tuple(x.clone() for x in compute.halfspace_window(coef, dur, planes, queries, t_res))
    if queries.shape[0] and int(outs[6].abs().sum()) != 0:
        raise ValueError("geofence_windows: msnap_halfspace_window reported failed queries")
    inf = float("inf")
    who = idx[row]
    first, arg = _earliest(outs[1], who, n, inf)
    last, _ = _earliest(outs[3], who, n, -inf, largest=True)
    until, _ = _earliest(outs[0], who, n, inf)
    frm, _ = _earliest(outs[5], who, n, -inf, largest=True)
    broken = torch.where(torch.isfinite(first) & (arg >= 0), con[arg.clamp(min=0)] if con.numel() else arg, torch.full_like(arg, -1))
    return GeofenceWindowResult(idx, queries, *outs[:6], first, last, until, frm, broken)


CORRIDOR_INSIDE, CORRIDOR_OUTSIDE, CORRIDOR_UNDECIDED, CORRIDOR_FAILED = 0, 1, 2, 3


@dataclass
class CorridorResult:
    verdict: object           # [N] int8: CORRIDOR_INSIDE / _OUTSIDE / _UNDECIDED / _FAILED
    proven_until: object      # [N] the time up to which the drone is proven inside the corridor (INSIDE: its total; NaN: failed)
    stage: object             # [N] int64: the stage of the drone's chain at which it stopped (-1: inside or failed)
    plane: object             # [N] int64: the plane (index into `planes`) that stopped it (-1: inside or failed)
    first_conflict: object    # [N] that plane's t_first (+inf: none found, inside, failed)
    value: object             # [N] its v_first, n.p at first_conflict (-inf: none found; NaN: inside, failed)
    handover: object          # [N, L] h_i, the time from which stage i had to hold (NaN: the stage was not reached)


def certify_corridor(compute, coef, dur, planes, poly_offsets, chain, radius: float = 0.0, t_res: float = 1e-6,
                     status=None) -> CorridorResult:
    """Certify in continuous time that every drone of `coef`, `dur` flies through a safe flight corridor: a chain of
    overlapping convex polytopes of free space, in each of which the path must stay until it is inside the next.

    `planes` [Q, 4] = (n, b), finite, meaning n.x <= b; polytope p is planes[poly_offsets[p]:poly_offsets[p + 1]] (an
    empty polytope is all of space); `chain` is [L] (shared by all drones) or [N, L] int64 polytope ids, -1 padding the
    tail, at least one stage per drone.  A drone is a sphere of `radius`, which moves each limit by radius |n|.
    L rounds, each one call of `compute.halfspace_window` (msnap_halfspace_window_device) over the drones still running,
    h_0 = 0.  In round i the planes of stage i are queried on [h_i, total]; stay_i is the smallest t_inside_until:
      all +inf                       the drone is certified inside through the end: INSIDE;
      some t_inside_until == h_i     the drone is not proven inside stage i at the hand-over: it stops.  What stopped it
                                     is the plane of stage i - 1 that it left before it was inside stage i (i = 0: the
                                     plane of stage 0 it starts outside of);
      the last stage of its chain    it stops there, proven inside until stay_i;
      otherwise                      h_{i+1} = max(h_i, stay_i - t_res), the latest time proven inside stage i -- the right
                                     choice for a chain: stage i + 1 has to hold from there.
    A drone that stopped names that `stage` and its `plane` with the smallest t_inside_until, whose t_first / v_first are
    `first_conflict` / `value`.  It is OUTSIDE only when that is definite: the position of the drone at `first_conflict`
    (compute.eval_state: msnap_eval_flat's lookup and arithmetic) violates at least one plane of EVERY polytope of its
    chain, by the unfused (n_x x + n_y y) + n_z z > limit.  Any other drone that stopped is UNDECIDED.  FAILED is as in
    certify_geofence: status != 0 (`status`: the solve's; or the entry's), nothing is certified.

    One rank: every drone is checked on its own, so a sharded swarm calls this per shard."""
    import torch
    if not (radius >= 0.0):
        raise ValueError("certify_corridor: radius >= 0")
    if not (t_res > 0.0 and t_res < float("inf")):
        raise ValueError("certify_corridor: t_res > 0 and finite")
    n, dev = dur.shape[0], dur.device
    f64 = dict(dtype=torch.float64, device=dev)
    pl = torch.as_tensor(planes, dtype=torch.float64).to(dev).reshape(-1, 4).clone()
    if not bool(torch.isfinite(pl).all()):
        raise ValueError("certify_corridor: planes must be finite")
    off = torch.as_tensor(poly_offsets, dtype=torch.int64).to(dev).reshape(-1)
    if off.numel() < 2 or int(off[0]) != 0 or int(off[-1]) != pl.shape[0] or bool((off[1:] < off[:-1]).any()):
        raise ValueError("certify_corridor: poly_offsets must rise from 0 to the number of planes")
    n_poly = off.numel() - 1
    ch = torch.as_tensor(chain, dtype=torch.int64).to(dev)
    if ch.dim() == 1:
        ch = ch[None, :].expand(n, -1)
    if ch.dim() != 2 or ch.shape[0] != n or ch.shape[1] < 1:
        raise ValueError("certify_corridor: chain must be [L] or [N, L] with L >= 1")
    valid = ch >= 0
    if bool((ch < -1).any() | (ch >= n_poly).any() | (valid[:, 1:] & ~valid[:, :-1]).any() | ~valid[:, 0].all()):
        raise ValueError("certify_corridor: chain holds polytope ids, -1 only as padding of the tail, one stage at least")
    L = ch.shape[1]
    length = valid.sum(dim=1)
    pl[:, 3] = pl[:, 3] - radius * torch.linalg.vector_norm(pl[:, :3], dim=1)
    sizes = off[1:] - off[:-1]
    total = torch.zeros((n,), **f64)
    for k in range(dur.shape[1]):      # (the running sum, as msnap_eval_flat accumulates it)
        total = total + dur[:, k]

    bad = torch.zeros((n,), dtype=torch.bool, device=dev)
    if status is not None:
        bad |= torch.as_tensor(status).to(dev) != 0
    inf, nan = float("inf"), float("nan")
    h = torch.zeros((n,), **f64)
    proven = torch.zeros((n,), **f64)
    handover = torch.full((n, L), nan, **f64)
    stage = torch.full((n,), -1, dtype=torch.int64, device=dev)
    plane = torch.full((n,), -1, dtype=torch.int64, device=dev)
    first = torch.full((n,), inf, **f64)
    value = torch.full((n,), nan, **f64)
    left_plane, left_first, left_value = plane.clone(), first.clone(), value.clone()      # of the stage a drone left last
    inside = torch.zeros_like(bad)
    run = ~bad
    for i in range(L):
        idx = torch.nonzero(run, as_tuple=True)[0]
        if not idx.numel():
            break
        handover[idx, i] = h[idx]
        poly = ch[idx, i]
        row, qp = _drone_plane_queries(idx, off[poly], sizes[poly])
        queries = torch.stack([idx[row], qp], dim=1).to(torch.int32).contiguous()
        outs = compute.halfspace_window(coef, dur, pl, queries, t_res, t_from=h[idx][row].contiguous())
        iu, tf, vf, st = outs[0].clone(), outs[1].clone(), outs[2].clone(), outs[6]
        failed = torch.zeros((idx.numel(),), dtype=torch.bool, device=dev)
        if queries.shape[0]:
            failed.index_put_((row,), st != 0, accumulate=True)
        iu = torch.where(torch.isnan(iu), torch.full_like(iu, inf), iu)
        stay, arg = _earliest(iu, row, idx.numel(), inf)
        hi = h[idx]
        done = ~failed & torch.isinf(stay)
        stop = ~failed & ~done & ((stay == hi) | (length[idx] - 1 == i))
        go = ~failed & ~done & ~stop
        bad[idx[failed]] = True
        inside[idx[done]] = True
        # what is proven: stage i up to stay_i, unless the drone is not inside it at the hand-over
        adv = (go | stop) & (stay > hi)
        proven[idx[adv]] = torch.maximum(proven[idx[adv]], stay[adv])
        # where it stopped: this stage's plane with the smallest t_inside_until -- or, when the hand-over into this
        # stage failed, the plane of the stage before that the drone left too early
        back = stop & (stay == hi) & (i > 0)
        here = stop & ~back
        s_i, s_q = idx[here], arg[here]
        stage[s_i], plane[s_i], first[s_i], value[s_i] = i, qp[s_q], tf[s_q], vf[s_q]
        b_i = idx[back]
        stage[b_i], plane[b_i], first[b_i], value[b_i] = i - 1, left_plane[b_i], left_first[b_i], left_value[b_i]
        handover[b_i, i] = nan      # (stage i was not reached)
        g_i, g_q = idx[go], arg[go]
        left_plane[g_i], left_first[g_i], left_value[g_i] = qp[g_q], tf[g_q], vf[g_q]
        h[g_i] = torch.maximum(hi[go], stay[go] - t_res)
        run = torch.zeros_like(run)
        run[idx[go]] = True

    stopped = stage >= 0
    outside = torch.zeros_like(bad)
    sidx = torch.nonzero(stopped & torch.isfinite(first), as_tuple=True)[0]
    if sidx.numel():
        pos, _ = compute.eval_state(coef[sidx].contiguous(), dur[sidx].contiguous(), first[sidx].contiguous())
        x, y, z = pos[:, 0:1], pos[:, 1:2], pos[:, 2:3]
        val = (pl[None, :, 0] * x + pl[None, :, 1] * y) + pl[None, :, 2] * z      # [S, Q], every operation rounded once
        viol = (val > pl[None, :, 3]).to(torch.float64)
        pid = torch.repeat_interleave(torch.arange(n_poly, device=dev), sizes, output_size=pl.shape[0])
        per_poly = torch.zeros((sidx.numel(), n_poly), **f64).index_add_(1, pid, viol) > 0
        along = per_poly.gather(1, ch[sidx].clamp(min=0)) | ~valid[sidx]
        outside[sidx] = along.all(dim=1)
    verdict = torch.full((n,), CORRIDOR_UNDECIDED, dtype=torch.int8, device=dev)
    verdict[inside], verdict[outside], verdict[bad] = CORRIDOR_INSIDE, CORRIDOR_OUTSIDE, CORRIDOR_FAILED
    proven = torch.where(inside, total, proven)
    proven = torch.where(bad, torch.full_like(proven, nan), proven)
    for x, fill in ((stage, -1), (plane, -1), (first, inf), (value, nan)):
        x[bad] = fill
    return CorridorResult(verdict, proven, stage, plane, first, value, handover)
