"""Context: the Python face of one msnap_ctx (one GPU, one HIP stream).

Host entry points take / return NumPy arrays (the library stages them through
device buffers).  ``*_device`` entry points take objects exposing
``data_ptr()`` (torch CUDA tensors) and are asynchronous on the context's
stream; torch is plumbing for device memory only and is imported lazily.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

from . import _lib

ST_OK, ST_SINGULAR, ST_TIMES, ST_NONFINITE, ST_PAIR = 0, 1, 2, 3, 4
RETIME_FIT, RETIME_COMMON = 1, 2      # msnap_retime_flags
STATUS_TEXT = {
    ST_OK: "ok",
    ST_SINGULAR: "singular system",
    ST_TIMES: "times not strictly increasing",
    ST_NONFINITE: "non-finite waypoint or time",
    ST_PAIR: "pair index out of range, or a drone paired with itself",
}


def _ptr(x):
    """Device pointer of a torch tensor (or a raw int address)."""
    if x is None:
        return None
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    return ctypes.c_void_p(x.data_ptr())


def _host(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


class _PinnedBlock:
    """Owner of one msnap_host_alloc block; arrays made by pinned_empty keep it alive."""

    def __init__(self, nbytes):
        self._lib = _lib.load()
        p = ctypes.c_void_p()
        _lib.check(self._lib, None, self._lib.msnap_host_alloc(ctypes.byref(p), max(int(nbytes), 1)))
        self.ptr, self.nbytes = p.value, int(nbytes)

    def __del__(self):
        ptr, self.ptr = getattr(self, "ptr", None), None
        if ptr:
            self._lib.msnap_host_free(ctypes.c_void_p(ptr))


def pinned_empty(shape, dtype=np.float64):
    """Uninitialised NumPy array in page-locked host memory (msnap_host_alloc).  Passing such
    arrays to solve_batch / solve_grid (inputs and `out=`) lets the copy engines move them
    directly, overlapped with the kernel; the memory is released with the last view."""
    dtype = np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(int(s) for s in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    block = _PinnedBlock(nbytes)
    buf = (ctypes.c_char * max(nbytes, 1)).from_address(block.ptr)
    buf._msnap_owner = block          # the ctypes buffer is the array's base and holds the block
    return np.frombuffer(buf, dtype=dtype, count=nbytes // dtype.itemsize).reshape(shape)


def _out_arrays(out, shapes):
    """Validate caller-provided (coef, dur, status) or allocate them."""
    dtypes = (np.float64, np.float64, np.int32)
    if out is None:
        return tuple(np.empty(s, dtype=d) for s, d in zip(shapes, dtypes))
    if len(out) != 3:
        raise ValueError("out must be (coef, dur, status)")
    for a, s, d in zip(out, shapes, dtypes):
        if not isinstance(a, np.ndarray) or a.shape != tuple(s) or a.dtype != d or not a.flags.c_contiguous \
                or not a.flags.writeable:
            raise ValueError(f"out arrays must be writable C-contiguous {np.dtype(d).name} of shape {tuple(s)}")
    return tuple(out)


def _waypoints_times(wp, t):
    """Validated host (wp [N, m, 4], t [N, m] or shared [m]) -> wp, its pointer, t, its pointer, N, m, shared."""
    wp, pwp = _host(wp, np.float64)
    t, pt = _host(t, np.float64)
    if wp.ndim != 3 or wp.shape[2] != 4:
        raise ValueError("wp must be [N, m, 4]")
    N, m, _ = wp.shape
    shared = int(t.ndim == 1)
    if (shared and t.shape != (m,)) or (not shared and t.shape != (N, m)):
        raise ValueError("t must be [N, m] or [m]")
    return wp, pwp, t, pt, N, m, shared


def _weights(weights):
    """The host array of the 4 axis weights (x, y, z, yaw) and its address; the caller holds the array while the
    library reads it.  The address is taken as a number: `_host`'s `data_as` costs several times as much, on every
    call of a device entry, and that pays for the frame the allocators' shared bodies add to such a call
    (profiles/timeopt_call_record.md)."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (4,):
        raise ValueError("weights must hold 4 values")
    return w, ctypes.c_void_p(w.ctypes.data)


class Context:
    """One msnap context (include/msnap.h: msnap_create / msnap_destroy)."""

    def __init__(self, device_id: int = 0, order: int = 7, max_segments: int = 256):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        self._lock = threading.Lock()   # a context is not re-entrant (msnap.h)
        self._glock = threading.RLock()  # the prepared grid is context state: prepare + solve as one step
        rc = self._lib.msnap_create(ctypes.byref(self._h), int(device_id), int(order), int(max_segments))
        if rc != 0:
            self._h = ctypes.c_void_p()
            _lib.check(self._lib, None, rc)
        self.device_id = int(device_id)
        self.order = int(order)
        self.ncoef = self.order + 1
        self.max_segments = int(max_segments)

    # ---- lifetime -------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.msnap_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc):
        _lib.check(self._lib, self._h, rc)

    # ---- launch-geometry options (msnap_set_option) ------------------------------
    def set_option(self, name: str, value: int):
        """Launch-geometry knob of this context (include/msnap.h lists the names), e.g.
        set_option("solve_grid_waves", 5) makes every wave of the large-batch solve walk
        several tiles on a batch small enough for the oracle."""
        with self._lock:
            self._ck(self._lib.msnap_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = ctypes.c_long()
        self._ck(self._lib.msnap_get_option(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def last_kernel(self) -> str:
        """Kernel instance the last solve call of this context launched (msnap_last_kernel)."""
        return self._lib.msnap_last_kernel(self._h).decode()

    def _coef_dur(self, coef, dur):
        """Validated host (coef [N,M,4,ncoef], dur [N,M]) and their pointers."""
        coef, pc = _host(coef, np.float64)
        dur, pd = _host(dur, np.float64)
        if dur.ndim != 2:
            raise ValueError("dur must be [N, M]")
        N, M = dur.shape
        if coef.shape != (N, M, 4, self.ncoef):
            raise ValueError(f"coef must be [N, M, 4, {self.ncoef}] = {(N, M, 4, self.ncoef)} for this "
                             f"order-{self.order} context, got {coef.shape}")
        return coef, pc, dur, pd, N, M

    def _mode_max_segments(self, fn):
        """What the library's `fn` (a *_max_segments entry) allows at this context's order, and at most max_segments."""
        return min(int(fn(self.order)), self.max_segments)

    def _optimize_times(self, entry, wp, t, states, weights, time_weight, min_fraction, max_iter, tol, gates=()):
        """The host allocators' one body: `entry` names the library's entry of the mode (looked up after the shape
        checks, which need no library), `states` is its (start, end), `time_weight` its (time_weight,) and `gates` the
        pointers of its (fix, via), behind the states in the call -- () where it takes none; the other arguments and
        the result tuple as optimize_times."""
        wp, pwp, t, pt, N, m, shared = _waypoints_times(wp, t)
        w, pw = _weights(weights)
        kts = []      # (the converted arrays and their pointers, as _host gives them)
        for kt in time_weight:
            kt = np.asarray(kt, dtype=np.float64)
            if kt.ndim == 0:
                kt = np.full((N,), float(kt))
            if kt.shape != (N,):
                raise ValueError("time_weight must be a number or [N]")
            kts.append(_host(kt, np.float64))
        ends = [self._state_block(x, N, name) for x, name in zip(states, ("start", "end"))]
        M = m - 1
        t_out = np.empty((N, m), dtype=np.float64)
        coef = np.empty((N, max(M, 0), 4, self.ncoef), dtype=np.float64)
        dur = np.empty((N, max(M, 0)), dtype=np.float64)
        status = np.empty((N,), dtype=np.int32)
        cost = np.empty((N, 2), dtype=np.float64)
        pg = np.empty((N,), dtype=np.float64)
        iters = np.empty((N,), dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        with self._lock:
            self._ck(getattr(self._lib, entry)(
                self._h, N, M, pwp, pt, shared, *(px for _, px in ends), *gates, pw, *(pk for _, pk in kts),
                float(min_fraction), int(max_iter), float(tol), vp(t_out), vp(coef), vp(dur), vp(status), vp(cost),
                vp(pg), vp(iters)))
        return t_out, coef, dur, status, {"cost": cost, "pg": pg, "iters": iters}

    def _optimize_times_device(self, entry, n_drones, n_seg, wp, t, shared_times, states, weights, time_weight,
                               min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters):
        """The device allocators' one body: `entry` names the library's _device entry of the mode, `states` holds the
        pointers of its (start, end) and `time_weight` that of its time weight -- () where it takes none."""
        w, pw = _weights(weights)
        with self._lock:
            self._ck(getattr(self._lib, entry)(
                self._h, int(n_drones), int(n_seg), _ptr(wp), _ptr(t), int(bool(shared_times)), *states, pw,
                *time_weight, float(min_fraction), int(max_iter), float(tol), _ptr(t_out), _ptr(coef), _ptr(dur),
                _ptr(status), _ptr(cost), _ptr(pg), _ptr(iters)))

    # ---- stream / timing ------------------------------------------------------
    def set_stream(self, hip_stream: int | None):
        """Launch on an external hipStream_t (0 / None = the HIP null stream)."""
        with self._lock:
            self._ck(self._lib.msnap_set_stream(self._h, ctypes.c_void_p(hip_stream or 0)))

    def use_own_stream(self):
        with self._lock:
            self._ck(self._lib.msnap_use_own_stream(self._h))

    def stream(self) -> int:
        return int(self._lib.msnap_get_stream(self._h) or 0)

    def sync(self):
        with self._lock:
            self._ck(self._lib.msnap_sync(self._h))

    def timer_start(self):
        self._ck(self._lib.msnap_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = ctypes.c_float()
        self._ck(self._lib.msnap_timer_stop(self._h, ctypes.byref(ms)))
        return float(ms.value)

    # ---- a1/a2 solve ----------------------------------------------------------
    def solve_batch(self, wp, t, out=None):
        """wp [N, m, 4], t [N, m] or shared [m] (host) ->
        coef [N, M, 4, ncoef], dur [N, M], status [N] int32.
        `out=(coef, dur, status)` writes into caller-owned arrays (e.g. from pinned_empty)."""
        wp, pwp, t, pt, N, m, shared = _waypoints_times(wp, t)
        M = m - 1
        coef, dur, status = _out_arrays(out, ((N, max(M, 0), 4, self.ncoef), (N, max(M, 0)), (N,)))
        with self._lock:
            self._ck(self._lib.msnap_solve_batch(
                self._h, N, M, pwp, pt, shared, coef.ctypes.data_as(ctypes.c_void_p),
                dur.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p)))
        return coef, dur, status

    def solve_batch_device(self, n_drones, n_seg, wp, t, shared_times, coef, dur, status):
        with self._lock:
            self._ck(self._lib.msnap_solve_batch_device(
                self._h, int(n_drones), int(n_seg), _ptr(wp), _ptr(t), int(bool(shared_times)),
                _ptr(coef), _ptr(dur), _ptr(status)))

    # ---- shared time grid (K2: fp64 MFMA GEMM) ---------------------------------
    def prepare_grid(self, t):
        """Build the operator of the shared time grid t [m] (host array)."""
        t, pt = _host(t, np.float64)
        if t.ndim != 1 or t.shape[0] < 2:
            raise ValueError("t must be [m], m >= 2")
        with self._glock:
            with self._lock:
                self._ck(self._lib.msnap_grid_prepare(self._h, t.shape[0] - 1, pt))
            self._grid_host = t.copy()

    def ensure_grid(self, t):
        """prepare_grid(t) unless the context already holds exactly this grid."""
        t = np.ascontiguousarray(t, dtype=np.float64)
        with self._glock:
            g = getattr(self, "_grid_host", None)
            if g is None or g.shape != t.shape or not np.array_equal(g, t):
                self.prepare_grid(t)

    def solve_on_grid(self, t, wp, out=None):
        """ensure_grid(t) + solve_grid(wp) as one step: two threads sharing a context (the node's
        callback1 / callback2) cannot swap the grid between the two calls."""
        with self._glock:
            self.ensure_grid(t)
            return self.solve_grid(wp, out=out)

    def prepare_grid_device(self, n_seg, t):
        with self._glock:     # (under the grid lock like prepare_grid: solve_on_grid must not see a half-updated grid)
            with self._lock:
                self._ck(self._lib.msnap_grid_prepare_device(self._h, int(n_seg), _ptr(t)))
            self._grid_host = None

    def grid_segments(self) -> int:
        """Segments of the grid this context holds (msnap_grid_segments; 0: none prepared)."""
        n = int(self._lib.msnap_grid_segments(self._h))
        if n < 0:
            _lib.check(self._lib, self._h, n)
        return n

    def grid_waypoints(self) -> int:
        """Waypoints per drone of the grid this context was last prepared for (raises MSNAP_ENOGRID without one)."""
        n = self.grid_segments()
        if n == 0:
            _lib.check(self._lib, self._h, -7)
        return n + 1

    def release_graph_buffers(self) -> int:
        """Free the blocks kept alive for graphs captured before a buffer grew (msnap_release_graph_buffers): call
        once every graph that captured calls of this context is destroyed.  Returns the bytes released."""
        n = ctypes.c_size_t()
        with self._lock:
            self._ck(self._lib.msnap_release_graph_buffers(self._h, ctypes.byref(n)))
        return int(n.value)

    def solve_grid(self, wp, out=None):
        """wp [N, m, 4] on the prepared grid -> coef, dur, status (as solve_batch)."""
        with self._glock:
            wp, pwp = _host(wp, np.float64)
            m = self.grid_waypoints()
            if wp.ndim != 3 or wp.shape[1:] != (m, 4):
                raise ValueError(f"wp must be [N, {m}, 4] for the prepared grid")
            N, M = wp.shape[0], m - 1
            coef, dur, status = _out_arrays(out, ((N, M, 4, self.ncoef), (N, M), (N,)))
            with self._lock:
                self._ck(self._lib.msnap_solve_grid(self._h, N, M, pwp, coef.ctypes.data_as(ctypes.c_void_p),
                                                   dur.ctypes.data_as(ctypes.c_void_p),
                                                   status.ctypes.data_as(ctypes.c_void_p)))
            return coef, dur, status

    def solve_grid_device(self, n_drones, n_seg, wp, coef, dur, status):
        """Device pointers.  `n_seg` is the segment count the buffers were sized for: the library refuses
        (MSNAP_ESEGMENTS) a count that is not the prepared grid's instead of writing past them."""
        with self._lock:
            self._ck(self._lib.msnap_solve_grid_device(self._h, int(n_drones), int(n_seg), _ptr(wp), _ptr(coef),
                                                      _ptr(dur), _ptr(status)))

    # ---- a7 pack ---------------------------------------------------------------
    def pack_pol_matrix(self, coef, dur):
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        out = np.empty((N, M, 1 + 4 * self.ncoef), dtype=np.float32)
        with self._lock:
            self._ck(self._lib.msnap_pack_pol_matrix(self._h, N, M, pc, pd, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def pack_pol_matrix_device(self, n_drones, n_seg, coef, dur, out):
        with self._lock:
            self._ck(self._lib.msnap_pack_pol_matrix_device(self._h, int(n_drones), int(n_seg), _ptr(coef),
                                                           _ptr(dur), _ptr(out)))

    # ---- a8 formation transform -----------------------------------------------
    def formation_transform(self, rb_pose, offsets):
        rb, prb = _host(rb_pose, np.float64)
        off, poff = _host(offsets, np.float64)
        if rb.ndim != 2 or rb.shape[1] != 7 or off.ndim != 2 or off.shape[1] != 3:
            raise ValueError("rb_pose must be [P, 7], offsets [K, 3]")
        P, K = rb.shape[0], off.shape[0]
        out = np.empty((K, P, 7), dtype=np.float64)
        with self._lock:
            self._ck(self._lib.msnap_formation_transform(self._h, P, K, prb, poff,
                                                        out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def formation_transform_device(self, n_poses, n_offsets, rb_pose, offsets, out):
        with self._lock:
            self._ck(self._lib.msnap_formation_transform_device(self._h, int(n_poses), int(n_offsets),
                                                               _ptr(rb_pose), _ptr(offsets), _ptr(out)))

    # ---- a5 sampler ------------------------------------------------------------
    def sample(self, coef, dur, dt: float, n_samples: int, n_axes: int = 3):
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        pos = np.empty((N, int(n_samples), int(n_axes)), dtype=np.float64)
        with self._lock:
            self._ck(self._lib.msnap_sample(self._h, N, M, pc, pd, float(dt), int(n_samples), int(n_axes),
                                           pos.ctypes.data_as(ctypes.c_void_p)))
        return pos

    def sample_device(self, n_drones, n_seg, coef, dur, dt, n_samples, n_axes, pos):
        with self._lock:
            self._ck(self._lib.msnap_sample_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                  float(dt), int(n_samples), int(n_axes), _ptr(pos)))

    # ---- flatness evaluator (Trajectory.eval) -------------------------------------
    def eval_flat(self, coef, dur, ts):
        """coef [N,M,4,nc], dur [N,M], ts [S] -> out [N,S,13] = pos3 vel3 acc3 omega3 yaw."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        ts, pt = _host(ts, np.float64)
        if ts.ndim != 1:
            raise ValueError("ts must be [S]")
        S = ts.shape[0]
        out = np.empty((N, S, 13), dtype=np.float64)
        with self._lock:
            self._ck(self._lib.msnap_eval_flat(self._h, N, M, pc, pd, S, pt, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def eval_flat_device(self, n_drones, n_seg, coef, dur, n_samples, ts, out):
        with self._lock:
            self._ck(self._lib.msnap_eval_flat_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                     int(n_samples), _ptr(ts), _ptr(out)))

    # ---- snap cost ---------------------------------------------------------------------
    def snap_cost(self, coef, dur):
        """J = sum_seg int (p^(k))^2 dt per drone and axis -> [N, 4]."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        cost = np.empty((N, 4), dtype=np.float64)
        with self._lock:
            self._ck(self._lib.msnap_snap_cost(self._h, N, M, pc, pd, cost.ctypes.data_as(ctypes.c_void_p)))
        return cost

    def snap_cost_device(self, n_drones, n_seg, coef, dur, cost):
        with self._lock:
            self._ck(self._lib.msnap_snap_cost_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                     _ptr(cost)))

    # ---- time allocation (include/msnap.h: segment times optimised per drone) ---------------
    def snap_cost_grad(self, coef, dur):
        """-E per drone, segment and axis -> [N, M, 4] (msnap_snap_cost_grad): the derivative of the optimal cost
        by each duration when `coef` is the solve's result for `dur`."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        grad = np.empty((N, M, 4), dtype=np.float64)
        with self._lock:
            self._ck(self._lib.msnap_snap_cost_grad(self._h, N, M, pc, pd, grad.ctypes.data_as(ctypes.c_void_p)))
        return grad

    def snap_cost_grad_device(self, n_drones, n_seg, coef, dur, grad):
        with self._lock:
            self._ck(self._lib.msnap_snap_cost_grad_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                           _ptr(grad)))

    def optimize_times(self, wp, t, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200, tol=1e-4):
        """Per-drone optimisation of the interior knot times, waypoints and total duration kept
        (msnap_optimize_times): wp [N, m, 4], t [N, m] or shared [m] with t[0] == 0 ->
        (t_out [N, m], coef [N, M, 4, ncoef], dur [N, M], status [N] int32, info) with info = {"cost": [N, 2] (at
        the input times, at t_out), "pg": [N] stopping measure, "iters": [N] accepted steps}."""
        return self._optimize_times("msnap_optimize_times", wp, t, (), weights, (), min_fraction, max_iter, tol)

    def optimize_times_device(self, n_drones, n_seg, wp, t, shared_times, weights, min_fraction, max_iter, tol,
                              t_out, coef, dur, status, cost=None, pg=None, iters=None):
        """Device pointers, asynchronous; `weights` is a host sequence of 4 (x, y, z, yaw)."""
        self._optimize_times_device("msnap_optimize_times_device", n_drones, n_seg, wp, t, shared_times, (), weights, (),
                                    min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters)

    # ---- dynamic limits (include/msnap.h: certified peaks, uniform retiming) --------------
    @staticmethod
    def limits_array(v_max=0.0, a_max=0.0, j_max=0.0, yaw_rate_max=0.0):
        """The limits[4] of msnap_retime_to_limits (0 or +inf: unconstrained) as a host array."""
        return np.array([v_max, a_max, j_max, yaw_rate_max], dtype=np.float64)

    @staticmethod
    def retime_flags(fit=False, common=False) -> int:
        return (RETIME_FIT if fit else 0) | (RETIME_COMMON if common else 0)

    def dynamic_peaks(self, coef, dur):
        """Certified peaks per drone: (peak [N, 4], t_peak [N, 4], status [N] int32); columns speed, acceleration,
        jerk, yaw rate (msnap_dynamic_peaks)."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        peak = np.empty((N, 4), dtype=np.float64)
        t_peak = np.empty((N, 4), dtype=np.float64)
        status = np.empty((N,), dtype=np.int32)
        with self._lock:
            self._ck(self._lib.msnap_dynamic_peaks(self._h, N, M, pc, pd, peak.ctypes.data_as(ctypes.c_void_p),
                                                   t_peak.ctypes.data_as(ctypes.c_void_p),
                                                   status.ctypes.data_as(ctypes.c_void_p)))
        return peak, t_peak, status

    def dynamic_peaks_device(self, n_drones, n_seg, coef, dur, peak, t_peak, status):
        with self._lock:
            self._ck(self._lib.msnap_dynamic_peaks_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                          _ptr(peak), _ptr(t_peak), _ptr(status)))

    def time_scale(self, coef, dur, scale):
        """Run drone d `scale[d]` times slower (c_j -> c_j scale^-j, T -> scale T): (coef, dur) new arrays."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        sc, psc = _host(scale, np.float64)
        if sc.shape != (N,):
            raise ValueError(f"scale must be [{N}]")
        coef_out, dur_out = np.empty_like(coef), np.empty_like(dur)
        with self._lock:
            self._ck(self._lib.msnap_time_scale(self._h, N, M, pc, pd, psc, coef_out.ctypes.data_as(ctypes.c_void_p),
                                                dur_out.ctypes.data_as(ctypes.c_void_p)))
        return coef_out, dur_out

    def time_scale_device(self, n_drones, n_seg, coef, dur, scale, coef_out, dur_out):
        with self._lock:
            self._ck(self._lib.msnap_time_scale_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                       _ptr(scale), _ptr(coef_out), _ptr(dur_out)))

    def retime_to_limits(self, coef, dur, v_max=0.0, a_max=0.0, j_max=0.0, yaw_rate_max=0.0, fit=False, common=False):
        """Uniformly retimed (coef, dur) that meet the limits, and the per-drone scale [N] (msnap_retime_to_limits;
        a limit of 0 or inf is no limit; `fit`: the scale may be below 1; `common`: one scale for the whole batch)."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        lim, plim = _host(self.limits_array(v_max, a_max, j_max, yaw_rate_max), np.float64)
        coef_out, dur_out = np.empty_like(coef), np.empty_like(dur)
        scale = np.empty((N,), dtype=np.float64)
        with self._lock:
            self._ck(self._lib.msnap_retime_to_limits(
                self._h, N, M, pc, pd, plim, self.retime_flags(fit, common), coef_out.ctypes.data_as(ctypes.c_void_p),
                dur_out.ctypes.data_as(ctypes.c_void_p), scale.ctypes.data_as(ctypes.c_void_p)))
        return coef_out, dur_out, scale

    def retime_to_limits_device(self, n_drones, n_seg, coef, dur, limits, flags, coef_out, dur_out, scale):
        """Device pointers; `limits` is a host sequence of 4 (speed, acceleration, jerk, yaw rate)."""
        lim, plim = _host(limits, np.float64)
        if lim.shape != (4,):
            raise ValueError("limits must hold 4 values")
        with self._lock:
            self._ck(self._lib.msnap_retime_to_limits_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                             plim, int(flags), _ptr(coef_out), _ptr(dur_out),
                                                             _ptr(scale)))

    # ---- pairwise clearance in continuous time (include/msnap.h) --------------------------
    def pair_clearance(self, coef, dur, pairs):
        """Certified distance of the listed pairs of drones while both fly: (min_dist [P], t_min [P], lower [P],
        status [P] int32) with lower <= infimum <= min_dist, min_dist attained at t_min (msnap_pair_clearance).
        `pairs`: [P, 2] drone indices into the batch."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        pr, ppr = _host(pairs, np.int32)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError("pairs must be [P, 2]")
        P = pr.shape[0]
        md = np.empty((P,), dtype=np.float64)
        tm = np.empty((P,), dtype=np.float64)
        lower = np.empty((P,), dtype=np.float64)
        status = np.empty((P,), dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        with self._lock:
            self._ck(self._lib.msnap_pair_clearance(self._h, N, M, pc, pd, P, ppr, vp(md), vp(tm), vp(lower),
                                                    vp(status)))
        return md, tm, lower, status

    def pair_clearance_device(self, n_drones, n_seg, coef, dur, n_pairs, pairs, min_dist, t_min, lower, status):
        """Device pointers (pairs int32 [n_pairs, 2]), asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_pair_clearance_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                           int(n_pairs), _ptr(pairs), _ptr(min_dist), _ptr(t_min),
                                                           _ptr(lower), _ptr(status)))

    # ---- cross clearance: two path sets on shifted clocks (include/msnap.h) ----------------
    def cross_clearance(self, coef_a, dur_a, coef_b, dur_b, pairs, t0_a=None, t0_b=None):
        """Certified distance of drone a of set A and drone b of set B for the listed pairs [P, 2] = (index in A, index
        in B), drone a flying P_a(t - t0_a[a]) on the common clock: (min_dist [P], t_min [P], lower [P], status [P]
        int32) as pair_clearance, t_min on the common clock (msnap_cross_clearance).  The sets have their own segment
        counts; t0_a [Na] / t0_b [Nb] default to zeros."""
        coef_a, pca, dur_a, pda, Na, Ma = self._coef_dur(coef_a, dur_a)
        coef_b, pcb, dur_b, pdb, Nb, Mb = self._coef_dur(coef_b, dur_b)
        pr, ppr = _host(pairs, np.int32)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError("pairs must be [P, 2]")
        t0 = []
        for name, x, n in (("t0_a", t0_a, Na), ("t0_b", t0_b, Nb)):
            if x is None:
                t0.append((None, None))
                continue
            x, px = _host(x, np.float64)
            if x.shape != (n,):
                raise ValueError(f"{name} must be [{n}]")
            t0.append((x, px))
        P = pr.shape[0]
        md = np.empty((P,), dtype=np.float64)
        tm = np.empty((P,), dtype=np.float64)
        lower = np.empty((P,), dtype=np.float64)
        status = np.empty((P,), dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        with self._lock:
            self._ck(self._lib.msnap_cross_clearance(self._h, Na, Ma, pca, pda, t0[0][1], Nb, Mb, pcb, pdb, t0[1][1], P,
                                                     ppr, vp(md), vp(tm), vp(lower), vp(status)))
        return md, tm, lower, status

    def cross_clearance_device(self, n_a, n_seg_a, coef_a, dur_a, t0_a, n_b, n_seg_b, coef_b, dur_b, t0_b, n_pairs,
                               pairs, min_dist, t_min, lower, status):
        """Device pointers (t0_a / t0_b may be None: zeros; pairs int32 [n_pairs, 2]), asynchronous on the context's
        stream."""
        with self._lock:
            self._ck(self._lib.msnap_cross_clearance_device(self._h, int(n_a), int(n_seg_a), _ptr(coef_a), _ptr(dur_a),
                                                            _ptr(t0_a), int(n_b), int(n_seg_b), _ptr(coef_b),
                                                            _ptr(dur_b), _ptr(t0_b), int(n_pairs), _ptr(pairs),
                                                            _ptr(min_dist), _ptr(t_min), _ptr(lower), _ptr(status)))

    # ---- conflict windows: from when until when a pair is too close (include/msnap.h) ------
    @staticmethod
    def _window_outputs(P):
        outs = [np.empty((P,), dtype=np.float64) for _ in range(6)] + [np.empty((P,), dtype=np.int32)]
        return outs, [a.ctypes.data_as(ctypes.c_void_p) for a in outs]

    def pair_conflict_window(self, coef, dur, pairs, threshold, t_res=1e-6):
        """From when until when the listed pairs [P, 2] of one batch are closer than `threshold` [m]:
        (t_clear_until, t_first, d_first, t_last, d_last, t_clear_from, status int32), each [P]
        (msnap_pair_conflict_window).  Clear is proven on [0, t_clear_until) and (t_clear_from, window]; t_first /
        t_last are the earliest / latest conflict found (+inf / -inf: none), to within `t_res` [s] of the proven
        ranges when the search closes."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        pr, ppr = _host(pairs, np.int32)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError("pairs must be [P, 2]")
        P = pr.shape[0]
        outs, ptrs = self._window_outputs(P)
        with self._lock:
            self._ck(self._lib.msnap_pair_conflict_window(self._h, N, M, pc, pd, P, ppr, float(threshold), float(t_res),
                                                          *ptrs))
        return tuple(outs)

    def pair_conflict_window_device(self, n_drones, n_seg, coef, dur, n_pairs, pairs, threshold, t_res, t_clear_until,
                                    t_first, d_first, t_last, d_last, t_clear_from, status):
        """Device pointers (pairs int32 [n_pairs, 2]), asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_pair_conflict_window_device(
                self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur), int(n_pairs), _ptr(pairs), float(threshold),
                float(t_res), _ptr(t_clear_until), _ptr(t_first), _ptr(d_first), _ptr(t_last), _ptr(d_last),
                _ptr(t_clear_from), _ptr(status)))

    def cross_conflict_window(self, coef_a, dur_a, coef_b, dur_b, pairs, threshold, t_res=1e-6, t0_a=None, t0_b=None):
        """pair_conflict_window for drone a of set A against drone b of set B on shifted clocks, as cross_clearance
        (msnap_cross_conflict_window); the times are on the common clock."""
        coef_a, pca, dur_a, pda, Na, Ma = self._coef_dur(coef_a, dur_a)
        coef_b, pcb, dur_b, pdb, Nb, Mb = self._coef_dur(coef_b, dur_b)
        pr, ppr = _host(pairs, np.int32)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError("pairs must be [P, 2]")
        t0 = []
        for name, x, n in (("t0_a", t0_a, Na), ("t0_b", t0_b, Nb)):
            if x is None:
                t0.append((None, None))
                continue
            x, px = _host(x, np.float64)
            if x.shape != (n,):
                raise ValueError(f"{name} must be [{n}]")
            t0.append((x, px))
        P = pr.shape[0]
        outs, ptrs = self._window_outputs(P)
        with self._lock:
            self._ck(self._lib.msnap_cross_conflict_window(self._h, Na, Ma, pca, pda, t0[0][1], Nb, Mb, pcb, pdb,
                                                           t0[1][1], P, ppr, float(threshold), float(t_res), *ptrs))
        return tuple(outs)

    def cross_conflict_window_device(self, n_a, n_seg_a, coef_a, dur_a, t0_a, n_b, n_seg_b, coef_b, dur_b, t0_b,
                                     n_pairs, pairs, threshold, t_res, t_clear_until, t_first, d_first, t_last, d_last,
                                     t_clear_from, status):
        """Device pointers (t0_a / t0_b may be None: zeros; pairs int32 [n_pairs, 2]), asynchronous on the context's
        stream."""
        with self._lock:
            self._ck(self._lib.msnap_cross_conflict_window_device(
                self._h, int(n_a), int(n_seg_a), _ptr(coef_a), _ptr(dur_a), _ptr(t0_a), int(n_b), int(n_seg_b),
                _ptr(coef_b), _ptr(dur_b), _ptr(t0_b), int(n_pairs), _ptr(pairs), float(threshold), float(t_res),
                _ptr(t_clear_until), _ptr(t_first), _ptr(d_first), _ptr(t_last), _ptr(d_last), _ptr(t_clear_from),
                _ptr(status)))

    # ---- mesh clearance in continuous time (include/msnap.h) ------------------------------
    def mesh_clearance(self, coef, dur, tris):
        """Certified distance of each drone's whole path to the mesh `tris` [T, 3, 3]: (min_dist [N], t_min [N],
        tri_min [N] int32, lower [N], status [N] int32) with lower <= infimum <= min_dist, min_dist attained at t_min
        against triangle tri_min (msnap_mesh_clearance)."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        tr, ptr_ = _host(tris, np.float64)
        if tr.ndim != 3 or tr.shape[1:] != (3, 3):
            raise ValueError("tris must be [T, 3, 3]")
        md = np.empty((N,), dtype=np.float64)
        tm = np.empty((N,), dtype=np.float64)
        tri = np.empty((N,), dtype=np.int32)
        lower = np.empty((N,), dtype=np.float64)
        status = np.empty((N,), dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        with self._lock:
            self._ck(self._lib.msnap_mesh_clearance(self._h, N, M, pc, pd, tr.shape[0], ptr_, vp(md), vp(tm), vp(tri),
                                                    vp(lower), vp(status)))
        return md, tm, tri, lower, status

    def mesh_clearance_device(self, n_drones, n_seg, coef, dur, n_tris, tris, min_dist, t_min, tri_min, lower, status):
        """Device pointers (tri_min, status int32), asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_mesh_clearance_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                           int(n_tris), _ptr(tris), _ptr(min_dist), _ptr(t_min),
                                                           _ptr(tri_min), _ptr(lower), _ptr(status)))

    # ---- mesh conflict windows (include/msnap.h) -------------------------------------------
    def mesh_conflict_window(self, coef, dur, tris, threshold, t_res=1e-6):
        """From when until when each drone is closer than `threshold` [m] to the mesh `tris` [T, 3, 3]:
        (t_clear_until, t_first, d_first, tri_first int32, t_last, d_last, tri_last int32, t_clear_from, status int32),
        each [N] (msnap_mesh_conflict_window).  Clear is proven on [0, t_clear_until) and (t_clear_from, total]; t_first
        / t_last are the earliest / latest conflict found (+inf / -inf: none), to within `t_res` [s] of the proven
        ranges when the search closes; d_* and tri_* are the sweep's distance and triangle there."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        tr, ptr_ = _host(tris, np.float64)
        if tr.ndim != 3 or tr.shape[1:] != (3, 3):
            raise ValueError("tris must be [T, 3, 3]")
        kinds = (np.float64, np.float64, np.float64, np.int32, np.float64, np.float64, np.int32, np.float64, np.int32)
        outs = [np.empty((N,), dtype=k) for k in kinds]
        with self._lock:
            self._ck(self._lib.msnap_mesh_conflict_window(self._h, N, M, pc, pd, tr.shape[0], ptr_, float(threshold),
                                                          float(t_res),
                                                          *[a.ctypes.data_as(ctypes.c_void_p) for a in outs]))
        return tuple(outs)

    def mesh_conflict_window_device(self, n_drones, n_seg, coef, dur, n_tris, tris, threshold, t_res, t_clear_until,
                                    t_first, d_first, tri_first, t_last, d_last, tri_last, t_clear_from, status):
        """Device pointers (tri_first, tri_last, status int32), asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_mesh_conflict_window_device(
                self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur), int(n_tris), _ptr(tris), float(threshold),
                float(t_res), _ptr(t_clear_until), _ptr(t_first), _ptr(d_first), _ptr(tri_first), _ptr(t_last),
                _ptr(d_last), _ptr(tri_last), _ptr(t_clear_from), _ptr(status)))

    # ---- path extent in continuous time (include/msnap.h) --------------------------------
    def path_extent(self, coef, dur, dirs):
        """Certified reach of each drone's whole path in the directions `dirs` [K, 3]: (ext [N, K], t_ext [N, K],
        upper [N, K], status [N] int32) with ext <= sup_t n.p(t) <= upper, ext attained at t_ext (msnap_path_extent).
        The six signed axes give a path's certified bounding box."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        dr, pdr = _host(dirs, np.float64)
        if dr.ndim != 2 or dr.shape[1] != 3:
            raise ValueError("dirs must be [K, 3]")
        K = dr.shape[0]
        ext = np.empty((N, K), dtype=np.float64)
        t_ext = np.empty((N, K), dtype=np.float64)
        upper = np.empty((N, K), dtype=np.float64)
        status = np.empty((N,), dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        with self._lock:
            self._ck(self._lib.msnap_path_extent(self._h, N, M, pc, pd, K, pdr, vp(ext), vp(t_ext), vp(upper),
                                                 vp(status)))
        return ext, t_ext, upper, status

    def path_extent_device(self, n_drones, n_seg, coef, dur, n_dirs, dirs, ext, t_ext, upper, status):
        """Device pointers (dirs float64 [n_dirs, 3], status int32), asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_path_extent_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                        int(n_dirs), _ptr(dirs), _ptr(ext), _ptr(t_ext), _ptr(upper),
                                                        _ptr(status)))

    # ---- half-space windows: from when until when a path is outside a half-space (include/msnap.h) ----
    def halfspace_window(self, coef, dur, planes, queries, t_res=1e-6, t_from=None, t_to=None):
        """From when until when the drone of each query is outside the half-space of that query: `planes` [K, 4] =
        (n, b), inside is n.x <= b; `queries` [Q, 2] = (drone, plane); `t_from` / `t_to` [Q] or None (0 / the whole
        flight) give each query's range.  Returns (t_inside_until, t_first, v_first, t_last, v_last, t_inside_from,
        status int32), each [Q] (msnap_halfspace_window): inside is proven on [S, t_inside_until) and
        (t_inside_from, W]; t_first / t_last are the earliest / latest time found outside (+inf / -inf: none), to within
        `t_res` [s] of the proven ranges when the search closes; v_* are n.p there."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        pl, ppl = _host(planes, np.float64)
        if pl.ndim != 2 or pl.shape[1] != 4:
            raise ValueError("planes must be [K, 4]")
        qr, pqr = _host(queries, np.int32)
        if qr.ndim != 2 or qr.shape[1] != 2:
            raise ValueError("queries must be [Q, 2]")
        Q = qr.shape[0]
        rng = []
        for name, x in (("t_from", t_from), ("t_to", t_to)):
            if x is None:
                rng.append((None, None))
                continue
            x, px = _host(x, np.float64)
            if x.shape != (Q,):
                raise ValueError(f"{name} must be [{Q}]")
            rng.append((x, px))
        outs, ptrs = self._window_outputs(Q)
        with self._lock:
            self._ck(self._lib.msnap_halfspace_window(self._h, N, M, pc, pd, pl.shape[0], ppl, Q, pqr, rng[0][1], rng[1][1], float(t_res), *ptrs))
        return tuple(outs)

    def halfspace_window_device(self, n_drones, n_seg, coef, dur, n_planes, planes, n_queries, queries, t_from, t_to,
                                t_res, t_inside_until, t_first, v_first, t_last, v_last, t_inside_from, status):
        """Device pointers (planes float64 [n_planes, 4]; queries int32 [n_queries, 2]; t_from / t_to may be None: 0 /
        the whole flight; status int32), asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_halfspace_window_device(
                self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur), int(n_planes), _ptr(planes), int(n_queries),
                _ptr(queries), _ptr(t_from), _ptr(t_to), float(t_res), _ptr(t_inside_until), _ptr(t_first),
                _ptr(v_first), _ptr(t_last), _ptr(v_last), _ptr(t_inside_from), _ptr(status)))

    # ---- replanning in flight (include/msnap.h) -------------------------------------
    def solve_states_max_segments(self) -> int:
        """Largest segment count solve_states takes at this context's order (and at most max_segments)."""
        return self._mode_max_segments(self._lib.msnap_solve_states_max_segments)

    def _state_block(self, x, N, name):
        if x is None:
            return None, None
        x, px = _host(x, np.float64)
        if x.shape != (N, 4, self.ncoef // 2 - 1):
            raise ValueError(f"{name} must be [N, 4, {self.ncoef // 2 - 1}] for this order-{self.order} context, "
                             f"got {x.shape}")
        return x, px

    def solve_states(self, wp, t, start=None, end=None):
        """solve_batch from and to given end states (msnap_solve_states): wp [N, m, 4], t [N, m] or shared [m] with
        t[0] == 0, start / end [N, 4, K-1] -- entry q-1 the q-th derivative at the first / last waypoint -- or None for
        rest -> coef [N, M, 4, ncoef], dur [N, M], status [N] int32."""
        wp, pwp, t, pt, N, m, shared = _waypoints_times(wp, t)
        M = m - 1
        start, ps = self._state_block(start, N, "start")
        end, pe = self._state_block(end, N, "end")
        coef, dur, status = _out_arrays(None, ((N, max(M, 0), 4, self.ncoef), (N, max(M, 0)), (N,)))
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        with self._lock:
            self._ck(self._lib.msnap_solve_states(self._h, N, M, pwp, pt, shared, ps, pe, vp(coef), vp(dur),
                                                  vp(status)))
        return coef, dur, status

    def solve_states_device(self, n_drones, n_seg, wp, t, shared_times, start, end, coef, dur, status):
        """Device pointers (start / end may be None: rest), asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_solve_states_device(self._h, int(n_drones), int(n_seg), _ptr(wp), _ptr(t),
                                                         int(bool(shared_times)), _ptr(start), _ptr(end), _ptr(coef),
                                                         _ptr(dur), _ptr(status)))

    # ---- gates: prescribed derivatives at interior waypoints (include/msnap.h) -------
    def solve_gates_max_segments(self) -> int:
        """Largest segment count solve_gates takes at this context's order (and at most max_segments)."""
        return self._mode_max_segments(self._lib.msnap_solve_gates_max_segments)

    def solve_gates(self, wp, t, start=None, end=None, fix=None, via=None):
        """solve_states with prescribed derivatives at interior waypoints (msnap_solve_gates): fix [N, M-1] int32 --
        bit q-1 of entry i-1: the q-th derivative at waypoint i is prescribed, on all four axes -- and via
        [N, M-1, 4, K-1] the values (unused entries may be NaN).  fix None: no gates, solve_states' bits
        -> coef [N, M, 4, ncoef], dur [N, M], status [N] int32."""
        wp, pwp, t, pt, N, m, shared = _waypoints_times(wp, t)
        M = m - 1
        start, ps = self._state_block(start, N, "start")
        end, pe = self._state_block(end, N, "end")
        (fix, pf), (via, pv) = self._gate_blocks(fix, via, N, M)
        coef, dur, status = _out_arrays(None, ((N, max(M, 0), 4, self.ncoef), (N, max(M, 0)), (N,)))
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        with self._lock:
            self._ck(self._lib.msnap_solve_gates(self._h, N, M, pwp, pt, shared, ps, pe, pf, pv, vp(coef), vp(dur),
                                                 vp(status)))
        return coef, dur, status

    def _gate_blocks(self, fix, via, N, M):
        """fix / via of a gated entry as host arrays with their pointers (None, None where not given), checked."""
        pf = pv = None
        if fix is not None:
            fix, pf = _host(fix, np.int32)
            if fix.shape != (N, max(M - 1, 0)):
                raise ValueError(f"fix must be [N, M-1] = {(N, max(M - 1, 0))}, got {fix.shape}")
            if via is None:
                raise ValueError("fix needs via")
        if via is not None:
            via, pv = _host(via, np.float64)
            if via.shape != (N, max(M - 1, 0), 4, self.ncoef // 2 - 1):
                raise ValueError(f"via must be [N, M-1, 4, {self.ncoef // 2 - 1}], got {via.shape}")
        return (fix, pf), (via, pv)

    def solve_gates_device(self, n_drones, n_seg, wp, t, shared_times, start, end, fix, via, coef, dur, status):
        """Device pointers (start / end may be None: rest; fix None: no gates, via may then be None too), asynchronous
        on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_solve_gates_device(self._h, int(n_drones), int(n_seg), _ptr(wp), _ptr(t),
                                                        int(bool(shared_times)), _ptr(start), _ptr(end), _ptr(fix),
                                                        _ptr(via), _ptr(coef), _ptr(dur), _ptr(status)))

    # ---- closed-loop paths (include/msnap.h) ----------------------------------------
    def solve_periodic_max_segments(self) -> int:
        """Largest segment count solve_periodic takes at this context's order (and at most max_segments)."""
        return self._mode_max_segments(self._lib.msnap_solve_periodic_max_segments)

    def solve_periodic(self, wp, t):
        """The closed-loop minimum-snap solve (msnap_solve_periodic): wp [N, m, 4], t [N, m] or shared [m] with
        t[0] == 0 and m >= 3; the last waypoint is joined to the first with derivatives 1 .. 2K-2 continuous, the period
        is t[-1], wp[:, -1] - wp[:, 0] the lap offset -> coef [N, M, 4, ncoef], dur [N, M], status [N] int32."""
        wp, pwp, t, pt, N, m, shared = _waypoints_times(wp, t)
        M = m - 1
        coef, dur, status = _out_arrays(None, ((N, max(M, 0), 4, self.ncoef), (N, max(M, 0)), (N,)))
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        with self._lock:
            self._ck(self._lib.msnap_solve_periodic(self._h, N, M, pwp, pt, shared, vp(coef), vp(dur), vp(status)))
        return coef, dur, status

    def solve_periodic_device(self, n_drones, n_seg, wp, t, shared_times, coef, dur, status):
        """Device pointers, asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_solve_periodic_device(self._h, int(n_drones), int(n_seg), _ptr(wp), _ptr(t),
                                                           int(bool(shared_times)), _ptr(coef), _ptr(dur),
                                                           _ptr(status)))

    def optimize_times_states_max_segments(self) -> int:
        """Largest segment count optimize_times_states takes at this context's order (and at most max_segments)."""
        return self._mode_max_segments(self._lib.msnap_optimize_times_states_max_segments)

    def optimize_times_states(self, wp, t, start=None, end=None, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200,
                              tol=1e-4):
        """optimize_times from and to given end states (msnap_optimize_times_states): wp, t, weights, min_fraction,
        max_iter, tol and the result tuple as optimize_times; start / end [N, 4, K-1] as solve_states takes them, or
        None for rest.  Waypoints, both end states and the total duration are kept; coef, dur are the boundary-state
        solution for t_out."""
        return self._optimize_times("msnap_optimize_times_states", wp, t, (start, end), weights, (),
                                    min_fraction, max_iter, tol)

    def optimize_times_states_device(self, n_drones, n_seg, wp, t, shared_times, start, end, weights, min_fraction,
                                     max_iter, tol, t_out, coef, dur, status, cost=None, pg=None, iters=None):
        """Device pointers (start / end may be None: rest), asynchronous; `weights` is a host sequence of 4."""
        self._optimize_times_device("msnap_optimize_times_states_device", n_drones, n_seg, wp, t, shared_times,
                                    (_ptr(start), _ptr(end)), weights, (), min_fraction, max_iter, tol, t_out, coef,
                                    dur, status, cost, pg, iters)

    def optimize_times_periodic_max_segments(self) -> int:
        """Largest segment count optimize_times_periodic takes at this context's order (and at most max_segments)."""
        return self._mode_max_segments(self._lib.msnap_optimize_times_periodic_max_segments)

    def optimize_times_periodic(self, wp, t, weights=(1, 1, 1, 1), min_fraction=0.1, max_iter=200, tol=1e-4):
        """optimize_times on closed loops (msnap_optimize_times_periodic): wp, t (m >= 3 waypoints) as solve_periodic
        takes them, the other arguments and the result tuple as optimize_times.  Waypoints and the period t[-1] are
        kept; coef, dur are the periodic solution for t_out."""
        return self._optimize_times("msnap_optimize_times_periodic", wp, t, (), weights, (), min_fraction,
                                    max_iter, tol)

    def optimize_times_periodic_device(self, n_drones, n_seg, wp, t, shared_times, weights, min_fraction, max_iter, tol,
                                       t_out, coef, dur, status, cost=None, pg=None, iters=None):
        """Device pointers, asynchronous; `weights` is a host sequence of 4 (x, y, z, yaw)."""
        self._optimize_times_device("msnap_optimize_times_periodic_device", n_drones, n_seg, wp, t, shared_times, (),
                                    weights, (), min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters)

    def optimize_times_free_max_segments(self) -> int:
        """Largest segment count optimize_times_free takes at this context's order (and at most max_segments)."""
        return self._mode_max_segments(self._lib.msnap_optimize_times_free_max_segments)

    def optimize_times_free(self, wp, t, start=None, end=None, weights=(1, 1, 1, 1), time_weight=1.0, min_fraction=0.1,
                            max_iter=200, tol=1e-4):
        """optimize_times_states with the total duration free (msnap_optimize_times_free): minimises
        sum_a weights[a] J_a + time_weight * t_out[-1] over every segment duration.  time_weight > 0 is a number or
        [N], one per drone; t[-1] is a starting guess and the floor's scale.  The result tuple is optimize_times's,
        with info["cost"] the objective (time term included) at the raised input times and at t_out."""
        return self._optimize_times("msnap_optimize_times_free", wp, t, (start, end), weights, (time_weight,),
                                    min_fraction, max_iter, tol)

    def optimize_times_free_device(self, n_drones, n_seg, wp, t, shared_times, start, end, weights, time_weight,
                                   min_fraction, max_iter, tol, t_out, coef, dur, status, cost=None, pg=None,
                                   iters=None):
        """Device pointers (start / end may be None: rest; time_weight [n_drones] float64 on the device),
        asynchronous; `weights` is a host sequence of 4."""
        self._optimize_times_device("msnap_optimize_times_free_device", n_drones, n_seg, wp, t, shared_times,
                                    (_ptr(start), _ptr(end)), weights, (_ptr(time_weight),), min_fraction, max_iter,
                                    tol, t_out, coef, dur, status, cost, pg, iters)

    def optimize_times_gates_max_segments(self) -> int:
        """Largest segment count optimize_times_gates takes at this context's order (and at most max_segments)."""
        return self._mode_max_segments(self._lib.msnap_optimize_times_gates_max_segments)

    def optimize_times_gates(self, wp, t, start=None, end=None, fix=None, via=None, weights=(1, 1, 1, 1),
                             min_fraction=0.1, max_iter=200, tol=1e-4):
        """optimize_times_states through gates (msnap_optimize_times_gates): fix [N, M-1] int32 and via [N, M-1, 4, K-1]
        as solve_gates takes them (fix None: no gates, optimize_times_states' bits).  Waypoints, both end states, the
        gate values in physical units and the total duration are kept; coef, dur are solve_gates' for t_out."""
        N, m = _waypoints_times(wp, t)[4:6]
        (fix, pf), (via, pv) = self._gate_blocks(fix, via, N, m - 1)      # (the arrays live until the call returns)
        return self._optimize_times("msnap_optimize_times_gates", wp, t, (start, end), weights, (), min_fraction,
                                    max_iter, tol, gates=(pf, pv))

    def optimize_times_gates_device(self, n_drones, n_seg, wp, t, shared_times, start, end, fix, via, weights,
                                    min_fraction, max_iter, tol, t_out, coef, dur, status, cost=None, pg=None,
                                    iters=None):
        """Device pointers (start / end may be None: rest; fix None: no gates, via may then be None too),
        asynchronous; `weights` is a host sequence of 4."""
        self._optimize_times_device("msnap_optimize_times_gates_device", n_drones, n_seg, wp, t, shared_times,
                                    (_ptr(start), _ptr(end), _ptr(fix), _ptr(via)), weights, (), min_fraction,
                                    max_iter, tol, t_out, coef, dur, status, cost, pg, iters)

    def eval_state(self, coef, dur, tq):
        """Full state of each drone at its own time tq [N] (msnap_eval_state): pos [N, 4], deriv [N, 4, K-1] with
        entry q-1 the q-th derivative -- the layout solve_states takes as `start`.  NaN where tq is outside the path."""
        coef, pc, dur, pd, N, M = self._coef_dur(coef, dur)
        tq, ptq = _host(tq, np.float64)
        if tq.shape != (N,):
            raise ValueError("tq must be [N]")
        pos = np.empty((N, 4), dtype=np.float64)
        deriv = np.empty((N, 4, self.ncoef // 2 - 1), dtype=np.float64)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        with self._lock:
            self._ck(self._lib.msnap_eval_state(self._h, N, M, pc, pd, ptq, vp(pos), vp(deriv)))
        return pos, deriv

    def eval_state_device(self, n_drones, n_seg, coef, dur, tq, pos, deriv):
        """Device pointers, asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_eval_state_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                       _ptr(tq), _ptr(pos), _ptr(deriv)))

    # ---- near pairs (include/msnap.h) ---------------------------------------------
    def near_pairs(self, pos, base: float, speed=None, gap: float = 0.0, margin: float = 0.0, max_pairs=None):
        """(pairs int32 [P, 2], dist [P]): every pair i < j of the swarm `pos` [N, S, 3] whose sampled distance is below
        (base + (speed[i] + speed[j]) gap) (1 + margin), in ascending (i, j) order, with that distance
        (msnap_formation_near_pairs).  `max_pairs=None` counts first and then fetches the whole list; with a number at
        most that many pairs are returned (the first of the order)."""
        p, pp = _host(pos, np.float64)
        if p.ndim != 3 or p.shape[2] != 3:
            raise ValueError("pos must be [N, S, 3]")
        N, S, _ = p.shape
        ps = None
        if speed is not None:
            sp, ps = _host(speed, np.float64)
            if sp.shape != (N,):
                raise ValueError("speed must be [N]")
        found = ctypes.c_longlong(0)

        def call(cap, pairs, dist):
            vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None      # noqa: E731
            with self._lock:
                self._ck(self._lib.msnap_formation_near_pairs(self._h, N, S, pp, float(base), ps, float(gap),
                                                              float(margin), cap, vp(pairs), vp(dist),
                                                              ctypes.byref(found)))
        if max_pairs is None:
            call(0, None, None)
            cap = int(found.value)
        else:
            cap = int(max_pairs)
            if cap < 0:
                raise ValueError("max_pairs >= 0")
        pairs = np.empty((cap, 2), dtype=np.int32)
        dist = np.empty((cap,), dtype=np.float64)
        if cap:
            call(cap, pairs, dist)
        elif max_pairs is not None:
            call(0, None, None)
        n = min(cap, int(found.value))
        return pairs[:n], dist[:n]

    def near_pairs_device(self, n_drones, n_samples, pos, base, speed, gap, margin, max_pairs, pairs, pair_dist, n_found):
        """Device pointers (speed, pairs with max_pairs == 0, and pair_dist may be None; n_found an int64 [1]),
        asynchronous on the context's stream."""
        with self._lock:
            self._ck(self._lib.msnap_formation_near_pairs_device(self._h, int(n_drones), int(n_samples), _ptr(pos),
                                                                 float(base), _ptr(speed), float(gap), float(margin),
                                                                 int(max_pairs), _ptr(pairs), _ptr(pair_dist),
                                                                 _ptr(n_found)))

    # ---- collision passes --------------------------------------------------------
    def formation_collide(self, pos_rows, pos_cols, radius: float, row_offset: int = 0):
        pr, ppr = _host(pos_rows, np.float64)
        pc, ppc = _host(pos_cols, np.float64)
        if pr.ndim != 3 or pr.shape[2] != 3 or pc.ndim != 3 or pc.shape[1:] != pr.shape[1:]:
            raise ValueError("pos_rows [R,S,3] and pos_cols [C,S,3] must share S")
        R, S, _ = pr.shape
        Cn = pc.shape[0]
        md = np.empty((R,), dtype=np.float64)
        partner = np.empty((R,), dtype=np.int32)
        hit = np.empty((R,), dtype=np.int32)
        with self._lock:
            self._ck(self._lib.msnap_formation_collide(
                self._h, R, int(row_offset), Cn, S, ppr, ppc, float(radius),
                md.ctypes.data_as(ctypes.c_void_p), partner.ctypes.data_as(ctypes.c_void_p),
                hit.ctypes.data_as(ctypes.c_void_p)))
        return md, partner, hit.astype(bool)

    def formation_collide_device(self, n_rows, row_offset, n_cols, n_samples, pos_rows, pos_cols, radius,
                                 min_dist, partner, hit):
        with self._lock:
            self._ck(self._lib.msnap_formation_collide_device(
                self._h, int(n_rows), int(row_offset), int(n_cols), int(n_samples), _ptr(pos_rows),
                _ptr(pos_cols), float(radius), _ptr(min_dist), _ptr(partner), _ptr(hit)))

    def collide_rows_t_doubles(self, n_rows: int, n_samples: int) -> int:
        return int(self._lib.msnap_collide_rows_t_doubles(int(n_rows), int(n_samples)))

    def collide_takes_broad_phase(self, n_rows: int, row_offset: int, n_cols: int, n_samples: int) -> bool:
        """Whether formation_collide with these arguments would run behind the exact broad phase (the library's own
        predicate: size limits and the "collide_*" options)."""
        return bool(self._lib.msnap_formation_collide_takes_broad_phase(self._h, int(n_rows), int(row_offset),
                                                                        int(n_cols), int(n_samples)))

    def whole_pass_pays(self, n_drones: int, n_ranks: int) -> bool:
        """After a whole-swarm pass: does running it on every one of `n_ranks` ranks beat dividing the pairs (the
        library's cost model on the counts that pass left; synchronises the stream)?"""
        pays = ctypes.c_int()
        with self._lock:
            self._ck(self._lib.msnap_formation_whole_pass_pays(self._h, int(n_drones), int(n_ranks), ctypes.byref(pays)))
        return bool(pays.value)

    def collide_reads_rows_t(self, n_rows: int, row_offset: int, n_cols: int, n_samples: int) -> bool:
        """Whether formation_collide_t_device with these arguments would read a row image (msnap.h): a whole swarm
        behind the exact broad phase builds its own, spatially sorted one."""
        return bool(self._lib.msnap_formation_collide_reads_rows_t(self._h, int(n_rows), int(row_offset), int(n_cols),
                                                                   int(n_samples)))

    def sample_collide_device(self, n_drones, n_seg, coef, dur, dt, n_samples, pos, pos_t):
        """The sampler with its second output: the transposed row image the pairwise pass reads."""
        with self._lock:
            self._ck(self._lib.msnap_sample_collide_device(self._h, int(n_drones), int(n_seg), _ptr(coef), _ptr(dur),
                                                          float(dt), int(n_samples), _ptr(pos), _ptr(pos_t)))

    def solve_grid_sample_device(self, n_drones, n_seg, wp, dt, n_samples, coef, dur, status, pos, pos_t=None):
        """The shared-grid solve and the sampler as one launch (msnap.h): the outputs of solve_grid_device followed by
        sample_collide_device (`pos_t` given) or the 3-axis sampler, bit for bit."""
        with self._lock:
            self._ck(self._lib.msnap_solve_grid_sample_device(
                self._h, int(n_drones), int(n_seg), _ptr(wp), float(dt), int(n_samples), _ptr(coef), _ptr(dur),
                _ptr(status), _ptr(pos), _ptr(pos_t) if pos_t is not None else None))

    def formation_collide_t_device(self, n_rows, row_offset, n_cols, n_samples, pos_rows_t, pos_rows, pos_cols, radius,
                                   min_dist, partner, hit):
        with self._lock:
            self._ck(self._lib.msnap_formation_collide_t_device(
                self._h, int(n_rows), int(row_offset), int(n_cols), int(n_samples), _ptr(pos_rows_t), _ptr(pos_rows),
                _ptr(pos_cols), float(radius), _ptr(min_dist), _ptr(partner), _ptr(hit)))

    # ---- the pairwise pass in parts: every unordered pair on exactly one rank (include/msnap.h) ----
    def formation_part_bytes(self, n_drones: int) -> int:
        return int(self._lib.msnap_formation_part_bytes(int(n_drones)))

    def formation_collide_part(self, pos_all, part: int, n_parts: int):
        """One rank's part of the pass over the whole swarm `pos_all` [N,S,3]: a uint8 block of
        formation_part_bytes(N) bytes (squared minima [N] float64, then partners [N] int32)."""
        pa, ppa = _host(pos_all, np.float64)
        if pa.ndim != 3 or pa.shape[2] != 3:
            raise ValueError("pos_all must be [N, S, 3]")
        N, S, _ = pa.shape
        out = np.empty((self.formation_part_bytes(N),), dtype=np.uint8)
        with self._lock:
            self._ck(self._lib.msnap_formation_collide_part(self._h, N, S, ppa, int(part), int(n_parts),
                                                            out.ctypes.data_as(ctypes.c_void_p)))
        return out

    @staticmethod
    def split_part(block, n_drones: int):
        """(squared minima [N] float64, partners [N] int32) views of one part block."""
        b = np.ascontiguousarray(block, dtype=np.uint8)
        return b[:8 * n_drones].view(np.float64), b[8 * n_drones:12 * n_drones].view(np.int32)

    def formation_collide_finish(self, parts, n_drones: int, radius: float, row_offset: int = 0, n_rows=None):
        """Fold the parts (uint8 [P, formation_part_bytes(N)]) for the rows [row_offset, row_offset + n_rows)."""
        pb, ppb = _host(parts, np.uint8)
        stride = self.formation_part_bytes(n_drones)
        if pb.ndim != 2 or pb.shape[1] != stride:
            raise ValueError("parts must be [P, formation_part_bytes(N)] uint8")
        n_rows = n_drones - row_offset if n_rows is None else int(n_rows)
        md = np.empty((n_rows,), dtype=np.float64)
        partner = np.empty((n_rows,), dtype=np.int32)
        hit = np.empty((n_rows,), dtype=np.int32)
        with self._lock:
            self._ck(self._lib.msnap_formation_collide_finish(
                self._h, int(n_drones), pb.shape[0], ppb, int(row_offset), n_rows, float(radius),
                md.ctypes.data_as(ctypes.c_void_p), partner.ctypes.data_as(ctypes.c_void_p),
                hit.ctypes.data_as(ctypes.c_void_p)))
        return md, partner, hit.astype(bool)

    def formation_collide_part_device(self, n_drones, n_samples, pos_all, part, n_parts, part_out):
        with self._lock:
            self._ck(self._lib.msnap_formation_collide_part_device(
                self._h, int(n_drones), int(n_samples), _ptr(pos_all), int(part), int(n_parts), _ptr(part_out)))

    def formation_collide_finish_device(self, n_drones, n_parts, parts, row_offset, n_rows, radius, min_dist,
                                        partner, hit):
        with self._lock:
            self._ck(self._lib.msnap_formation_collide_finish_device(
                self._h, int(n_drones), int(n_parts), _ptr(parts), int(row_offset), int(n_rows), float(radius),
                _ptr(min_dist), _ptr(partner), _ptr(hit)))

    def mesh_sweep(self, pos, tris, radius: float):
        p, pp = _host(pos, np.float64)
        tr, ptr_ = _host(tris, np.float64)
        if p.ndim != 3 or p.shape[2] != 3:
            raise ValueError("pos must be [N, S, 3]")
        if tr.ndim != 3 or tr.shape[1:] != (3, 3):
            raise ValueError("tris must be [T, 3, 3]")
        N, S, _ = p.shape
        Tn = tr.shape[0]
        md = np.empty((N,), dtype=np.float64)
        hit = np.empty((N,), dtype=np.int32)
        with self._lock:
            self._ck(self._lib.msnap_mesh_sweep(self._h, N, S, pp, Tn, ptr_, float(radius),
                                               md.ctypes.data_as(ctypes.c_void_p),
                                               hit.ctypes.data_as(ctypes.c_void_p)))
        return md, hit.astype(bool)

    def mesh_validity(self, states, robot_tris, env_tris):
        """states [N,4] (x,y,z,yaw), meshes [R,3,3] / [E,3,3] -> valid [N] bool (True = no collision):
        the planner's isStateValid for a batch of states."""
        st, pst = _host(states, np.float64)
        rt, prt = _host(robot_tris, np.float64)
        et, pet = _host(env_tris, np.float64)
        if st.ndim != 2 or st.shape[1] != 4:
            raise ValueError("states must be [N, 4]")
        if rt.ndim != 3 or rt.shape[1:] != (3, 3) or et.ndim != 3 or et.shape[1:] != (3, 3):
            raise ValueError("robot_tris / env_tris must be [T, 3, 3]")
        N = st.shape[0]
        valid = np.empty((N,), dtype=np.int32)
        with self._lock:
            self._ck(self._lib.msnap_mesh_validity(self._h, N, pst, rt.shape[0], prt, et.shape[0], pet,
                                                  valid.ctypes.data_as(ctypes.c_void_p)))
        return valid.astype(bool)

    def mesh_validity_device(self, n_states, states, n_rtris, rtris, n_etris, etris, valid):
        with self._lock:
            self._ck(self._lib.msnap_mesh_validity_device(self._h, int(n_states), _ptr(states), int(n_rtris),
                                                         _ptr(rtris), int(n_etris), _ptr(etris), _ptr(valid)))

    def mesh_sweep_device(self, n_drones, n_samples, pos, n_tris, tris, radius, min_dist, hit):
        with self._lock:
            self._ck(self._lib.msnap_mesh_sweep_device(self._h, int(n_drones), int(n_samples), _ptr(pos),
                                                      int(n_tris), _ptr(tris), float(radius), _ptr(min_dist),
                                                      _ptr(hit)))


_default = {}
_default_lock = threading.Lock()


def default_context(order: int = 7, device_id: int = 0) -> Context:
    """Process-wide context per (device, order), created on first use."""
    key = (int(device_id), int(order))
    with _default_lock:
        ctx = _default.get(key)
        if ctx is None:
            ctx = Context(device_id=device_id, order=order, max_segments=4096)
            _default[key] = ctx
        return ctx
