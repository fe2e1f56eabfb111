/* msnap.h -- C-ABI of the MI355X-native minimum-snap trajectory hot path.
 *
 * The reference (mjmyt/drone_path_planning_python) has no FFI: its de-facto
 * boundary for this path is the Python call
 *     calculate_trajectory4D(waypoints)      src/optimizations/__init__.py:2,
 *                                            src/optimizations/calculatingTrajectories.py:200-213
 * invoked from scripts/drones_pols_generator.py:58.  Every entry point below
 * names the reference interface it replaces.  Plain pointers and sizes only;
 * no torch / numpy types cross this boundary.
 *
 * Conventions
 *   - all arrays row-major, caller-owned, fp64 unless noted;
 *   - entry points WITHOUT a suffix take HOST pointers and are synchronous (device
 *     staging owned by the context; the two solve entry points cut large batches
 *     into chunks that overlap upload, kernel and download -- at full PCIe rate when
 *     the host buffers come from msnap_host_alloc, correct with any host memory);
 *   - entry points ending in _device take DEVICE pointers, are asynchronous on
 *     the context's stream (msnap_sync / stream order to observe results);
 *   - order = polynomial degree, 7 (minimum snap, the reference) or 9
 *     (minimum crackle, BASELINE.json configs[4]; no reference exists);
 *     ncoef = order + 1; coefficients are in ASCENDING powers (c_k t^k), the
 *     reference's Polynomial.p layout (src/optimizations/uav_trajectory.py:17-22);
 *   - functions return 0 or a negative msnap_error; they never throw or abort.
 *     Per-drone problems are reported in status[] (the reference raises
 *     numpy.linalg.LinAlgError / AssertionError out of the ROS callback instead).
 *   - a context is not re-entrant: serialise calls per context (the Python
 *     wrapper holds a lock; rospy runs callback1/callback2 on separate threads,
 *     scripts/drones_pols_generator.py:102-103).  Contexts are independent.
 */
#ifndef MSNAP_H
#define MSNAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msnap_ctx msnap_ctx;

enum msnap_error {
  MSNAP_OK = 0,
  MSNAP_EINVAL = -1,      /* null pointer / negative size / bad flag          */
  MSNAP_EHIP = -2,        /* a HIP runtime call failed (msnap_last_hip_error) */
  MSNAP_EORDER = -3,      /* order is not 7 or 9                              */
  MSNAP_ESEGMENTS = -4,   /* n_seg < 1 or n_seg > max_segments of the context */
  MSNAP_ENOMEM = -5,      /* host or device allocation failed                 */
  MSNAP_ENODEVICE = -6,   /* no gfx950 device / device_id out of range        */
  MSNAP_ENOGRID = -7,     /* msnap_solve_grid without a prepared grid          */
  MSNAP_ECAPTURE = -8     /* a scratch buffer of the context would have to grow while its stream is being
                             captured into a graph (growing synchronises and frees), or a query that has to
                             synchronise the stream was made during a capture: run the same call once outside the
                             capture first -- the buffers then have their size */
};

/* Stream capture (hipGraph) and the context's scratch buffers.  A call captured into a graph records raw pointers
 * into the context's internal buffers.  The library therefore remembers every buffer a capture has used: when a
 * LATER call (eager, or another capture) needs such a buffer larger, the old block is not freed -- it is retired and
 * stays valid until msnap_destroy or msnap_release_graph_buffers -- so a graph instantiated earlier keeps replaying
 * on memory that is still its own and still gives the result of the pass it captured.  A replay does not see options
 * set after the capture; a graph that captured msnap_solve_grid_device is tied to the grid prepared at that time --
 * preparing another grid on the context invalidates it (its memory stays valid, its results do not).  msnap_release_graph_buffers frees the retired
 * blocks: call it once every graph that captured calls of this context has been destroyed; it returns the number of
 * bytes released through *bytes (may be NULL). */
int msnap_release_graph_buffers(msnap_ctx *ctx, size_t *bytes);

enum msnap_status {       /* per-drone, written to status[]                   */
  MSNAP_ST_OK = 0,
  MSNAP_ST_SINGULAR = 1,  /* a pivot of the block LDL^T was <= 0 or not finite */
  MSNAP_ST_TIMES = 2,     /* times not strictly increasing (or t[1] <= 2 t[0]) */
  MSNAP_ST_NONFINITE = 3, /* NaN / Inf in the waypoints or times               */
  MSNAP_ST_PAIR = 4       /* msnap_pair_clearance: a drone index outside [0, n_drones), or a == b; msnap_cross_clearance:
                             an index outside its set; msnap_halfspace_window: a drone or plane index out of range */
};

int msnap_version(void);                       /* 10000*major + 100*minor + patch */
const char *msnap_strerror(int code);
const char *msnap_last_hip_error(const msnap_ctx *ctx);
/* Name (as a profiler prints it, e.g. "msnap::solve_kernel_twin<5, 10>") of the kernel instance the most recent
 * solve entry point of this context launched -- msnap_solve_batch[_device] or msnap_solve_grid[_device];
 * "" before the first one.  The choice depends on order, segment count, batch size and the options above. */
const char *msnap_last_kernel(const msnap_ctx *ctx);

/* One HIP stream + pinned/device scratch per context. */
int msnap_create(msnap_ctx **out, int device_id, int order, int max_segments);
void msnap_destroy(msnap_ctx *ctx);
/* Borrow an external hipStream_t (e.g. torch's current stream; NULL is the HIP
 * null stream).  msnap_use_own_stream goes back to the context's own stream. */
int msnap_set_stream(msnap_ctx *ctx, void *hip_stream);
int msnap_use_own_stream(msnap_ctx *ctx);
void *msnap_get_stream(msnap_ctx *ctx);
int msnap_sync(msnap_ctx *ctx);
/* Page-locked host memory for the host-pointer entry points (the reference's arrays
 * are ordinary NumPy allocations, src/optimizations/calculatingTrajectories.py:137-144;
 * pinned ones let the copy engines read and write them directly). */
int msnap_host_alloc(void **ptr, size_t bytes);
int msnap_host_free(void *ptr);
/* Options of a context (launch geometry: tests and tuning tools, every default is chosen per
 * launch from the device's CU count; stream priority: callers that overlap two contexts).  Unknown
 * names return MSNAP_EINVAL.
 *   "solve_grid_waves"     cap on the persistent grid of the large-batch solve kernel (0 = default);
 *                          a small cap makes every wave walk several tiles (the regime of a
 *                          saturating batch) on a batch the oracle checks in seconds
 *   "gemm_grid_waves"      the same for the shared-grid GEMM
 *   "gemm_stream_waves_per_cu"  wavefronts per CU up to which the streaming GEMM (16 and more segments) slices its
 *                          column tiles over more waves (0 = default: 16)
 *   "no_grid_sample"       1: msnap_solve_grid_sample_device runs the two kernels where it would fuse (A/B timing)
 *   "twist_max_drones"     largest batch that takes the small-batch two-sided kernel (0 = default)
 *   "no_twist"             1: small batches stay on the one-sided kernels
 *   "twist_waves"          waves per 8-drone tile of the small-batch kernel: 1, 2 or 4 (0 = default: 4 up to
 *                          one tile per four CUs, 2 up to one per two, 1 above); outputs are bitwise the same
 *   "twin_max_drones"      largest batch that takes the two-sided column-split throughput kernel (0 = default:
 *                          order 7 up to 128 drones per CU, order 9 any size)
 *   "no_twin"             1: order-9 batches stay on the one-sided throughput kernel where the two-sided
 *                          column-split one would run (A/B timing)
 *   "collide_waves_per_cu" shares per CU of the pairwise pass (0 = one 8-column x 128-row block per share)
 *   "collide_sample_parts" waves per share of the pairwise pass, each a range of the sample chunks
 *                          (0 = chosen per launch: more than one only when the launch is small)
 *   "collide_no_sym"       1: the rows handed to msnap_formation_collide are not the slice of its columns at
 *                          row_offset -- every pair is evaluated one-sidedly (read-only companion
 *                          "collide_last_sym": 1 if the last pass evaluated its own-range pairs once)
 *   "collide_cull_min_drones"  smallest whole swarm that takes the exact broad phase (0 = default 3072; at least
 *                          256: tests lower it to check the path against the oracle on small swarms)
 *   "collide_no_cull"      1: whole-swarm passes (row_offset 0, n_rows == n_cols, 3072..16384 drones) skip the exact
 *                          broad phase -- spatial sort, per-drone bounds, box test per 8-column share -- and
 *                          evaluate every pair; results are identical either way (a dense swarm, where nothing
 *                          can be culled, saves the sort: about a sixth of the pass at 4096 drones).  Read-only
 *                          companions: "collide_last_cull" (1 if the last pass took the broad phase),
 *                          "collide_last_shares" (its 128 x 8 shares before the test), "collide_last_survivors"
 *                          (the shares that pass it) and "collide_last_group_pairs" (the 8 x 8 group pairs that
 *                          pass it; both synchronise the stream).  msnap_set_option refuses the read-only names
 *                          ("collide_last_*") with MSNAP_EINVAL
 *   "collide_cull_mode"    what the broad phase evaluates: 1 the surviving 128 x 8 shares (then the merge of their
 *                          entries), 2 the surviving 8 x 8 group pairs (then the per-group fold of their candidates;
 *                          swarms up to 8192 drones: every group pair has a list slot), 0 (default) chosen per pass
 *                          on the HOST -- the two launch sequences and their buffers differ -- from the survivor
 *                          counts the context's previous pass over a swarm of this size left in page-locked memory
 *                          (read without synchronising; a pass without such counts takes the shares).  Results are
 *                          identical either way
 *   "mesh_waves_per_cu"    wavefronts per CU msnap_mesh_sweep's grid is capped at (0 = one workgroup per drone: a large
 *                          sweep then holds every wave slot of the chip for its whole run).  A sweep on a second
 *                          stream beside other kernels leaves them room with 8..12 (it runs longer itself:
 *                          4096 drones x 96 samples x 68 triangles 33 -> 40..45 us, the pipeline around it 106 -> 102)
 *   "mesh_count_tests"     1: count the point-triangle tests msnap_mesh_sweep evaluates (the ones
 *                          its bounding-box cull does not skip); msnap_get_option returns the count
 *                          since the option was last set (and synchronises the stream); 0: off
 *   "pipe_chunk_mb"        output megabytes per chunk of the chunked host-pointer solves
 *   "own_stream_priority"  0 default, 1 the lowest, 2 the highest priority the device offers: re-creates
 *                          the context's own stream (after draining it).  A pass that should only fill the
 *                          gaps of another context's work -- the mesh sweep beside the pairwise pass --
 *                          runs on a lowest-priority stream: its workgroups are dispatched when the
 *                          other queue has none waiting.  Setting it destroys and re-creates the stream:
 *                          set it BEFORE msnap_get_stream() hands the handle to anybody (a wrapper around
 *                          the old handle -- e.g. torch.cuda.ExternalStream -- would dangle)
 * msnap_create seeds them once from the environment variables MSNAP_SOLVE_GRID_WAVES,
 * MSNAP_GEMM_GRID_WAVES, MSNAP_GEMM_STREAM_WAVES_PER_CU, MSNAP_NO_GRID_SAMPLE, MSNAP_MESH_WAVES_PER_CU, MSNAP_TWIST_MAX_DRONES, MSNAP_NO_TWIST, MSNAP_NO_TWIN, MSNAP_TWIN_MAX_DRONES, MSNAP_COLLIDE_WAVES_PER_CU,
 * MSNAP_COLLIDE_SAMPLE_PARTS, MSNAP_COLLIDE_NO_CULL, MSNAP_COLLIDE_CULL_MIN_DRONES,
 * MSNAP_COLLIDE_CULL_MODE and MSNAP_PIPE_CHUNK_MB; nothing on a launch path reads the environment. */
int msnap_set_option(msnap_ctx *ctx, const char *name, long value);
int msnap_get_option(const msnap_ctx *ctx, const char *name, long *value);
/* hipEvent timing on the context's stream (bench.py roofline leg). */
int msnap_timer_start(msnap_ctx *ctx);
int msnap_timer_stop(msnap_ctx *ctx, float *elapsed_ms);   /* synchronises */

/* ---- a1/a2: calculate_trajectory1D / calculate_trajectory4D, batched ----------
 * replaces src/optimizations/calculatingTrajectories.py:37-197 (per axis) and
 * :200-213 (4 axes) for n_drones independent trajectories.
 *   wp     [n_drones][n_seg+1][4]   x, y, z, yaw per waypoint
 *   t      [n_drones][n_seg+1] absolute times, or [n_seg+1] if shared_times != 0
 *   coef   [n_drones][n_seg][4][ncoef]  out, ascending powers
 *   dur    [n_drones][n_seg]            out, T_i = t[i+1]-t[i]  (time_points, :59-61)
 *   status [n_drones]                   out, msnap_status
 * Drones with status != 0 get NaN coefficients.
 */
int msnap_solve_batch(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp,
                      const double *t, int shared_times, double *coef, double *dur,
                      int32_t *status);
int msnap_solve_batch_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp,
                             const double *t, int shared_times, double *coef,
                             double *dur, int32_t *status);

/* ---- a1/a2 on a SHARED time grid: one fp64 MFMA GEMM -----------------------------
 * The reference's own usage: path_to_pol gives every drone the uniform grid
 * t_i = i*10/n (scripts/drones_pols_generator.py:44-46,56), so the matrix of
 * calculate_trajectory1D (src/optimizations/calculatingTrajectories.py:48-131) is
 * shared and the coefficients are linear in the waypoints.
 *   msnap_grid_prepare  builds the (n_seg+1) x (n_seg*ncoef) operator for t on
 *                       the GPU (the solve kernel on unit waypoint vectors);
 *   msnap_solve_grid    applies it to n_drones waypoint sets: same outputs as
 *                       msnap_solve_batch(.., t, shared_times = 1, ..).
 * The operator stays valid until the next msnap_grid_prepare on this context.
 * n_seg of msnap_solve_grid[_device] is the segment count the CALLER sized wp / coef / dur for (as in
 * msnap_solve_batch): it must equal the prepared grid's, else MSNAP_ESEGMENTS and nothing is written -- the reference
 * call sizes its output from its input (calculatingTrajectories.py:45-49), a C caller's buffers cannot be inspected.
 * msnap_grid_segments: segments of the grid this context holds (0: none prepared, negative: error).
 */
int msnap_grid_prepare(msnap_ctx *ctx, int n_seg, const double *t /* host [n_seg+1] */);
int msnap_grid_prepare_device(msnap_ctx *ctx, int n_seg, const double *t /* device */);
int msnap_grid_segments(const msnap_ctx *ctx);
int msnap_solve_grid(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, double *coef, double *dur,
                     int32_t *status);
int msnap_solve_grid_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, double *coef,
                            double *dur, int32_t *status);

/* ---- a7: the float32 [T | x | y | z | yaw] matrix of path_to_pol -----------------
 * replaces scripts/drones_pols_generator.py:63-77.
 *   out [n_drones][n_seg][1 + 4*ncoef] float32
 */
int msnap_pack_pol_matrix(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef,
                          const double *dur, float *out);
int msnap_pack_pol_matrix_device(msnap_ctx *ctx, int n_drones, int n_seg,
                                 const double *coef, const double *dur, float *out);

/* ---- a8: transform(path) of the formation node, K offsets ------------------------
 * replaces scripts/drones_traj_generator.py:56-89 (K = 2 hard-coded there).
 *   rb_pose [n_poses][7]   x y z qx qy qz qw of the rigid body
 *   offsets [n_offsets][3] body-frame drone positions (identity orientation)
 *   out     [n_offsets][n_poses][7]   p' = R(q) p_k + t,  q' = quaternion of R(q) (KDL GetQuaternion)
 */
int msnap_formation_transform(msnap_ctx *ctx, int n_poses, int n_offsets,
                              const double *rb_pose, const double *offsets, double *out);
int msnap_formation_transform_device(msnap_ctx *ctx, int n_poses, int n_offsets,
                                     const double *rb_pose, const double *offsets,
                                     double *out);

/* ---- a5: PiecewisePolynomial.eval on a uniform grid -------------------------------
 * replaces src/optimizations/uav_trajectory.py:154-169 (strict '<' lookup, the
 * last piece extrapolates) sampled as np.arange(0, .., dt) (scripts/path_vis.py:28,
 * src/trajectory_visualising/visualization.py:53).
 *   pos [n_drones][n_samples][n_axes]  (n_axes = 3: x,y,z; 4: + yaw), sample s at t = s*dt
 */
int msnap_sample(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef,
                 const double *dur, double dt, int n_samples, int n_axes, double *pos);
int msnap_sample_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef,
                        const double *dur, double dt, int n_samples, int n_axes,
                        double *pos);

/* ---- Trajectory.eval / Polynomial4D.eval: differential-flatness outputs -------------
 * replaces src/optimizations/uav_trajectory.py:64-85 (pos, vel, acc, omega, yaw from the
 * x,y,z,yaw polynomials) with the piece lookup of Trajectory.eval, :119-127 ('<=').
 *   ts  [n_samples] sample times shared by all drones
 *   out [n_drones][n_samples][13] = pos[3] vel[3] acc[3] omega[3] yaw ; NaN outside [0, duration]
 */
int msnap_eval_flat(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                    int n_samples, const double *ts, double *out);
int msnap_eval_flat_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef,
                           const double *dur, int n_samples, const double *ts, double *out);

/* ---- snap cost J = sum_seg int (p^(k))^2 dt per drone and axis (k = 4 at order 7) ------
 * The objective whose KKT system the reference's collocation rows encode
 * (src/optimizations/calculatingTrajectories.py:13-33 states the conditions; the
 * reference never evaluates J).   cost [n_drones][4]
 */
int msnap_snap_cost(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                    double *cost);
int msnap_snap_cost_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef,
                           const double *dur, double *cost);

/* ---- dynamic limits: certified peaks and uniform retiming (new capability) ----
 * The reference gives every path the grid t_i = i*10/n (scripts/drones_pols_generator.py:44-46,56) and checks the
 * result against nothing.  For each drone, over the closed range [0, sum(dur)], each segment on its closed [0, T_i]:
 *   q = 0  speed         max |p'(t)|    (Euclidean norm of the x, y, z derivative)
 *   q = 1  acceleration  max |p''(t)|
 *   q = 2  jerk          max |p'''(t)|
 *   q = 3  yaw rate      max |psi'(t)|
 *   peak   [n_drones][4]  a value the trajectory ATTAINS (SI units), up to rounding (below), at
 *   t_peak [n_drones][4]  absolute time, 0 <= t_peak <= sum(dur) as msnap_eval_flat accumulates it (both ends
 *                         included: msnap_eval_flat at t_peak is finite).  If S is the supremum for the exact real
 *                         polynomials of the fp64 coefficients:
 *                           S (1 - 1e-9) - 1e-12 - r_q  <=  peak  <=  S (1 + 1e-12) + 1e-12 + r_q
 *                           r_q = C_ROUND_PEAKS * 2^-52 * R_q,   C_ROUND_PEAKS = 17
 *                         R_q is the size of what the value is summed from: the largest value, over the quantity's
 *                         axes and the drone's segments i, of sum_j |d_j| T_i^j, d the coefficients of the r-th
 *                         derivative of that axis (r = q + 1; yaw rate: r = 1) and T_i the segment's duration.  peak is
 *                         the segment's polynomial at its local time T_i u, recomputed by msnap_eval_flat's Horner,
 *                         which is good to an ulp of that sum, not of the value: for a solved path r_q is some 1e-14
 *                         of the peak, for a segment whose speed oscillates between equal extrema (R_q 2e4 to 7e5
 *                         times the value) 1e-10 to 3e-9 of it.  (C_ROUND_PEAKS: ten times the worst
 *                         |peak - exact value at T_i u| / (2^-52 R_q) measured, 1.64 -- DESIGN.md §5 K7.)
 *                         t_peak = (start of the segment, the running fp64 sum of dur) + T_i u is rounded once more,
 *                         by up to half an ulp of t_peak, and r_q does NOT cover what that does to the value: on a
 *                         steep flank 1500 segments into a path the exact polynomial at t_peak differs from peak
 *                         by 7 times r_q, and by more further on.  What holds is
 *                           | peak - |p^(r)(t_peak)| |  <=  r_q + 2^-52 * t_peak * R'_q
 *                         with R'_q the size of the NEXT derivative, the largest sum_j j |d_j| T_i^(j-1) over the same
 *                         axes and segments (proven: half an ulp of t_peak times that sum per axis, sqrt(3) for the
 *                         norm), the polynomial being that of the segment msnap_eval_flat's lookup selects at t_peak.
 *                         The second term is zero at t_peak = 0 and negligible where the peak is a stationary point
 *                         of the quantity -- every interior peak of a solved path.  The inequality against S does not
 *                         involve t_peak.  A caller computes R_q and R'_q from coef and dur alone.
 *                         Ties and near-ties: the larger value, then the earlier time.  A stationary drone reports
 *                         peaks <= 1e-12.
 *                         Coefficient sets whose derivative of order r jumps at a knot (no solve produces one): the
 *                         peak may sit on either side of the jump; t_peak names the knot, and the value is that of
 *                         the segment that holds it.  msnap_eval_flat at the same time evaluates the EARLIER segment, so
 *                         it gives the peak back only when that one holds it.
 *                         The search ends a lane at 40 bisections of a segment or 4096 nodes with the best value seen;
 *                         no status is raised for it, and the inequality above is not proven for such a lane (the
 *                         clearances carry a proven bound for theirs; the peaks do not).  No input is known that gets
 *                         there: the most found is 183 nodes, on the order-9 equioscillating speed, and none of the
 *                         families of tools/limits_rounding.py meets a cap.
 *   status [n_drones]     msnap_status: MSNAP_ST_NONFINITE for a NaN / Inf coefficient or duration (what a failed
 *                         solve leaves), else MSNAP_ST_TIMES for a duration <= 0; peak and t_peak are NaN then.
 * A drone's results are bit-identical whatever its position in the batch, the batch size, or host versus device entry.
 * Both orders, n_seg 1 .. max_segments.  (Method: branch and bound on Bernstein bounds of |.|^2 per segment.)
 */
int msnap_dynamic_peaks(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, double *peak,
                        double *t_peak, int32_t *status);
int msnap_dynamic_peaks_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                               double *peak, double *t_peak, int32_t *status);
/* Uniform retiming.  Both orders impose homogeneous end conditions (derivatives 1..3 zero at order 7, 1..4 at order 9)
 * and continuity of derivatives 1..6 (1..8) at the knots, so the solution for the times k t is the same path run k
 * times slower: segment i keeps its polynomial with c_j -> c_j k^-j and T_i -> k T_i (derivative q scales by k^-q) --
 * no second solve.
 *   msnap_time_scale        applies a given scale [n_drones] (c_j times r^j with r = 1/k by repeated multiplication,
 *                           T times k); a scale that is not finite and > 0 copies the drone unchanged.  The building
 *                           block of a common scale over several ranks.
 *   msnap_retime_to_limits  limits[4] = (speed, acceleration, jerk, yaw rate), a HOST array in both versions; 0 or
 *                           +inf: unconstrained; negative or NaN: MSNAP_EINVAL.  Per drone, from peak (1 + 2e-9) (so
 *                           that the limits hold for the true supremum):
 *                             k = max(v / v_lim, sqrt(a / a_lim), cbrt(j / j_lim), yr / yr_lim)
 *                           flags 0: stretch only, k = max(k, 1);  MSNAP_RETIME_FIT: k may be below 1 -- the fastest
 *                           uniform retiming whose tightest limit is just met (k = 1 when nothing is constrained or
 *                           every peak is 0);  MSNAP_RETIME_COMMON: one k for all drones of the call, their maximum
 *                           (failed drones ignored, as fmax does): a formation stays in step.
 *                           scale [n_drones] receives k; a failed drone (status != 0 above) passes through unchanged,
 *                           with scale NaN.
 * coef_out / dur_out may be coef / dur (in place).  Device versions only launch (no synchronisation).
 */
enum msnap_retime_flags {
  MSNAP_RETIME_FIT = 1,
  MSNAP_RETIME_COMMON = 2
};
int msnap_time_scale(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                     const double *scale, double *coef_out, double *dur_out);
int msnap_time_scale_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                            const double *scale, double *coef_out, double *dur_out);
int msnap_retime_to_limits(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                           const double limits[4], int flags, double *coef_out, double *dur_out, double *scale);
int msnap_retime_to_limits_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                  const double limits[4], int flags, double *coef_out, double *dur_out,
                                  double *scale);

/* ---- pairwise clearance in continuous time (new capability) ----
 * The formation pass takes its minimum distance on the sampling grid and can miss a crossing between two samples.
 * msnap_pair_clearance certifies the distance of listed pairs of drones of ONE coef / dur batch (same order, same n_seg,
 * per-drone durations) between the samples as well.  For pair p = (a, b) = pairs[p][0..1] the window is
 * [0, min(sum dur_a, sum dur_b)] -- while both fly; a drone that has landed is NOT held at its end point, what happens
 * after the shorter path ends is out of scope.  D is the infimum of |p_a(t) - p_b(t)| over the window for the exact
 * real polynomials of the fp64 coefficients.
 *   min_dist [n_pairs]  a distance the pair ATTAINS, at
 *   t_min    [n_pairs]  absolute time, 0 <= t_min <= window (smaller value, then the earlier time): msnap_eval_flat of
 *                       the two drones at t_min gives positions whose distance is min_dist;
 *   lower    [n_pairs]  a proven lower bound:  lower <= D <= min_dist, each up to rounding (ten times the worst
 *                       deviation measured against an exact reference):
 *                         lower <= D (1 + 1e-13) + r   and   D <= min_dist (1 + 1e-13) + r,
 *                         r = 1e-13 + C_ROUND * 2^-52 * R   [m],   C_ROUND = 8
 *                       R is the size of what the pair's positions are computed from: the largest value of
 *                       sum_k |c_k| T_i^k over x, y, z, both drones and every segment i that starts before the window
 *                       ends (c_k the segment's coefficients, T_i its duration).  The positions of the two drones are
 *                       rounded to an ulp of the coordinate, not of the distance: two drones 1 m apart at 5000 m from
 *                       the origin carry 1e-12 m of it, and a rest-to-rest segment of 2000 m has R = 4e5 m whatever
 *                       its duration.  A caller computes R from coef and dur alone.
 *                       When the search closes (always, short of its caps: 40 bisections of an interval between knots,
 *                       4096 nodes per interval):  lower >= min_dist (1 - 1e-9) - 1e-9 - r  -- the absolute term
 *                       A = 1e-9 m is what lets a crossing (D = 0) close.  A pair that meets a cap still gets a valid
 *                       lower, only further from min_dist; no status is raised for it (two drones that cross at
 *                       560 m/s on one 11 s segment of order 9 meet the depth cap).
 *   status   [n_pairs]  msnap_status: MSNAP_ST_PAIR for an index outside [0, n_drones) or a == b (nothing is read for
 *                       such a pair), else MSNAP_ST_NONFINITE for a NaN / Inf coefficient or duration of either drone,
 *                       else MSNAP_ST_TIMES for a duration <= 0.  min_dist, t_min and lower of a failed pair are NaN.
 * A pair's outputs are bit-identical whatever its place in the list, the list's length, host versus device entry, and
 * for (b, a) in place of (a, b).  n_pairs == 0 is a no-op.  The device version only launches; its scratch is a buffer
 * of the context under the capture rules above (MSNAP_ECAPTURE: run the call once outside the capture first).
 * (Method: per interval between consecutive knots of the two drones, branch and bound on Bernstein bounds of the
 * squared norm of the DIFFERENCE polynomial.)
 */
int msnap_pair_clearance(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_pairs,
                         const int32_t *pairs, double *min_dist, double *t_min, double *lower, int32_t *status);
int msnap_pair_clearance_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                int n_pairs, const int32_t *pairs, double *min_dist, double *t_min, double *lower,
                                int32_t *status);

/* ---- cross clearance: two path sets on shifted clocks (new capability) ----
 * msnap_pair_clearance takes both drones from one batch on one clock.  A replanned path (msnap_solve_states) starts at
 * its own time, with its own segment count.  msnap_cross_clearance certifies the distance of drone a of set A and drone
 * b of set B for the listed pairs p = (a, b) = pairs[p][0..1] (index in A, index in B).  Both sets have the context's
 * order; n_seg_a and n_seg_b are independent, each 1 .. max_segments; the two sets may be the same arrays.
 * Clock.  Drone a of set A is at P_a(t - t0_a[a]) at common-clock time t, P_a its piecewise polynomial with knots at
 * the fp64 running sums of dur_a, as everywhere else; set B likewise.  t0_a [n_a] and t0_b [n_b] may each be NULL:
 * zeros.
 * Window.  [S, W] with S = max(t0_a[a], t0_b[b]) and W = min(fl(t0_a[a] + total_a), fl(t0_b[b] + total_b)), total the
 * running sum of the drone's durations: while both fly.  A drone that has landed is NOT held at its end point, as for
 * msnap_pair_clearance.  D is the infimum of the distance over the window for the exact real polynomials of the fp64
 * coefficients, with the exact sums t0 + knot as knots.
 *   min_dist [n_pairs]  a distance the pair ATTAINS, at
 *   t_min    [n_pairs]  common-clock time, S <= t_min <= W (smaller value, then the earlier time).  Attained bit for
 *                       bit: with tau_x = min(max(fl(t_min - t0_x), 0), total_x) for each of the two drones,
 *                       msnap_eval_flat of drone a at tau_a and of drone b at tau_b gives positions whose
 *                       sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) is min_dist;
 *   lower    [n_pairs]  a proven lower bound.  The inequalities are msnap_pair_clearance's,
 *                         lower <= D (1 + 1e-13) + r   and   D <= min_dist (1 + 1e-13) + r,
 *                         lower >= min_dist (1 - 1e-9) - 1e-9 - r   when the search closes (same caps: 40 bisections
 *                         of an interval between knots, 4096 nodes per interval),
 *                       with
 *                         r = 1e-13 + C_ROUND_CROSS * 2^-52 * R + C_CLOCK * 2^-52 * T_c * R'   [m],
 *                         C_ROUND_CROSS = 7,   C_CLOCK = 1
 *                       R is msnap_pair_clearance's R over the segments of either drone that meet the window (the
 *                       largest sum_k |c_k| T_i^k over x, y, z); T_c = max(|S|, |W|); R' is the largest
 *                       sum_j j |c_j| T_i^(j-1) over the same axes, drones and segments -- the size of the velocity, as
 *                       R'_q of msnap_dynamic_peaks.  The clock term is there because a local time fl(t - t0) is off by
 *                       up to an ulp of t: at t0 = 1e4 s a drone at 10 m/s carries 2e-11 m of it.  Both constants are
 *                       ten times the worst deviation measured against an exact reference.
 *   status   [n_pairs]  msnap_status, first condition wins: MSNAP_ST_PAIR for an index outside [0, n_a) or [0, n_b)
 *                       (nothing is read for such a pair; a == b is legal here), else MSNAP_ST_NONFINITE for a NaN /
 *                       Inf coefficient, duration or t0 of either drone, else MSNAP_ST_TIMES for a duration <= 0.
 *                       min_dist, t_min and lower of a failed pair are NaN.
 * W < S (the drones never fly at the same time): min_dist = lower = +inf, t_min = NaN, status 0.  W == S: the distance
 * at that one instant, t_min = S, lower = min_dist.
 * Bit identities.  A pair's outputs do not depend on its place in the list or on the list's length; host entry and
 * device entry give the same bits; NULL and an array of zeros give the same bits; exchanging the two sets, with the
 * pairs flipped, gives the same bits; and with A == B, equal segment counts and zero offsets the outputs are bit for
 * bit those of msnap_pair_clearance (a != b).
 * n_pairs == 0 is a no-op.  MSNAP_EINVAL: a null context, a null array other than t0_a / t0_b, negative sizes, a launch
 * grid beyond 2^31 blocks; MSNAP_ESEGMENTS per set as everywhere.  The device version only launches; its scratch is a
 * buffer of the context under the capture rules above (MSNAP_ECAPTURE: run the call once outside the capture first).
 * (Method: msnap_pair_clearance's, on the merged knots of the two drones on the common clock.)
 */
int msnap_cross_clearance(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                          const double *t0_a, int n_b, int n_seg_b, const double *coef_b, const double *dur_b,
                          const double *t0_b, int n_pairs, const int32_t *pairs, double *min_dist, double *t_min,
                          double *lower, int32_t *status);
int msnap_cross_clearance_device(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                                 const double *t0_a, int n_b, int n_seg_b, const double *coef_b, const double *dur_b,
                                 const double *t0_b, int n_pairs, const int32_t *pairs, double *min_dist, double *t_min,
                                 double *lower, int32_t *status);

/* ---- conflict windows: from when until when a pair is too close (new capability) ----
 * msnap_pair_clearance / msnap_cross_clearance say that two paths come too close and where they are closest; t_min lies
 * INSIDE the violation.  These entries certify the interval during which |p_a(t) - p_b(t)| < threshold: the latest safe
 * hand-over time of a replan, how long one drone must wait for the other to pass, which of two conflicts comes first.
 * msnap_pair_conflict_window takes both drones from one batch on one clock, msnap_cross_conflict_window drone a of set A
 * and drone b of set B on shifted clocks.  The window [S, W], the clocks, the knots, the pair rules, the status
 * precedence and the capture rules are exactly those of msnap_pair_clearance / msnap_cross_clearance.
 *   threshold  a centre distance [m], finite and >= 0;   t_res  the time resolution [s], finite and > 0
 *              (either outside its range: MSNAP_EINVAL).
 * A pair is IN CONFLICT at t when its distance is < threshold (strict, as the sampled pass's md < 2 radius) and CLEAR at
 * t when its distance is >= threshold.  Outputs, each [n_pairs]:
 *   t_clear_until  proven: clear for every t in [S, t_clear_until);
 *   t_first        the earliest time found at which the pair is in conflict (+inf: none found);
 *   d_first        the distance at t_first, formed in the t domain exactly as the clearance entries form min_dist:
 *                  msnap_eval_flat of the two drones at t_first (cross: at the clamped local times
 *                  tau_x = min(max(fl(t_first - t0_x), 0), total_x)) gives positions whose
 *                  sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) is d_first bit for bit (+inf: no t_first);
 *   t_last, d_last the latest such time and its distance (-inf / +inf: none);
 *   t_clear_from   proven: clear for every t in (t_clear_from, W];
 *   status         as for the clearance entries; every double output of a failed pair is NaN.
 * Always S <= t_clear_until <= t_first <= t_last <= t_clear_from <= W, where the values are finite.  Verdicts:
 *   certified clear over the whole window   t_clear_until = +inf, t_clear_from = -inf, t_first = +inf, t_last = -inf;
 *   undecided        no conflict found, but t_clear_until is finite: a graze the search could not separate within its
 *                    caps.  t_clear_until and t_clear_from still hold;
 *   closed search    t_first - t_clear_until <= t_res and t_clear_from - t_last <= t_res: always so for a transversal
 *                    crossing.  The caps are msnap_pair_clearance's: 40 bisections of an interval between knots, 4096
 *                    nodes per interval.
 *   W < S (cross): certified clear.  W == S: the one instant decides (in conflict: all four times are S).
 * Rounding.  "Proven" and "in conflict" hold up to the rounding allowance r of the matching clearance entry
 * (msnap_pair_clearance: r = 1e-13 + C_ROUND 2^-52 R; msnap_cross_clearance: r = 1e-13 + C_ROUND_CROSS 2^-52 R +
 * C_CLOCK 2^-52 T_c R', with the constants, R, R' and T_c stated there).  For the exact real polynomials of the fp64
 * coefficients:
 *     distance >= threshold - r   at every t of [S, t_clear_until) and of (t_clear_from, W],
 *     distance at t_first and at t_last  <  threshold + r.
 * Bit identities.  A pair's outputs do not depend on its place in the list or on the list's length; host entry and
 * device entry give the same bits; NULL and an array of zeros give the same bits; exchanging the two sets, with the
 * pairs flipped, gives the same bits; with A == B, equal segment counts and zero offsets the cross entry gives the pair
 * entry's bits; (b, a) gives the bits of (a, b).
 * n_pairs == 0 is a no-op.  The device versions only launch; their scratch is a buffer of the context under the capture
 * rules above (MSNAP_ECAPTURE: run the call once outside the capture first).
 * (Method: per interval between consecutive knots, a time-ordered walk over dyadic sub-intervals in both directions --
 * a node whose smallest Bernstein coefficient of |difference|^2 is >= threshold^2 is clear, a node that starts in
 * conflict ends the walk, a node shorter than t_res is a leaf.  A later interval does not know that an earlier one
 * already holds the first conflict: every interval is walked.)
 */
int msnap_pair_conflict_window(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                               int n_pairs, const int32_t *pairs, double threshold, double t_res,
                               double *t_clear_until, double *t_first, double *d_first, double *t_last, double *d_last,
                               double *t_clear_from, int32_t *status);
int msnap_pair_conflict_window_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                      int n_pairs, const int32_t *pairs, double threshold, double t_res,
                                      double *t_clear_until, double *t_first, double *d_first, double *t_last,
                                      double *d_last, double *t_clear_from, int32_t *status);
int msnap_cross_conflict_window(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                                const double *t0_a, int n_b, int n_seg_b, const double *coef_b, const double *dur_b,
                                const double *t0_b, int n_pairs, const int32_t *pairs, double threshold, double t_res,
                                double *t_clear_until, double *t_first, double *d_first, double *t_last, double *d_last,
                                double *t_clear_from, int32_t *status);
int msnap_cross_conflict_window_device(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                                       const double *t0_a, int n_b, int n_seg_b, const double *coef_b,
                                       const double *dur_b, const double *t0_b, int n_pairs, const int32_t *pairs,
                                       double threshold, double t_res, double *t_clear_until, double *t_first,
                                       double *d_first, double *t_last, double *d_last, double *t_clear_from,
                                       int32_t *status);

/* ---- mesh clearance in continuous time (new capability) ----
 * msnap_mesh_sweep takes the point-triangle distance on the sampling grid only, and an STL wall has no thickness: a
 * drone that passes it at 4 m/s has its 0.1 s samples 0.2 m either side of it.  msnap_mesh_clearance certifies the
 * distance of each drone's whole path to the mesh.  coef, dur as everywhere else; tris [n_tris][3][3] as for
 * msnap_mesh_sweep; every output is [n_drones].  Per drone, D is the infimum of the sweep's distance function over t in
 * [0, sum dur] (each segment on its closed [0, T_i]) and over all triangles, for the exact real polynomials of the fp64
 * coefficients.  A triangle the sweep takes as degenerate counts as the union of its three edges, as there; a triangle
 * with a non-finite vertex never wins and is skipped.
 *   min_dist  a distance the drone ATTAINS, at
 *   t_min     absolute time, against triangle
 *   tri_min   (smaller value, then the earlier time, then the lowest triangle index): msnap_mesh_sweep of the single
 *             position msnap_eval_flat gives at t_min, over the whole mesh, returns min_dist bit for bit;
 *   lower     a proven lower bound:  lower <= D <= min_dist, each up to rounding (ten times the worst deviation
 *             measured against an exact reference):
 *               lower <= D (1 + 1e-13) + r   and   D <= min_dist (1 + 1e-13) + r,
 *               r = 1e-13 + C_ROUND_MESH * 2^-52 * R   [m],   C_ROUND_MESH = 3
 *             R = the largest value of sum_k |c_k| T_i^k over x, y, z and the drone's segments (msnap_pair_clearance's
 *             R for one drone) plus the largest |vertex coordinate| of the mesh's finite triangles.
 *             When the search closes (short of its caps: 40 bisections of a segment, 4096 nodes per segment):
 *               lower >= min_dist (1 - 1e-9) - 1e-9 - r.
 *             A drone that meets a cap still gets a valid lower, only further from min_dist; no status is raised.  The
 *             closing inequality is not promised against a degenerate triangle of non-zero area (the bound is the
 *             hull's, which is below the edge-union distance inside the sliver); it is for zero-area triangles.
 *   status    msnap_status: MSNAP_ST_NONFINITE for a NaN / Inf coefficient or duration of the drone, else
 *             MSNAP_ST_TIMES for a duration <= 0.  min_dist, t_min and lower of a failed drone are NaN, tri_min -1.
 * n_tris == 0 (or no triangle with finite vertices): min_dist = lower = +inf, t_min = 0, tri_min = -1, status as
 * above.  n_drones == 0 is a no-op.  MSNAP_EINVAL: a null context, a null array, negative sizes, tris == NULL with
 * n_tris > 0.  A drone's outputs are bit-identical whatever its place in the batch, the batch size, and host versus
 * device entry.  The device version only launches; its scratch is a buffer of the context under the capture rules above
 * (MSNAP_ECAPTURE: run the call once outside the capture first).
 * (Method: per segment, branch and bound over dyadic sub-intervals; a sub-interval's Bernstein control points enclose
 * the path, and for any |n| <= 1 the distance to a triangle is at least min_k n.b_k - max_j n.v_j; n is tried as the
 * two face normals and the direction away from the triangle at the sub-interval's farthest point.)
 */
int msnap_mesh_clearance(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_tris,
                         const double *tris, double *min_dist, double *t_min, int32_t *tri_min, double *lower,
                         int32_t *status);
int msnap_mesh_clearance_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                int n_tris, const double *tris, double *min_dist, double *t_min, int32_t *tri_min,
                                double *lower, int32_t *status);

/* ---- mesh conflict windows: from when until when a path is too close to a mesh (new capability) ----
 * msnap_mesh_clearance says that a path comes too close to the mesh and where it is closest; t_min lies INSIDE the
 * violation.  This entry certifies the interval during which the distance is < threshold: from when a replan has to
 * have taken over, and when the drone is out of the margin again.  It is msnap_pair_conflict_window with a mesh in the
 * place of the second drone.  coef, dur, tris as for msnap_mesh_clearance; every output is [n_drones].  The window of a
 * drone is [0, W], W the running fp64 sum of its durations as msnap_eval_flat accumulates it, each segment on its closed
 * [0, T_i].  The distance is the sweep's: the minimum over the triangles with finite vertices; a triangle the sweep
 * takes as degenerate counts as the union of its three edges; a triangle with a non-finite vertex is skipped.
 *   threshold  a distance [m], finite and >= 0;   t_res  the time resolution [s], finite and > 0
 *              (either outside its range: MSNAP_EINVAL, also with n_drones == 0).
 * A drone is IN CONFLICT at t when its distance is < threshold (strict, as the sweep's min_dist < radius) and CLEAR at t
 * when its distance is >= threshold.  Outputs:
 *   t_clear_until  proven: clear for every t in [0, t_clear_until);
 *   t_first        the earliest time found at which the drone is in conflict (+inf: none found);
 *   d_first        the distance at t_first by msnap_mesh_clearance's rule for min_dist: msnap_mesh_sweep of the single
 *                  position msnap_eval_flat gives at t_first, over the whole mesh, returns d_first bit for bit (+inf: no
 *                  t_first);
 *   tri_first      the lowest triangle index that attains d_first (-1: none);
 *   t_last, d_last, tri_last   the latest such time, its distance and triangle (-inf / +inf / -1: none);
 *   t_clear_from   proven: clear for every t in (t_clear_from, W];
 *   status         as for msnap_mesh_clearance (MSNAP_ST_NONFINITE, then MSNAP_ST_TIMES); the six doubles of a failed
 *                  drone are NaN, both triangle outputs -1.
 * Always 0 <= t_clear_until <= t_first <= t_last <= t_clear_from <= W, where the values are finite.  Verdicts:
 *   certified clear over the whole window   t_clear_until = t_first = d_first = +inf, tri_first = -1, t_last = -inf,
 *                    d_last = +inf, tri_last = -1, t_clear_from = -inf.  n_tris == 0, or no finite triangle, gives this;
 *   undecided        no conflict found, but t_clear_until is finite: a graze the search could not separate within its
 *                    caps.  t_clear_until and t_clear_from still hold;
 *   closed search    t_first - t_clear_until <= t_res and t_clear_from - t_last <= t_res: always so for a transversal
 *                    entry and exit.  The caps are msnap_mesh_clearance's: 40 bisections of a segment, 4096 nodes per
 *                    segment and direction.  Against a degenerate triangle of non-zero area the closing is not promised
 *                    (the bound is the hull's, as there); the proven ranges still hold.
 * Rounding.  "Proven" and "in conflict" hold up to an allowance of msnap_mesh_clearance's form,
 *     r = 1e-13 + C_ROUND_MESH_WINDOW * 2^-52 * R   [m],   C_ROUND_MESH_WINDOW = 8,   R as for msnap_mesh_clearance.
 * For the exact real polynomials of the fp64 coefficients:
 *     distance >= threshold - r   at every t of [0, t_clear_until) and of (t_clear_from, W],
 *     distance at t_first and at t_last  <  threshold + r.
 * (The constant is ten times the worst deviation measured against an exact reference, 0.732, rounded up -- more than
 * msnap_mesh_clearance's C_ROUND_MESH = 3, which that measurement does not stay below: DESIGN.md §5 K19.)
 * An entry or exit that falls exactly on a boundary of the search's dyadic subdivision of a segment has the distance
 * EQUAL to the threshold at a node's end; the last bit then decides whether that node is proven clear, and the gap on
 * that side can be up to 2 t_res.
 * n_drones == 0 is a no-op.  MSNAP_EINVAL, MSNAP_ESEGMENTS and the grid limit are msnap_mesh_clearance's.  A drone's
 * outputs are bit-identical whatever its place in the batch, the batch size, and host versus device entry.  The device
 * version only launches; its scratch is msnap_mesh_clearance's buffer of the context under the capture rules above
 * (MSNAP_ECAPTURE: run the call once outside the capture first).
 * (Method: per segment a time-ordered walk over dyadic sub-intervals in both directions.  A node whose support-plane
 * bound, msnap_mesh_clearance's, is >= threshold is clear; a triangle whose bounding box lies threshold or more from the
 * box of the node's control points is left out of the node; a node that starts in conflict ends the walk; a node
 * shorter than t_res is a leaf.  A later segment does not know that an earlier one already holds the first conflict:
 * every segment is walked.)
 */
int msnap_mesh_conflict_window(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                               int n_tris, const double *tris, double threshold, double t_res,
                               double *t_clear_until, double *t_first, double *d_first, int32_t *tri_first,
                               double *t_last, double *d_last, int32_t *tri_last, double *t_clear_from,
                               int32_t *status);
int msnap_mesh_conflict_window_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                      int n_tris, const double *tris, double threshold, double t_res,
                                      double *t_clear_until, double *t_first, double *d_first, int32_t *tri_first,
                                      double *t_last, double *d_last, int32_t *tri_last, double *t_clear_from,
                                      int32_t *status);

/* ---- path extent in continuous time: the support function of a path (new capability) ----
 * The peaks, the pairwise clearance and the mesh clearance say nothing about WHERE a path goes, and a minimum-snap fit
 * through waypoints inside a workspace overshoots it between them.  msnap_path_extent certifies, per drone and per given
 * direction, how far the whole path reaches in that direction.  coef, dur as everywhere else; dirs [n_dirs][3]
 * (directions need not have unit length); ext, t_ext and upper are [n_drones][n_dirs], status is [n_drones].  For
 * direction n_k and one drone, S is the supremum of n_k.p(t) over t in [0, sum dur] (each segment on its closed
 * [0, T_i]), for the exact real polynomials of the fp64 coefficients and the fp64 direction.  The six signed axes give
 * the certified bounding box of a path; the normals of half-spaces n.x <= b a convex geofence or corridor.
 *   ext      a value the path ATTAINS, at
 *   t_ext    absolute time, 0 <= t_ext <= sum dur (larger value, then the earlier time): for the position (x, y, z)
 *            msnap_eval_flat gives at t_ext, (n_x * x + n_y * y) + n_z * z -- every operation rounded once, in this
 *            order, none fused -- is ext bit for bit;
 *   upper    a proven upper bound:  ext <= upper always, and ext <= S <= upper, each up to rounding (ten times the worst
 *            deviation measured against an exact reference):
 *              ext <= S + r   and   S <= upper + r,
 *              r = 1e-13 + C_ROUND_EXTENT * 2^-52 * R_k,   C_ROUND_EXTENT = 9
 *            R_k = the largest value, over the drone's segments i, of sum_a |n_a| sum_j |c_{a,j}| T_i^j (a over x, y, z;
 *            c_{a,j} the segment's coefficients, T_i its duration): the size of what n_k.p is computed from.  A caller
 *            computes R_k from coef, dur and dirs alone.
 *            When the search closes (short of its caps: 40 bisections of a segment, 4096 nodes per segment):
 *              upper <= ext + 1e-9 |ext| + 1e-9 + r.
 *            A lane that meets a cap still gets a valid upper, only further from ext; no status is raised.
 *            No solve produces coefficient sets whose position jumps at a knot.  For such a set t_ext may name the
 *            knot, and ext is the value of the segment that msnap_eval_flat's lookup selects there; upper still bounds
 *            both sides; the closing inequality is not promised.
 *   status   msnap_status: MSNAP_ST_NONFINITE for a NaN / Inf coefficient or duration of the drone, else
 *            MSNAP_ST_TIMES for a duration <= 0.  ext, t_ext and upper of a failed drone are NaN.
 * A direction with a non-finite component has NaN in its column for every drone; status is unaffected.  A zero
 * direction gives ext = upper = 0 at t_ext = 0.  n_dirs == 0 or n_drones == 0 is a no-op.  MSNAP_EINVAL: a null context,
 * a null array, negative sizes, dirs == NULL with n_dirs > 0, n_drones * n_seg * n_dirs beyond what one launch covers.
 * MSNAP_ESEGMENTS as everywhere.  Both orders, n_seg 1 .. max_segments.  An (ext, t_ext, upper) triple is bit-identical
 * whatever the drone's place in the batch, the batch size, the direction's place in dirs, n_dirs, and host versus
 * device entry.  The device version takes device pointers, dirs included, and only launches; its scratch is a buffer of
 * the context under the capture rules above (MSNAP_ECAPTURE: run the call once outside the capture first).
 * (Method: per segment and direction, branch and bound over dyadic sub-intervals on the scalar polynomial n.p; the
 * largest Bernstein coefficient on a sub-interval bounds it there.)
 */
int msnap_path_extent(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_dirs,
                      const double *dirs /* [n_dirs][3] */, double *ext, double *t_ext, double *upper, int32_t *status);
int msnap_path_extent_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                             int n_dirs, const double *dirs, double *ext, double *t_ext, double *upper,
                             int32_t *status);

/* ---- half-space windows: from when until when a path is outside a half-space (new capability) ----
 * msnap_path_extent reports one extreme per direction over the whole flight; it cannot say WHEN a path leaves a
 * half-space n.x <= b or when it is back inside.  This entry certifies that, per query and from a start time of the
 * query's own: what a safe flight corridor needs (a chain of overlapping convex polytopes; the path must stay in one
 * until it is inside the next), and the time-resolved sibling of the geofence.  It is msnap_pair_conflict_window with a
 * half-space in the place of the second drone.  coef, dur as everywhere else.
 *   planes   [n_planes][4] = (n_x, n_y, n_z, b): inside is n.x <= b; the normals need not have unit length;
 *   queries  int32 [n_queries][2] = (drone, plane): index into the batch, index into planes;
 *   t_from, t_to  [n_queries] each, or NULL: the query's range is [S, W] = [max(t_from, 0), min(t_to, total)], total the
 *            running fp64 sum of the drone's durations as msnap_eval_flat accumulates it.  NULL t_from means 0, NULL t_to
 *            the whole flight; NULL gives the same bits as an array of zeros / of the totals;
 *   t_res    the time resolution [s], finite and > 0 (else MSNAP_EINVAL, also with n_queries == 0).
 * A query is OUTSIDE at t when n.p(t) > b (strict: a path that only touches a limit is not outside) and INSIDE at t when
 * n.p(t) <= b.  Outputs, each [n_queries]:
 *   t_inside_until  proven: inside for every t in [S, t_inside_until);
 *   t_first         the earliest time found at which the path is outside (+inf: none found);
 *   v_first         n.p at t_first, formed as msnap_path_extent forms ext: for the position (x, y, z) msnap_eval_flat
 *                   gives at t_first, (n_x * x + n_y * y) + n_z * z -- every operation rounded once, in this order, none
 *                   fused -- is v_first bit for bit (-inf: no t_first);
 *   t_last, v_last  the latest such time and its value (-inf / -inf: none);
 *   t_inside_from   proven: inside for every t in (t_inside_from, W];
 *   status          msnap_status, first condition wins: MSNAP_ST_PAIR for a drone index outside [0, n_drones) or a plane
 *                   index outside [0, n_planes) (nothing is read for such a query), else MSNAP_ST_NONFINITE for a NaN /
 *                   Inf coefficient or duration of the drone or a NaN / Inf t_from or t_to of the query, else
 *                   MSNAP_ST_TIMES for a duration <= 0.  The six doubles of a failed query are NaN.
 * Always S <= t_inside_until <= t_first <= t_last <= t_inside_from <= W, where the values are finite.  Verdicts:
 *   certified inside over the whole range   t_inside_until = t_first = +inf, t_last = t_inside_from = -inf;
 *   undecided        nothing found outside, but t_inside_until is finite: a graze the search could not separate within
 *                    its caps.  t_inside_until and t_inside_from still hold;
 *   closed search    t_first - t_inside_until <= t_res and t_inside_from - t_last <= t_res: always so for a transversal
 *                    crossing.  The caps are msnap_path_extent's: 40 bisections of a segment, 4096 nodes per segment and
 *                    direction.
 *   W < S: certified inside.  W == S: the one instant decides (outside: all four times are S).
 * A plane with a non-finite entry gives NaN in the six doubles of its queries; their status is the drone's, unaffected
 * (msnap_path_extent's rule for a non-finite direction).  A zero normal is inside when 0 <= b and outside at every
 * instant otherwise (t_inside_until = t_first = S, t_last = t_inside_from = W, both values 0).
 * Rounding.  "Proven" and "outside" hold up to msnap_path_extent's allowance, unchanged:
 *     r = 1e-13 + C_ROUND_EXTENT * 2^-52 * R_k,   C_ROUND_EXTENT = 9,   R_k as stated there for (drone, n).
 * For the exact real polynomials of the fp64 coefficients and the fp64 plane:
 *     n.p(t) <= b + r   at every t of [S, t_inside_until) and of (t_inside_from, W],
 *     n.p at t_first and at t_last  >  b - r.
 * (Measured on the fp64 restatement of the method, not on the kernel, against an exact reference at t_res = 1e-14, both
 * orders, paths shifted by up to 1e5 m: the worst deviation is 0.697 in units of 2^-52 R_k; ten times that
 * stays below C_ROUND_EXTENT = 9, so the entry uses K12's r.  tools/halfspace_window_rounding.py)
 * A crossing that falls exactly on a boundary of the search's dyadic subdivision has n.p EQUAL to b at a node's end;
 * the last bit then decides whether that node is proven inside, and the gap on that side can be up to 2 t_res.
 * Bit identities.  A query's outputs do not depend on its place in the list, on the list's length, on the plane's place
 * in planes or on n_planes; nor on the batch size or the drone's place in the batch; host entry and device entry give
 * the same bits.
 * n_queries == 0 is a no-op.  MSNAP_EINVAL: a null context, a null array other than t_from / t_to, negative sizes, t_res
 * not finite or <= 0, planes == NULL with n_planes > 0, n_queries * n_seg beyond what one launch covers.
 * MSNAP_ESEGMENTS as everywhere.  Both orders, n_seg 1 .. max_segments.  The device version takes device pointers and
 * only launches; its scratch is msnap_path_extent's buffer of the context under the capture rules above
 * (MSNAP_ECAPTURE: run the call once outside the capture first).
 * (Method: one lane per query and segment on the part of the segment inside the range: the scalar polynomial -(n.p),
 * a time-ordered walk over dyadic sub-intervals in both directions against the level -b, which is never rounded into
 * the coefficients -- a node whose smallest Bernstein coefficient is >= -b is proven inside, a node that starts outside
 * ends the walk, a node shorter than t_res is a leaf.  A later segment does not know that an earlier one already holds
 * the first exit: every segment is walked.)
 */
int msnap_halfspace_window(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_planes,
                           const double *planes /* [n_planes][4] = (n, b): inside is n.x <= b */, int n_queries,
                           const int32_t *queries /* [n_queries][2] = (drone, plane) */, const double *t_from,
                           const double *t_to /* [n_queries] each, or NULL */, double t_res, double *t_inside_until,
                           double *t_first, double *v_first, double *t_last, double *v_last, double *t_inside_from,
                           int32_t *status);
int msnap_halfspace_window_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                  int n_planes, const double *planes, int n_queries, const int32_t *queries,
                                  const double *t_from, const double *t_to, double t_res, double *t_inside_until,
                                  double *t_first, double *v_first, double *t_last, double *v_last,
                                  double *t_inside_from, int32_t *status);

/* ---- replanning in flight: solve from and to given end states (new capability) ----
 * Every other solve starts and ends at rest.  msnap_eval_state reads the full state of each drone on its current path
 * at a time of its own; msnap_solve_states solves a new path from such a state, through new waypoints, to a given end
 * state.  With K = (order + 1) / 2:
 *
 * msnap_solve_states.  wp, t, shared_times, coef, dur, status as for msnap_solve_batch.  start and end are
 * [n_drones][4][K-1], axis-major (x, y, z, yaw): entry q-1 is the q-th time derivative at the first / last waypoint, in
 * SI units (velocity, acceleration, jerk; snap too at order 9).  Either may be NULL: rest.  The result minimises the same
 * cost as msnap_solve_batch -- the integral of (p^(K))^2 per axis -- interpolates the waypoints and has derivatives
 * 1 .. K-1 at both ends equal to the given values; coef[0][a][0] is wp[0][a] bit for bit.  msnap_eval_state returns
 * the given start derivatives at tq = 0 within 4 * 2^-52 relative, and the given end derivatives at the sum of the
 * durations (as msnap_eval_flat accumulates it) within 4 * 2^-52 of max(|value|, sum_j |d_j| T^j), d the coefficients
 * of the derivative being evaluated on the last segment: that segment takes one refinement step on its end conditions.
 *   status   MSNAP_ST_NONFINITE for a NaN / Inf waypoint, time or state entry of that drone; MSNAP_ST_TIMES for times
 *            not strictly increasing or t[0] != 0 (as msnap_optimize_times: the reference's quirk of taking segment 0's
 *            start rows at local time t[0] has no meaning for a path that starts from a moving state, so it is not
 *            reproduced here); MSNAP_ST_SINGULAR as in msnap_solve_batch.  A failed drone gets NaN coefficients;
 *            dur[i] = t[i+1] - t[i] is written for every drone.
 *   n_seg    1 .. msnap_solve_states_max_segments(order) -- 47 at order 7, 32 at order 9: what a 16-drone tile's state
 *            leaves of 160 KiB of LDS; a replanning horizon is short -- and at most max_segments; MSNAP_ESEGMENTS above,
 *            and nothing is written.  msnap_solve_states_max_segments returns MSNAP_EORDER for any other order.
 * MSNAP_EINVAL: a null context, a null wp, t, coef, dur or status, negative n_drones.  n_drones == 0 is a no-op.  A
 * drone's outputs are bit-identical whatever its place in the batch, the batch size, and host versus device entry;
 * NULL and an array of zeros give the same bits.  The device version only launches (no synchronisation, no context
 * buffer, so no capture rules).
 *
 * msnap_eval_state.  coef, dur as everywhere else; tq [n_drones]: drone d is evaluated at its own time tq[d].
 *   pos   [n_drones][4]       the value of each axis;
 *   deriv [n_drones][4][K-1]  entry q-1 its q-th derivative: the layout of msnap_solve_states' start, so a replan hands
 *                             deriv over unchanged and copies pos into wp[d][0].
 * The piece lookup is msnap_eval_flat's (the first segment with t <= acc + T_i: a knot belongs to the earlier segment),
 * the arithmetic its Horner carried to derivative K-1: each derivative's coefficients are (double)(i + 1) * d[i + 1] of
 * the previous one's, Horner uses a separate multiply and add, nothing is fused -- reproducible bit for bit in NumPy,
 * and position, first and second derivative are bit for bit msnap_eval_flat's out[0..2], [3..5], [6..8] and yaw out[12]
 * at the same time.  tq[d] outside [0, sum dur], or NaN, gives NaN in that drone's pos and deriv.  Both orders, n_seg
 * 1 .. max_segments.  MSNAP_EINVAL / MSNAP_ESEGMENTS as everywhere; n_drones == 0 is a no-op; the device version only
 * launches.
 */
int msnap_solve_states(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                       const double *start /* [n_drones][4][K-1] or NULL */,
                       const double *end /* [n_drones][4][K-1] or NULL */, double *coef, double *dur, int32_t *status);
int msnap_solve_states_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                              int shared_times, const double *start, const double *end, double *coef, double *dur,
                              int32_t *status);
int msnap_solve_states_max_segments(int order);     /* largest n_seg the entry takes; < 0: MSNAP_EORDER */
int msnap_eval_state(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                     const double *tq /* [n_drones] */, double *pos /* [n_drones][4] */,
                     double *deriv /* [n_drones][4][K-1] */);
int msnap_eval_state_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                            const double *tq, double *pos, double *deriv);

/* ---- gates: prescribed derivatives at interior waypoints (new capability) ----
 * Every other solve treats an interior waypoint as a position only; its velocity, acceleration and jerk (snap too at
 * order 9) are what the minimisation picks.  msnap_solve_gates is msnap_solve_states with any of those prescribed at any
 * interior waypoint: "pass this gate at 3 m/s along its axis", "stop at waypoint 4, then go on", "hold zero
 * acceleration where the payload is released".  wp, t, shared_times, start, end, coef, dur, status as for
 * msnap_solve_states.  With K = (order + 1) / 2:
 *   fix [n_drones][n_seg-1]           int32; entry i-1 is the mask of interior waypoint i (1 .. n_seg-1): bit q-1 set
 *                                     means its q-th time derivative is prescribed, on all four axes of the drone.
 *   via [n_drones][n_seg-1][4][K-1]   the values, per waypoint in the layout of start / end: entry [a][q-1] is the q-th
 *                                     derivative of axis a.  An entry under a clear bit is never used and may be NaN.
 * fix == NULL: no gates -- coef, dur and status are msnap_solve_states' bit for bit, and via may be NULL too; so are
 * they with a mask of zeros.  The result minimises the same cost over the paths that interpolate the waypoints, have
 * the given end states and the prescribed derivatives: derivatives 1 .. K-1 stay continuous at every waypoint, and
 * at a gated one the continuity of derivative 2K-1-q is given up for each prescribed q.  On the segment that leaves a
 * gated waypoint coef[i][a][q] * q! is the prescribed value within 4 * 2^-52 relative; on the segment that arrives it
 * is met as every interior waypoint's continuity is met (DESIGN.md K21 has the figures).  A waypoint with every bit
 * set decouples the two sides: the path is the two msnap_solve_states solutions of its halves, to rounding.
 *   status   as msnap_solve_states, and MSNAP_ST_NONFINITE for a NaN / Inf via entry under a set bit or a fix entry that
 *            is negative or >= 2^(K-1).  A failed drone gets NaN coefficients; dur is written for every drone.
 *   n_seg    1 .. msnap_solve_gates_max_segments(order) -- 47 at order 7, 32 at order 9, msnap_solve_states' range: the
 *            gates take no LDS -- and at most max_segments; MSNAP_ESEGMENTS above, and nothing is written.
 *            msnap_solve_gates_max_segments returns MSNAP_EORDER for any other order.
 * MSNAP_EINVAL: as msnap_solve_states, and fix given without via.  n_drones == 0 is a no-op.  A drone's outputs are
 * bit-identical whatever its place in the batch, the batch size, and host versus device entry.  The device version
 * only launches.  Masks are per drone, not per axis, and the end states are always whole; the time allocation
 * through gates is msnap_optimize_times_gates, and the periodic solves take no gates.
 */
int msnap_solve_gates(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                      const double *start, const double *end,          /* as msnap_solve_states */
                      const int32_t *fix /* [n_drones][n_seg-1] or NULL */,
                      const double *via /* [n_drones][n_seg-1][4][K-1] or NULL */,
                      double *coef, double *dur, int32_t *status);
int msnap_solve_gates_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                             int shared_times, const double *start, const double *end, const int32_t *fix,
                             const double *via, double *coef, double *dur, int32_t *status);
int msnap_solve_gates_max_segments(int order);      /* largest n_seg the entry takes; < 0: MSNAP_EORDER */

/* ---- closed-loop paths: the periodic solve (new capability) ----
 * Every other solve ends at rest or in a state the caller supplies; msnap_solve_periodic joins the last waypoint to the
 * first, for holding patterns and repeating figures.  wp, t, shared_times, coef, dur, status as for msnap_solve_states.
 * With K = (order + 1) / 2:
 *   - the result interpolates every waypoint;
 *   - among all such paths whose derivatives 1 .. K-1 at the last waypoint equal those at the first it minimises the
 *     cost of msnap_solve_batch, the integral of (p^(K))^2 per axis.  The seam's derivatives are free: the minimisation
 *     chooses them;
 *   - consequently derivatives 1 .. 2K-2 are continuous across the seam, exactly as at an interior knot.  The period is
 *     t[n_seg];
 *   - wp[n_seg] need NOT equal wp[0].  The difference is the lap offset: 0 for a closed curve, 2 pi k in yaw for a
 *     turning one, a constant step for a helix.  The library does not judge it;
 *   - coef[i][a][0] is wp[i][a] bit for bit.
 * Through the evaluator: msnap_eval_state at the sum of the durations (as msnap_eval_flat accumulates it) returns
 * derivatives 1 .. K-1 equal to those it returns at tq = 0, and the position wp[n_seg], within the bound
 * msnap_solve_states states for its end state -- 4 * 2^-52 of max(|value|, sum_j |d_j| T^j), d the coefficients of the
 * derivative being evaluated on the last segment: that segment takes the same refinement step on its end conditions,
 * with the solved seam state as its end vector.  Time is not wrapped anywhere: callers reduce t modulo the period.
 *   status   MSNAP_ST_NONFINITE, MSNAP_ST_TIMES (times not strictly increasing, or t[0] != 0) and MSNAP_ST_SINGULAR
 *            (the seam knot's pivots are tested like every other knot's) as in msnap_solve_states.  A failed drone gets
 *            NaN coefficients; dur[i] = t[i+1] - t[i] is written for every drone.
 *   n_seg    2 .. msnap_solve_periodic_max_segments(order) -- 27 at order 7, 18 at order 9: what a 16-drone tile's
 *            stash (one more matrix and one more vector per knot than the boundary-state solve) leaves of 160 KiB of
 *            LDS -- and at most max_segments.  One segment is excluded.  MSNAP_ESEGMENTS outside, and nothing is written.
 *            msnap_solve_periodic_max_segments returns MSNAP_EORDER for any other order.
 * MSNAP_EINVAL: a null context, a null wp, t, coef, dur or status, negative n_drones.  n_drones == 0 is a no-op.  A
 * drone's outputs are bit-identical whatever its place in the batch, the batch size, and host versus device entry.  The
 * device version only launches (no synchronisation, no context buffer, so no capture rules).
 */
int msnap_solve_periodic(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                         double *coef, double *dur, int32_t *status);
int msnap_solve_periodic_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, double *coef, double *dur, int32_t *status);
int msnap_solve_periodic_max_segments(int order);   /* largest n_seg the entry takes; < 0: MSNAP_EORDER */

/* ---- near pairs: every pair of a swarm whose sampled distance is below a per-pair limit ----
 * msnap_formation_collide names one partner per drone; msnap_formation_near_pairs lists every close pair, e.g. the
 * pairs msnap_pair_clearance has to see.  pos [n_drones][n_samples][3] as the sampler writes it; speed [n_drones] or
 * NULL (zeros); pairs [max_pairs][2]; pair_dist [max_pairs] or NULL; n_found [1].
 *   distance  for i < j: d2_ij = min over the samples of fma(dz, dz, fma(dy, dy, dx * dx)) -- the expression and the
 *             minNum rule of msnap_formation_collide: a non-finite sample never wins, and a drone without a finite
 *             sample is in no pair;
 *   limit     lim_ij = (base + (speed[i] + speed[j]) * gap) * (1 + margin), every operation rounded once, in this
 *             order, none fused (what the same expression gives in NumPy or torch);
 *   kept      iff sqrt(d2_ij) < lim_ij: strict, so a NaN limit (a NaN speed) keeps nothing of that drone.
 * Output: the kept pairs as (i, j), i < j, in ascending lexicographic order; pair_dist[p] = sqrt(d2) of pair p;
 * *n_found = the number of kept pairs whether or not they fit.  Only the first max_pairs pairs of that order are
 * written and nothing at or beyond max_pairs (nor, when fewer are kept, at or beyond *n_found): a caller that
 * overflowed calls again with max_pairs >= *n_found and gets the same list.  max_pairs == 0 with pairs == NULL is a
 * pure count.  The list, its order and pair_dist are bit-identical from run to run, host versus device entry and for
 * any max_pairs (no atomic decides a position).  n_drones 0 or 1: *n_found = 0, nothing else is touched.
 * MSNAP_EINVAL: a null context, pos or n_found; negative sizes; n_samples < 1; max_pairs < 0; pairs == NULL with
 * max_pairs > 0; base, gap or margin NaN; n_drones > 16384, the largest swarm the formation pipeline is sized for.
 * The device version only launches (n_found is a device long long[1]); its scratch is a buffer of the context under
 * the capture rules above (MSNAP_ECAPTURE: run the call once outside the capture first).
 * (Method: the pairwise pass's register tiling over the upper triangle writes keep bits, one byte per 8 columns and
 * row, each with one writer; popcount per row and a scan give every row its list offset; a wave per row emits.)
 */
int msnap_formation_near_pairs(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, double base,
                               const double *speed, double gap, double margin, long long max_pairs, int32_t *pairs,
                               double *pair_dist, long long *n_found);
int msnap_formation_near_pairs_device(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, double base,
                                      const double *speed, double gap, double margin, long long max_pairs,
                                      int32_t *pairs, double *pair_dist, long long *n_found);

/* ---- time allocation: segment times optimised per drone (new capability) ----
 * Everything above takes the waypoint times as given (the reference's grid t_i = i*10/n,
 * scripts/drones_pols_generator.py:44-46,56).  msnap_optimize_times moves the interior knot times of each drone,
 * independently, to lower its cost with the waypoints and the total duration kept.
 *
 * Per drone: wp [n_seg+1][4], t [n_seg+1] absolute with t[0] == 0 (t may be one grid shared by the batch:
 * shared_times != 0), weights[4] >= 0 for x, y, z, yaw (a HOST array in both versions), min_fraction in (0, 1],
 * max_iter >= 0, tol >= 0.  With M = n_seg and T_i the durations:
 *   objective   J(T) = sum_a weights[a] * J_a, J_a the msnap_snap_cost (crackle at order 9) of the solve for T;
 *   feasible    sum T_i = t[M] and T_i >= T_min = min_fraction * t[M] / M.  Input durations below T_min are raised to it
 *               and every other duration becomes T_min + (T_i - T_min) * f with the one factor
 *               f = 1 - (sum of the raises) / (sum of the other durations' excess over T_min), which keeps the sum;
 *               an input with no duration below T_min is taken bit for bit;
 *   t_out [M+1] t_out[0] = 0 and t_out[M] = t[M] bit for bit;  dur[i] = t_out[i+1] - t_out[i] as the solve entries form
 *               it, coef [M][4][order+1] the solution for t_out (the arithmetic of msnap_solve_batch's kernels);
 *   cost  [2]   J at the (raised) input times and at t_out;  pg [1] the stopping measure at t_out;
 *   iters [1]   accepted steps.  cost, pg, iters may be NULL.
 * Guarantees: every dur[i] >= T_min (1 - 1e-12);  cost[1] <= cost[0] (only decreasing steps are accepted: max_iter = 0
 * returns the input times and cost[1] == cost[0]);  the run ends when
 *               |P g|_2 * t[M] / (sqrt(M) * J) <= tol,
 * after max_iter accepted steps, or when the line search cannot lower J any more.  g_i = dJ/dT_i, and P removes the
 * mean over the free segments (a segment within T_min (1 + 1e-9) whose descent direction points below T_min is not
 * free).  The measure has no unit, and every quantity of the iteration scales by a power of two when the waypoints
 * do: t_out, dur, iters, pg are then bit-identical.  A drone's outputs are bit-identical whatever its position in the
 * batch, the batch size, or host versus device entry.
 * status [n_drones]: MSNAP_ST_NONFINITE for NaN / Inf in wp or t; MSNAP_ST_TIMES for times not strictly increasing or
 * t[0] != 0 (the solve entries evaluate segment 0's start rows at local time t[0], the reference's quirk; the gradient
 * below does not hold then); MSNAP_ST_SINGULAR for a non-positive pivot, or a cost that is not finite, at the input
 * times.  A failed drone gets NaN coef, t_out, dur, cost, pg and iters 0.  A trial point whose solve fails is a rejected
 * step, not a failed drone.
 * Method: projected gradient descent with Armijo backtracking, the whole iteration of the batch in one launch.
 * Direction -P g; first proposal 0.25 * min T / max |P g|; the step is the proposal cut so that no T_i passes T_min;
 * accepted when J_new <= J - 1e-4 * step * |P g|^2, after which the proposal is twice the step (the same proposal again
 * when the step had been cut); rejected otherwise, the proposal then half the step, at most 30 times in a row.  The
 * trial knots are the running sum of max(T_i + step * d_i, T_min) from 0, the last one t[M].
 * n_seg: 1 (returns the input) .. 80 at order 7, .. 58 at order 9 (what one tile's state leaves of the LDS), and at most
 * max_segments; MSNAP_ESEGMENTS above.  MSNAP_EINVAL: a weight that is negative or not finite, min_fraction outside
 * (0, 1], negative max_iter or tol.  The device version only launches (no synchronisation, no context buffer).
 *
 * msnap_snap_cost_grad: grad [n_drones][n_seg][4] = -E per segment and axis, E the Ostrogradsky energy of the
 * segment's polynomial at its start, with x^(q)(0) = q! c_q and k = (order + 1) / 2:
 *   E = (x^(k))^2 + 2 sum_{m=1..k-1} (-1)^m x^(k-m) x^(k+m)
 *     = 576 c4^2 - 1440 c3 c5 + 2880 c2 c6 - 10080 c1 c7                                              (order 7)
 *     = 14400 c5^2 - 34560 c4 c6 + 60480 c3 c7 - 161280 c2 c8 + 725760 c1 c9                          (order 9)
 * For a minimiser between fixed end states E is constant along the segment, and by the envelope theorem
 * dJ_a/dT_i = grad[.][i][a] -- but ONLY when coef is the solve's result for dur; for any other coefficients grad is
 * just this expression.  dur is not read (it names the point the derivative belongs to).
 */
int msnap_snap_cost_grad(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                         double *grad);
int msnap_snap_cost_grad_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                double *grad);
int msnap_optimize_times(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                         const double weights[4], double min_fraction, int max_iter, double tol, double *t_out,
                         double *coef, double *dur, int32_t *status, double *cost, double *pg, int32_t *iters);
int msnap_optimize_times_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, const double weights[4], double min_fraction, int max_iter,
                                double tol, double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                double *pg, int32_t *iters);

/* msnap_optimize_times_states: the same time allocation from and to given end states -- the step a replan in flight
 * lacks between msnap_eval_state and msnap_solve_states.  Arguments as msnap_optimize_times, with start and end after
 * shared_times in msnap_solve_states's layout: [n_drones][4][K-1], K = (order + 1) / 2, entry q-1 the q-th time
 * derivative at the first / last waypoint.  Either may be NULL: rest.  Objective, feasible set, floor (T_min =
 * min_fraction * t[M] / M, inputs below it raised as above), direction, step rules, stopping measure, cost / pg /
 * iters and the method are msnap_optimize_times's, word for word, with "the solve for T" read as msnap_solve_states's:
 * dJ/dT_i = -sum_a weights[a] E_i,a holds for the first and last segment too, whose outer end states are data instead
 * of stationary unknowns.
 *   kept        the waypoints, both end states, t_out[0] == 0 and t_out[M] == t[M] bit for bit.  The total duration is
 *               an input; it is not optimised (stretching a path changes no given end state, but choosing t[M] against
 *               dynamic limits is not this entry's job);
 *   coef, dur   the boundary-state solution for t_out: dur[i] = t_out[i+1] - t_out[i] bit for bit, coef what
 *               msnap_solve_states returns for t_out to rounding (norm-relative 1e-9); coef[0][a][0] is wp[0][a] bit for
 *               bit;
 *   end state   as msnap_solve_states states it: msnap_eval_state returns the given start derivatives at tq = 0 within
 *               4 * 2^-52 relative, and the given end derivatives at the sum of dur (as msnap_eval_flat accumulates it)
 *               within 4 * 2^-52 of max(|value|, sum_j |d_j| T^j).  The last segment takes the same refinement step on
 *               its end conditions, once, when the coefficients leave; cost, pg and the iteration's decisions are taken
 *               from the unrefined coefficients (the refinement moves them by units in the last place);
 *   status      MSNAP_ST_NONFINITE for NaN / Inf in wp, t or a state entry of that drone; MSNAP_ST_TIMES for times not
 *               strictly increasing or t[0] != 0; MSNAP_ST_SINGULAR for a non-positive pivot or a cost that is not
 *               finite at the (raised) input times.  A failed drone gets NaN coef, t_out, dur, cost, pg and iters 0; a
 *               trial point whose solve fails is a rejected step.
 * Guarantees as above: every dur[i] >= T_min (1 - 1e-12), cost[1] <= cost[0], max_iter = 0 returns the (raised) input
 * times.  A drone's outputs are bit-identical whatever its place in the batch, the batch size, or host versus device
 * entry; NULL and an array of zeros give the same bits.  With both blocks zero the problem is msnap_optimize_times's, and
 * the two agree to rounding (not bit for bit: this entry applies the last knot's coupling block to a zero end state).
 * n_seg: 1 (one Hermite segment, nothing to optimise: iters 0, t_out the input) ..
 * msnap_optimize_times_states_max_segments(order) -- 79 at order 7, 57 at order 9: what an 8-drone tile's state and its
 * two state images leave of 160 KiB of LDS -- and at most max_segments; MSNAP_ESEGMENTS above.  The query returns
 * MSNAP_EORDER for any other order.  MSNAP_EINVAL as msnap_optimize_times; n_drones == 0 is a no-op.  The device
 * version only launches (no synchronisation, no context buffer: the capture rules are msnap_optimize_times_device's).
 */
int msnap_optimize_times_states(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, const double *start /* [n_drones][4][K-1] or NULL */,
                                const double *end /* [n_drones][4][K-1] or NULL */, const double weights[4],
                                double min_fraction, int max_iter, double tol, double *t_out, double *coef, double *dur,
                                int32_t *status, double *cost, double *pg, int32_t *iters);
int msnap_optimize_times_states_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                       int shared_times, const double *start, const double *end,
                                       const double weights[4], double min_fraction, int max_iter, double tol,
                                       double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                       double *pg, int32_t *iters);
int msnap_optimize_times_states_max_segments(int order);     /* largest n_seg the entry takes; < 0: MSNAP_EORDER */

/* msnap_optimize_times_periodic: the same time allocation on closed loops.  Arguments as
 * msnap_optimize_times; wp, t as msnap_solve_periodic takes them: wp[M] - wp[0] is the lap offset, t[M] the period.
 * Objective, feasible set, floor (T_min = min_fraction * t[M] / M, inputs below it raised as above), direction, step
 * rules, stopping measure, cost / pg / iters, the power-of-two scaling property and the method are
 * msnap_optimize_times's, word for word, with "the solve for T" read as msnap_solve_periodic's: dJ/dT_i =
 * -sum_a weights[a] E_i,a holds on the ring, the seam state being a stationary unknown like every interior knot.
 *   kept        the waypoints, t_out[0] == 0 and t_out[M] == t[M] -- the period -- bit for bit;
 *   coef, dur   the periodic solution for t_out: dur[i] = t_out[i+1] - t_out[i] bit for bit, coef what
 *               msnap_solve_periodic returns for t_out to rounding (norm-relative 1e-9); coef[i][a][0] is wp[i][a] bit
 *               for bit;
 *   seam        as msnap_solve_periodic promises it: msnap_eval_state at the sum of dur returns derivatives 1 .. K-1
 *               equal to those at 0, and the position wp[M], within 4 * 2^-52 of the evaluation scale.  The
 *               coefficients that leave take msnap_solve_periodic's refinement step and the step on the last
 *               segment's end conditions, once; the trials run unrefined, and cost, pg and the iteration's decisions
 *               are taken from the unrefined coefficients, as in msnap_optimize_times_states;
 *   status      MSNAP_ST_NONFINITE for NaN / Inf in wp or t; MSNAP_ST_TIMES for times not strictly increasing or
 *               t[0] != 0; MSNAP_ST_SINGULAR for a non-positive pivot, the seam block's included, or a cost that is not
 *               finite at the (raised) input times.  A failed drone gets NaN coef, t_out, dur, cost, pg and iters 0; a
 *               trial point whose solve fails is a rejected step.
 * Guarantees as above: every dur[i] >= T_min (1 - 1e-12), cost[1] <= cost[0], max_iter = 0 returns the (raised) input
 * times.  A drone's outputs are bit-identical whatever its place in the batch, the batch size, or host versus device
 * entry.  Where the loop is cut changes the result by rounding only.
 * n_seg: 2 .. msnap_optimize_times_periodic_max_segments(order) -- 48 at order 7, 33 at order 9: what an 8-drone
 * tile's state leaves of 160 KiB of LDS (16-drone tiles up to 24 and 17 segments); every loop msnap_solve_periodic
 * takes (27, 18) can be allocated -- and at most max_segments; MSNAP_ESEGMENTS otherwise, nothing written.  The query
 * returns MSNAP_EORDER for any other order.  MSNAP_EINVAL as msnap_optimize_times; n_drones == 0 is a no-op.  The device
 * version only launches (no synchronisation, no context buffer: the capture rules are msnap_optimize_times_device's).
 */
int msnap_optimize_times_periodic(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                  int shared_times, const double weights[4], double min_fraction, int max_iter,
                                  double tol, double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                  double *pg, int32_t *iters);
int msnap_optimize_times_periodic_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                         int shared_times, const double weights[4], double min_fraction, int max_iter,
                                         double tol, double *t_out, double *coef, double *dur, int32_t *status,
                                         double *cost, double *pg, int32_t *iters);
int msnap_optimize_times_periodic_max_segments(int order);   /* largest n_seg the entry takes; < 0: MSNAP_EORDER */

/* msnap_optimize_times_free: time allocation from and to given end states with the total duration free (DESIGN.md §5
 * K17) -- what a replan in flight needs, whose start state is in physical units so that no uniform stretch
 * (msnap_retime_to_limits) can follow.  Arguments as msnap_optimize_times_states with time_weight [n_drones] after
 * weights: k_T > 0 per drone, the price of a second in units of the cost (a HOST array in the host version, a DEVICE
 * array in the device version; weights stays a host array in both).  With M = n_seg and T_i the durations:
 *   objective   F(T) = sum_a weights[a] * J_a(T) + k_T * sum_i T_i over ALL T_i, J_a as in msnap_optimize_times with
 *               "the solve for T" read as msnap_solve_states's.  dJ/dT_i = -sum_a weights[a] E_i,a is the derivative of
 *               segment i's cost at fixed end states and never asked for a fixed sum, so
 *               g_i = dF/dT_i = k_T - sum_a weights[a] E_i,a comes out of the same solve and nothing is projected;
 *   feasible    T_i >= T_min = min_fraction * t[M] / M, taken from the INPUT total.  Input durations below T_min are
 *               raised to it; every other input duration is taken bit for bit (no factor pays for the raise: the sum
 *               grows), and an input with no duration below T_min is taken bit for bit, knots included;
 *   t_out [M+1] t_out[0] = 0; t_out[M], the total, is an output.  t[M] is a starting guess;
 *   coef, dur   the msnap_solve_states solution for t_out: dur[i] = t_out[i+1] - t_out[i] bit for bit, coef what
 *               msnap_solve_states returns for t_out to rounding (norm-relative 1e-9), coef[0][a][0] is wp[0][a] bit for
 *               bit; the end states through msnap_eval_state as msnap_optimize_times_states promises them (the same
 *               refinement step on the last segment, once, when the coefficients leave);
 *   cost  [2]   F at the (raised) input times and at t_out;  pg [1] the stopping measure at t_out;  iters [1] accepted
 *               steps.  cost, pg, iters may be NULL;
 *   status      as msnap_optimize_times_states; a time_weight that is NaN, Inf or not > 0 gives that drone
 *               MSNAP_ST_NONFINITE and NaN outputs (at 0 the optimum is at infinity).
 * Method: gradient descent with Armijo backtracking, one launch.  Direction d_i = -g_i, and 0 on a segment within
 * T_min (1 + 1e-9) with g_i > 0: no mean is removed and no free set iterated, one pass.  The step rules are
 * msnap_optimize_times's word for word with J read as F and |P g| as |d|: first proposal 0.25 * min T / max |d|; the
 * step is the proposal cut so that no T_i passes T_min; accepted when F_new <= F - 1e-4 * step * |d|^2, after which the
 * proposal is twice the step (the same proposal again when the step had been cut); rejected otherwise, the proposal
 * then half the step, at most 30 times in a row.  The trial knots are the running sum of max(T_i + step * d_i, T_min)
 * from 0, the last knot included.  The run ends when
 *               |d|_2 * T_cur / (sqrt(M) * F) <= tol,          T_cur the current total,
 * after max_iter accepted steps, or when the line search cannot lower F any more.
 * Guarantees: every dur[i] >= T_min (1 - 1e-12);  cost[1] <= cost[0];  t_out[M] <= cost[0] / time_weight (F only
 * decreases and J >= 0);  max_iter = 0 returns the (raised) input times.  A drone's outputs are bit-identical whatever
 * its place in the batch, the batch size, or host versus device entry; NULL and an array of zeros give the same bits.
 * With both state blocks zero and no segment at the floor J is homogeneous of degree -(2k - 1) in the durations,
 * k = (order + 1) / 2, so sum_i T_i g_i = k_T T - (2k - 1) J (Euler), and since |sum_i T_i g_i| <= |g|_2 T the
 * stopping measure gives at a converged return |(2k - 1) J - k_T t_out[M]| <= tol * sqrt(M) * F; the ratios
 * dur / t_out[M] are then those msnap_optimize_times finds on the same waypoints, to the tolerance.
 * n_seg: 1 -- one duration between two given states, a real problem here: it iterates -- ..
 * msnap_optimize_times_free_max_segments(order) = 79 at order 7, 57 at order 9 (the LDS of msnap_optimize_times_states;
 * 16-drone tiles up to 39 and 28 segments), and at most max_segments; MSNAP_ESEGMENTS above.  The query returns
 * MSNAP_EORDER for any other order.  MSNAP_EINVAL as msnap_optimize_times_states, and for a NULL time_weight;
 * n_drones == 0 is a no-op.  The device version only launches (no synchronisation, no context buffer: the capture
 * rules are msnap_optimize_times_device's).
 */
int msnap_optimize_times_free(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                              int shared_times, const double *start /* [n_drones][4][K-1] or NULL */,
                              const double *end /* [n_drones][4][K-1] or NULL */, const double weights[4],
                              const double *time_weight /* [n_drones] */, double min_fraction, int max_iter, double tol,
                              double *t_out, double *coef, double *dur, int32_t *status, double *cost, double *pg,
                              int32_t *iters);
int msnap_optimize_times_free_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                     int shared_times, const double *start, const double *end,
                                     const double weights[4], const double *time_weight, double min_fraction,
                                     int max_iter, double tol, double *t_out, double *coef, double *dur,
                                     int32_t *status, double *cost, double *pg, int32_t *iters);
int msnap_optimize_times_free_max_segments(int order);       /* largest n_seg the entry takes; < 0: MSNAP_EORDER */

/* msnap_optimize_times_gates: time allocation through gates -- msnap_optimize_times_states on a path
 * whose interior waypoints may carry prescribed derivatives.  A path with gates is where a guessed time grid costs
 * most, and a uniform stretch (msnap_retime_to_limits) cannot mend it: it divides the prescribed velocities.
 * Arguments as msnap_optimize_times_states with fix and via after end, in msnap_solve_gates' layout and meaning:
 * fix [n_drones][n_seg-1] int32 masks (bit q-1: the q-th derivative at that interior waypoint is prescribed, on all four
 * axes), via [n_drones][n_seg-1][4][K-1] the values, K = (order + 1) / 2; an entry under a clear bit is never used and
 * may be NaN.  Objective, feasible set, floor, direction, step rules, stopping measure, cost / pg / iters and the method
 * are msnap_optimize_times's, word for word, with "the solve for T" read as msnap_solve_gates's: in Hermite form
 * J*(T) = min_u J(u, T), a gated component of u_i is data instead of a stationary unknown, which the envelope argument
 * does not look at, so dJ/dT_i = -sum_a weights[a] E_i,a holds as it does with given end states.
 *   kept        the waypoints, both end states, the gate values IN PHYSICAL UNITS (a velocity gate is met in m/s at
 *               whatever time its waypoint is crossed), t_out[0] == 0 and t_out[M] == t[M] bit for bit;
 *   moves       the interior knot times, and with them every derivative no gate prescribes;
 *   coef, dur   dur[i] = t_out[i+1] - t_out[i] bit for bit; coef is what msnap_solve_gates returns for t_out (same fix,
 *               via, start, end), bit for bit, so the gates are honoured as that entry states: on the segment that
 *               leaves a gated waypoint coef[i][a][q] * q! is the prescribed value within 4 * 2^-52 relative, on the
 *               segment that arrives it is met as every interior waypoint's continuity is met; the end states through
 *               msnap_eval_state as msnap_optimize_times_states promises them (the same refinement step on the last
 *               segment, once, when the coefficients leave; cost, pg and the decisions use the unrefined ones);
 *   status      as msnap_optimize_times_states, and MSNAP_ST_NONFINITE for a NaN / Inf via entry under a set bit or a
 *               fix entry that is negative or >= 2^(K-1): seen by the solve at the input times, before any step.  A
 *               failed drone gets NaN coef, t_out, dur, cost, pg and iters 0, and disturbs no other drone.
 * fix == NULL: no gates, via may be NULL too -- every output is msnap_optimize_times_states', bit for bit; so is it with
 * a mask of zeros.  Guarantees as there: every dur[i] >= T_min (1 - 1e-12), cost[1] <= cost[0], max_iter = 0 returns the
 * (raised) input times; a drone's outputs are bit-identical whatever its place in the batch, the batch size, or host
 * versus device entry.  A waypoint with every bit set decouples its two sides; the times are still allocated over the
 * whole path, since the sum is shared.
 * n_seg: 1 .. msnap_optimize_times_gates_max_segments(order) = 79 at order 7, 57 at order 9 -- msnap_optimize_times_
 * states' range (16-drone tiles up to 39 and 28 segments): masks and values stay in global memory and take no LDS --
 * and at most max_segments; MSNAP_ESEGMENTS above.  Note that msnap_solve_gates itself ends at 47 / 32.  The query
 * returns MSNAP_EORDER for any other order.  MSNAP_EINVAL as msnap_optimize_times_states, and for fix given without
 * via; n_drones == 0 is a no-op.  The device version only launches (no synchronisation, no context buffer: the capture
 * rules are msnap_optimize_times_device's).  Not built: a free total duration through gates, gates on closed loops,
 * per-axis masks.
 */
int msnap_optimize_times_gates(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                               int shared_times, const double *start /* [n_drones][4][K-1] or NULL */,
                               const double *end /* [n_drones][4][K-1] or NULL */,
                               const int32_t *fix /* [n_drones][n_seg-1] or NULL */,
                               const double *via /* [n_drones][n_seg-1][4][K-1] or NULL */, const double weights[4],
                               double min_fraction, int max_iter, double tol, double *t_out, double *coef, double *dur,
                               int32_t *status, double *cost, double *pg, int32_t *iters);
int msnap_optimize_times_gates_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                      int shared_times, const double *start, const double *end, const int32_t *fix,
                                      const double *via, const double weights[4], double min_fraction, int max_iter,
                                      double tol, double *t_out, double *coef, double *dur, int32_t *status,
                                      double *cost, double *pg, int32_t *iters);
int msnap_optimize_times_gates_max_segments(int order);      /* largest n_seg the entry takes; < 0: MSNAP_EORDER */

/* ---- drone-vs-drone formation pass (new capability; no reference) -------
 * rows: the n_rows drones this caller owns (a shard), starting at global index
 * row_offset; cols: all n_cols drones (after the all-gather).  Spheres of `radius`.
 *   pos_rows [n_rows][n_samples][3], pos_cols [n_cols][n_samples][3]
 *   min_dist [n_rows]  min over other drones j != global row and samples of |p_i-p_j|, the squared
 *                      distance taken as fma(dz, dz, fma(dy, dy, dx*dx)) (differences rounded once,
 *                      two fused multiply-adds: one rounding less than the plain sum of squares
 *                      and 7 instead of 9 vector operations per pair and sample)
 *   partner  [n_rows]  lowest global j attaining it (-1 if none)
 *   hit      [n_rows]  min_dist < 2*radius
 * pos_rows must be the rows [row_offset, row_offset + n_rows) of pos_cols (the same samples):
 * pairs inside that range are evaluated once and credited to both drones.  The host-pointer entry
 * compares the two arrays and falls back to the one-sided evaluation when they differ; a device-pointer
 * caller whose rows are some other set of drones sets the option "collide_no_sym" first.
 * n_cols == 0 gives (+inf, -1, 0).
 * Non-finite samples never win a minimum (IEEE minNum): a drone whose samples are NaN -- the
 * output of a solve with status != 0 -- reports (+inf, -1, 0) and is invisible to the other
 * drones.  Check status[] of the solve before trusting a "no hit" (the Python pipeline,
 * swarm.formation_pass, refuses such drones).  The same holds for msnap_mesh_sweep.
 */
int msnap_formation_collide(msnap_ctx *ctx, int n_rows, int row_offset, int n_cols,
                            int n_samples, const double *pos_rows, const double *pos_cols,
                            double radius, double *min_dist, int32_t *partner,
                            int32_t *hit);
int msnap_formation_collide_device(msnap_ctx *ctx, int n_rows, int row_offset, int n_cols,
                                   int n_samples, const double *pos_rows,
                                   const double *pos_cols, double radius,
                                   double *min_dist, int32_t *partner, int32_t *hit);

/* The same pass for a caller whose positions come from this library's sampler: msnap_sample_collide_device writes,
 * next to the positions, what the pass over these drones would otherwise compute in a launch of its own -- into
 * pos_rows_t, msnap_collide_rows_t_doubles(n_rows, n_samples) doubles, whose content is the pair's private matter:
 *   - the rows' TRANSPOSED image [n_samples][3][P], P = n_rows rounded up to whole 128-row blocks (the pass reads its
 *     rows from it, 512 contiguous bytes per wave and load, and skips its own transposition pass), or
 *   - where the pass over the n_rows drones as a whole swarm runs behind the exact broad phase: every drone's path
 *     box and sort key (the sampler has the samples in LDS; the pass then starts with its sort, without a key launch).
 * The context remembers which of the two it last wrote and where, as a pair (positions buffer pos, hand-over buffer
 * pos_t): the pass reads the hand-over only when it is handed that same pair -- pos_rows (row image) or pos_cols (boxes
 * and keys) the sampler's pos -- for the same drone and sample counts.  A buffer that is not that hand-over, comes with
 * other positions or no longer fits the options in force is ignored, never misread: the pass computes its own image or
 * keys.  A caller who rewrites the positions in place, without the sampler, must sample again; that case cannot be
 * detected.  The read-only option "collide_last_handover" reports what the last pass read (0 nothing, 1 the row
 * image, 2 the boxes and keys).  Device pointers only: the pair exists to keep the formation pipeline (sampler ->
 * pairwise pass) on the GPU without the intermediate launch. */
size_t msnap_collide_rows_t_doubles(int n_rows, int n_samples);
/* 1 if msnap_formation_collide_t_device with these arguments reads the sampler's hand-over, 0 if not (paths shorter
 * than 6 samples take plain loops: the caller can then sample with msnap_sample and save the second output). */
int msnap_formation_collide_reads_rows_t(const msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples);
int msnap_sample_collide_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef,
                                const double *dur, double dt, int n_samples, double *pos, double *pos_t);
/* The shared-grid solve and the sampler as ONE launch, the reference's drones_pols_generator -> drones_traj_generator
 * step for a swarm on a common grid (scripts/drones_pols_generator.py:44-77 -> scripts/drones_traj_generator.py:28-46):
 * the same outputs, bit for bit, as msnap_solve_grid_device followed by msnap_sample_collide_device (pos_t != NULL) or
 * msnap_sample_device with 3 axes (pos_t == NULL) -- the coefficients stay in LDS between the fp64 MFMA product and
 * the Horner loops, which saves the dependent launch and the read-back.  Shapes outside the fused kernel's range
 * (more than 11 segments, where it stops paying; samples beyond its LDS image) run as those two launches; the option "no_grid_sample"
 * forces that (A/B timing).  n_samples == 0: the solve alone. */
int msnap_solve_grid_sample_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, double dt, int n_samples,
                                   double *coef, double *dur, int32_t *status, double *pos /* [n_drones][n_samples][3] */,
                                   double *pos_t /* NULL or msnap_collide_rows_t_doubles(n_drones, n_samples) doubles */);
int msnap_formation_collide_t_device(msnap_ctx *ctx, int n_rows, int row_offset, int n_cols,
                                     int n_samples, const double *pos_rows_t, const double *pos_rows,
                                     const double *pos_cols, double radius, double *min_dist,
                                     int32_t *partner, int32_t *hit);

/* ---- the same pass split over the ranks of a job: every unordered pair on exactly ONE rank --------
 * BASELINE.json north_star: "the drone batch shards across the 8 GPUs ... with an RCCL all-gather for the
 * inter-drone formation collision pass".  After the all-gather every rank holds pos_all [n_drones][n_samples][3].
 * The swarm's unordered pairs form one triangular line of (128-row block, column) units -- the line a single
 * msnap_formation_collide launch walks; part `part` of `n_parts` evaluates the part-th of n_parts equal contiguous
 * ranges of it, each pair once, and credits both drones.  part_out (msnap_formation_part_bytes(n_drones) bytes,
 * 8-byte aligned) receives, for EVERY drone of the swarm, the squared minimum over the pairs this part met
 * (double [n_drones]) followed by the partner (int32 [n_drones]; +inf / -1 where it met none).  The ranks exchange
 * their part_out blocks (one more all-gather of n_parts x 12 B x n_drones) and msnap_formation_collide_finish folds
 * them for the rows [row_offset, row_offset + n_rows) a rank owns: minimum over the parts (lowest partner wins a
 * tie), distance, hit -- bit for bit what one msnap_formation_collide over the whole swarm returns.
 *   parts [n_parts] blocks of msnap_formation_part_bytes(n_drones) bytes, part p at offset p * that
 */
size_t msnap_formation_part_bytes(int n_drones);
/* Who evaluates which pairs on several ranks is a choice between the parts above and "every rank runs the pass over
 * the whole gathered swarm behind the exact broad phase and keeps its rows" (one collective instead of two; pays when
 * the broad phase leaves few pairs).  Both inputs of that choice are the library's own and are exported here, so that
 * a host does not re-type launch thresholds or cost-model constants:
 *   msnap_formation_collide_takes_broad_phase  1 if msnap_formation_collide[_device] with these arguments would run
 *       behind the broad phase (size limits, "collide_no_cull", "collide_no_sym", "collide_cull_min_drones"), else 0;
 *   msnap_formation_whole_pass_pays  after a whole-swarm pass of n_drones on this context: *pays = 1 if, by the
 *       counts that pass left (pairs it evaluated: 8 x 8 per surviving group pair or 128 x 8 per surviving share,
 *       whichever list its evaluator walked) and the evaluator's cost model, the whole pass on every one of n_ranks
 *       ranks is quicker than a rank's 1 / n_ranks of all pairs plus the second collective; 0 if not, or if the last
 *       pass did not take the broad phase.  Synchronises the stream (MSNAP_ECAPTURE during a capture).
 * Read-only options of the same pass: "collide_last_by_groups" (1: its evaluator walked the group pairs) and
 * "collide_last_pairs_evaluated" (drone pairs it evaluated); both synchronise. */
int msnap_formation_collide_takes_broad_phase(const msnap_ctx *ctx, int n_rows, int row_offset, int n_cols,
                                              int n_samples);
int msnap_formation_whole_pass_pays(msnap_ctx *ctx, int n_drones, int n_ranks, int *pays);
int msnap_formation_collide_part(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos_all,
                                 int part, int n_parts, void *part_out);
int msnap_formation_collide_part_device(msnap_ctx *ctx, int n_drones, int n_samples,
                                        const double *pos_all, int part, int n_parts, void *part_out);
int msnap_formation_collide_finish(msnap_ctx *ctx, int n_drones, int n_parts, const void *parts,
                                   int row_offset, int n_rows, double radius, double *min_dist,
                                   int32_t *partner, int32_t *hit);
int msnap_formation_collide_finish_device(msnap_ctx *ctx, int n_drones, int n_parts, const void *parts,
                                          int row_offset, int n_rows, double radius, double *min_dist,
                                          int32_t *partner, int32_t *hit);

/* ---- drone-vs-mesh sweep against resources/stl obstacles (new capability) ----------
 *   tris [n_tris][3][3] fp64 vertices (binary STL float32 widened by the caller)
 *   min_dist [n_drones] min over samples and triangles of the point-triangle distance
 *   hit      [n_drones] min_dist < radius
 */
int msnap_mesh_sweep(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos,
                     int n_tris, const double *tris, double radius, double *min_dist,
                     int32_t *hit);
int msnap_mesh_sweep_device(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos,
                            int n_tris, const double *tris, double radius,
                            double *min_dist, int32_t *hit);

/* ---- rigid-body state validity, batched (the planner's OMPL validity callback) -------
 * replaces isStateValid, src/RigidBodyPlanners/RB_planning_sep_coll_check.py:208-226
 * (robot mesh at (x,y,z) with quaternion_from_euler(0,0,yaw), fcl.collide against the
 * environment mesh, src/RigidBodyPlanners/fcl_checker.py:93-100) for many states at once.
 *   states [n_states][4]  x, y, z, yaw
 *   rtris  [n_rtris][3][3] robot mesh (body frame), etris [n_etris][3][3] environment mesh
 *   valid  [n_states]  1 = no robot triangle intersects an environment triangle
 */
int msnap_mesh_validity(msnap_ctx *ctx, int n_states, const double *states, int n_rtris,
                        const double *rtris, int n_etris, const double *etris, int32_t *valid);
int msnap_mesh_validity_device(msnap_ctx *ctx, int n_states, const double *states, int n_rtris,
                               const double *rtris, int n_etris, const double *etris,
                               int32_t *valid);

#ifdef __cplusplus
}
#endif
#endif /* MSNAP_H */
