// Internal declarations shared by the translation units of libmsnap.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/msnap.h"
#include "msnap_solve_plan.h"   // kWave, kDronesPerWave, kMaxLdsBytes and the K1 solve's sizes

#define MSNAP_VERSION_NUM 500  /* 0.5.0: pairwise clearance in continuous time (msnap_clearance.hip) */

namespace msnap {

constexpr int kAxes = 4;                // x, y, z, yaw: one lane each

// s_waitcnt vmcnt(N): returns once all but the N most recent vector-memory operations of the wave have
// completed (loads and stores share the counter on gfx950 and retire in order).  For hand-issued asm
// prefetch loads followed by AT LEAST N stores; the immediate is a compile-time constant (a run-time
// choice between immediates compiles into a flag dispatch with a static path around every wait, which
// tools/check_prefetch_isa.py could not tell from a missing wait).
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "6-bit vmcnt field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// A workgroup barrier that orders LDS only.  __syncthreads() is a release / acquire fence pair around s_barrier, and the
// release waits for every global store the wave has in flight (s_waitcnt vmcnt(0)): a kernel that has just issued
// stores would sit out their round trip at the next barrier although nothing in the workgroup reads them back.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// growable device buffer
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  bool in_graph = false;   // a stream capture has used this block: a graph may hold pointers into it (ensure())
};
// a block a graph may still replay on, replaced by a larger one: freed by msnap_release_graph_buffers / msnap_destroy
struct RetiredBuf {
  void *p;
  size_t cap;
  RetiredBuf *next;
};

}  // namespace msnap

struct msnap_ctx {
  int device = 0;
  int order = 7;
  int khalf = 4;           // (order+1)/2
  int max_segments = 0;
  int n_cu = 256;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  msnap::DevBuf scratch;   // global-memory scratch for n_seg too large for LDS
  msnap::DevBuf host_stage;    // the host-pointer entry points' staging arena (msnap_api.hip, staged()); also the device
                               // side of solve_host's bounce buffer and its shared time grid when chunked
  msnap::DevBuf collide_work;  // the pairwise pass's working set (msnap_collide.hip, launch_formation_collide[_part])
  msnap::DevBuf limits_work;   // msnap_limits.hip: per-(drone, segment, quantity) peaks, then the retiming's per-drone peaks
  msnap::DevBuf extent_work;   // msnap_extent.hip: per-(drone, direction, segment) results, then the per-(drone, segment) flags
  msnap::DevBuf clearance_work;   // msnap_clearance.hip (pairwise and cross): per-(pair, slot) results, then the per-(drone, segment) flags of each set
  msnap::DevBuf mesh_clearance_work;   // msnap_mesh_clearance.hip: per-(drone, segment) results, then the per-(drone, segment) flags
  msnap::DevBuf pairs_work;       // msnap_pairs.hip: the row image, the keep-bit matrix, the rows' counts and list offsets
  // chunked host-pointer solves: two streams alternate H2D -> kernel -> D2H over chunks of drones,
  // each with its own staging set (wp, t, coef, dur, status)
  hipStream_t pipe_stream[2] = {nullptr, nullptr};
  hipEvent_t pipe_start = nullptr;
  msnap::DevBuf pipe[2][5];
  size_t pipe_chunk_bytes = 64u << 20;   // output bytes per chunk (MSNAP_PIPE_CHUNK_MB overrides)
  // small host-pointer solves: one page-locked bounce buffer, one upload and one download per call
  void *bounce = nullptr;
  size_t bounce_cap = 0;
  // shared-time-grid operator (K2): built by msnap_grid_prepare
  msnap::DevBuf grid_t, grid_wp, grid_op, grid_dur, grid_status, grid_frag;
  int grid_seg = 0;
  int grid_ready = 0;
  // launch-geometry options (msnap_set_option; the MSNAP_* environment variables of msnap.h only
  // seed them in msnap_create -- nothing on a launch path reads the environment)
  int no_twist = 0;             // "no_twist": keep small batches on the one-sided kernels (A/B timing)
  int gemm_stream_waves_per_cu = 0;   // "gemm_stream_waves_per_cu": wave target of the streaming GEMM's column slicing (0: default)
  int no_grid_sample = 0;      // "no_grid_sample": msnap_solve_grid_sample runs the two kernels (A/B timing)
  int no_twin = 0;             // "no_twin": batches keep solve_kernel_reg where solve_kernel_twin would run (A/B timing)
  int twin_max_drones = 0;      // "twin_max_drones": largest batch that takes solve_kernel_twin (0: default per order)
  int twist_max_drones = 0;     // "twist_max_drones": batches up to this size take the small-batch kernel (0: default)
  int twist_waves = 0;          // "twist_waves": waves per 8-drone tile of the small-batch kernel: 1, 2, 4 (0: chosen per launch)
  int solve_grid_waves = 0;     // "solve_grid_waves": cap on solve_kernel_reg's persistent grid (0: default)
  int gemm_grid_waves = 0;      // "gemm_grid_waves": cap on the shared-grid GEMM's persistent grid (0: default)
  void *mesh_tests = nullptr;   // "mesh_count_tests": device counter of the point-triangle tests evaluated (not culled)
  int collide_waves_per_cu = 0; // "collide_waves_per_cu": shares per CU of the pairwise pass (0: one column block per share)
  int collide_sample_parts = 0; // "collide_sample_parts": waves per share of the pairwise pass (0: chosen per launch)
  int collide_no_sym = 0;       // "collide_no_sym": 1 = the rows of msnap_formation_collide[_device] are NOT the slice of the columns at row_offset: one-sided evaluation
  int collide_no_cull = 0;      // "collide_no_cull": 1 = whole-swarm passes without the exact broad phase (A/B, dense swarms)
  int collide_cull_mode = 0;         // "collide_cull_mode": evaluator behind the broad phase: 0 chosen per pass, 1 surviving shares, 2 surviving group pairs
  int collide_cull_min_drones = 0;   // "collide_cull_min_drones": smallest whole swarm that takes the broad phase (0: default 3072)
  int collide_last_cull = 0;    // "collide_last_cull" (read): 1 if the last msnap_formation_collide took the broad-phase path
  int collide_last_shares = 0;  // "collide_last_shares" (read): 8-column x 128-row shares of that pass before the broad phase
  const int32_t *collide_meta = nullptr;   // device: its survivor counts ("collide_last_survivors" / "_group_pairs", read: synchronise)
  int collide_last_by_groups = 0;   // "collide_last_by_groups" (read): that pass's evaluator walked the surviving group pairs
  int collide_last_n = 0;           // its swarm size
  const void *blist_clean = nullptr;   // the group evaluator's reverse lists at this address (for blist_clean_n groups) are all-zero
  int blist_clean_n = 0;
  // one 64-bit word in page-locked host memory the broad phase's evaluator writes its survivor counts to: the next
  // pass's choice of evaluator reads it without synchronising (csrc/msnap_collide.hip::cull_hint_pack)
  unsigned long long *cull_hint = nullptr;
  // what msnap_sample_collide_device left for the pairwise pass, and where (the last few buffers it wrote): 1 the
  // transposed row image, 2 the per-drone boxes and sort keys of a whole-swarm pass behind the broad phase, each with
  // the positions buffer the sampler wrote beside it.  A buffer the pass is handed that is not on record -- or whose
  // record does not fit the pass, positions included -- is ignored, never misread.
  struct Handover {
    const void *ptr = nullptr;
    const void *pos = nullptr;
    int n = 0, s = 0, form = 0;
  } handover[8];
  int handover_next = 0;
  int collide_last_sym = 0;     // "collide_last_sym" (read): 1 if the last msnap_formation_collide evaluated its own-range pairs once
  int collide_last_handover = 0;   // "collide_last_handover" (read): the sampler's hand-over that pass read (0 none, 1 row image, 2 boxes and keys)
  int mesh_waves_per_cu = 0;    // "mesh_waves_per_cu": wavefronts per CU the mesh sweep's grid is capped at (0: one workgroup per drone)
  int own_stream_priority = 0;  // "own_stream_priority": 0 default, 1 lowest, 2 highest (re-creates own_stream)
  msnap::RetiredBuf *retired = nullptr;   // blocks kept alive for graphs captured before they were outgrown
  int timeopt_ready = 0;        // msnap_timeopt_kernel.h: bit m set when mode m's kernels' dynamic-LDS limit has been raised on this context's device
  char hip_err[256] = {0};
  char last_kernel[96] = {0};   // msnap_last_kernel: the solve kernel instance the last solve entry point launched
};

namespace msnap {

int record_hip_error(msnap_ctx *ctx, hipError_t e, const char *what);
int ensure(msnap_ctx *ctx, DevBuf &b, size_t bytes);
bool stream_is_capturing(const msnap_ctx *ctx);
// form (1 row image, 2 boxes and keys; 0: not on record for these positions, n drones x n_samples) of a sampler
// hand-over buffer
int handover_form(const msnap_ctx *ctx, const void *ptr, const void *pos, int n, int n_samples);

// records the kernel instance a solve launcher chose (msnap_last_kernel; bench.py labels its rooflines with it)
void note_kernel(msnap_ctx *ctx, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// blocks of `threads` that cover `items`
inline unsigned blocks_of(size_t items, int threads) { return (unsigned)((items + threads - 1) / threads); }

#define MSNAP_HIP(ctx, call)                                         \
  do {                                                               \
    hipError_t e__ = (call);                                         \
    if (e__ != hipSuccess) return msnap::record_hip_error(ctx, e__, #call); \
  } while (0)

// kernel launchers (device pointers, asynchronous on ctx->stream)
int launch_solve(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                 int shared_times, double *coef, double *dur, int32_t *status);
int launch_pack(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                float *out);
int launch_formation_transform(msnap_ctx *ctx, int n_poses, int n_offsets, const double *rb_pose,
                               const double *offsets, double *out);
int launch_sample(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                  double dt, int n_samples, int n_axes, double *pos, double *pos_t, bool keys_form);
int launch_eval_flat(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                     int n_samples, const double *ts, double *out);
int launch_snap_cost(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, double *cost);
int launch_snap_cost_grad(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, double *grad);
// time allocation (msnap_timeopt.hip): the whole iteration of a batch in one launch.  The modes: rest to rest
// (msnap_optimize_times), from and to given end states (_states), closed loop, the trial being the periodic solve
// (_periodic), end states with the total duration free (_free), end states with prescribed derivatives at interior
// waypoints (_gates).
enum TimeoptMode : int { kTimeoptRest = 0, kTimeoptEnds = 1, kTimeoptRing = 2, kTimeoptFree = 3, kTimeoptGates = 4 };
// One allocation call, in the order of msnap_optimize_times_free's parameters, the gates behind them.  Every mode reads
// all fields but these: start / end ([n_drones][4][K-1], or null for rest) are read with kTimeoptEnds, kTimeoptFree and
// kTimeoptGates only, time_weight ([n_drones], required) with kTimeoptFree only, fix / via ([n_drones][n_seg-1] masks
// and [..][4][K-1] values, fix null: no gates) with kTimeoptGates only; an entry whose mode has none leaves them null.
// cost, pg, iters may be null in every mode.  weights is a host array of 4; every other pointer is the host's in a host entry and the device's
// from launch_optimize_times on.
struct TimeoptCall {
  int n_drones, n_seg;
  const double *wp, *t;
  int shared_times;
  const double *start, *end, *weights, *time_weight;
  double min_fraction;
  int max_iter;
  double tol;
  double *t_out, *coef, *dur;
  int32_t *status;
  double *cost, *pg;
  int32_t *iters;
  const int32_t *fix = nullptr;
  const double *via = nullptr;
};
// the one launch other code calls, asynchronous on ctx->stream
int launch_optimize_times(msnap_ctx *ctx, int mode, const TimeoptCall &call);
// (what it calls for the modes whose instances are objects of their own: msnap_timeopt_periodic.hip,
// msnap_timeopt_free.hip, msnap_timeopt_gates.hip)
int launch_optimize_times_ring(msnap_ctx *ctx, const TimeoptCall &call);
int launch_optimize_times_free(msnap_ctx *ctx, const TimeoptCall &call);
int launch_optimize_times_gates(msnap_ctx *ctx, const TimeoptCall &call);
// largest n_seg whose per-tile state fits LDS (80 at order 7, 58 at order 9; kTimeoptEnds and kTimeoptGates: see
// DESIGN.md K8; kTimeoptRing: 48, 33)
int timeopt_max_segments(int khalf, int mode);
// The tile solves beside K1 (entries: msnap_states.hip): from and to given end states (msnap_solve_states), with
// prescribed derivatives at interior knots as well (msnap_solve_gates), closed loop (msnap_solve_periodic).
enum SolveMode : int { kSolveEnds = 0, kSolveGates = 1, kSolveRing = 2 };
// One such call, in the order of msnap_solve_gates' parameters.  start / end ([n_drones][4][K-1], or null for rest) are
// read with kSolveEnds and kSolveGates, fix / via ([n_drones][n_seg-1] masks and [..][4][K-1] values, fix null: no
// gates) with kSolveGates; an entry whose mode has none leaves them null.  The pointers are the host's in a host entry
// and the device's from the launchers on.
struct SolveCall {
  int n_drones, n_seg;
  const double *wp, *t;
  int shared_times;
  const double *start, *end;
  const int32_t *fix;
  const double *via;
  double *coef, *dur;
  int32_t *status;
};
// each mode's kernels and launcher stay in their unit (msnap_states.hip, msnap_gates.hip, msnap_periodic.hip)
int launch_solve_states(msnap_ctx *ctx, const SolveCall &call);
int launch_solve_gates(msnap_ctx *ctx, const SolveCall &call);
int launch_solve_periodic(msnap_ctx *ctx, const SolveCall &call);
// the closed loop's cap from its own LDS layout (27 at order 7, 18 at order 9)
int periodic_max_segments(int khalf);
// (the pairwise pass: msnap_collide.h)
int launch_mesh_sweep(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, int n_tris,
                      const double *tris, double radius, double *min_dist, int32_t *hit);
int launch_mesh_validity(msnap_ctx *ctx, int n_states, const double *states, int n_rtris, const double *rtris,
                         int n_etris, const double *etris, int32_t *valid);
int solve_kernel_setup(msnap_ctx *ctx);
// true when launch_solve would use the context's single global scratch slab (very long paths):
// such launches must not overlap each other
bool solve_uses_global_scratch(const msnap_ctx *ctx, int n_seg);
int launch_grid_prepare(msnap_ctx *ctx, int n_seg, const double *t, int t_on_device);
int launch_solve_grid(msnap_ctx *ctx, int n_drones, const double *wp, double *coef, double *dur,
                      int32_t *status);
bool grid_gemm_supported(const msnap_ctx *ctx, int n_seg);
// k-step pitch of the packed operator fragments ([column tile][pitch][64]); 0: no GEMM operator for this grid
int grid_frag_ks_pitch(const msnap_ctx *ctx, int n_seg);
int launch_grid_sample(msnap_ctx *ctx, int n_drones, const double *wp, double dt, int n_samples, double *coef,
                       double *dur, int32_t *status, double *pos, double *pos_t, bool keys_form);

// dynamic limits (msnap_limits.hip): one lane per (drone, segment, quantity), kLimitsThreads lanes per block
constexpr int kLimitsThreads = 256;
inline int check_limits_args(const msnap_ctx *ctx, int n_drones, int n_seg) {
  if (!ctx || n_drones < 0) return MSNAP_EINVAL;
  if (n_seg < 1 || n_seg > ctx->max_segments) return MSNAP_ESEGMENTS;
  if (((size_t)n_drones * n_seg * 4 + kLimitsThreads - 1) / kLimitsThreads > 0x7fffffffu) return MSNAP_EINVAL;   // grid size
  return MSNAP_OK;
}
inline int check_limits(const double *limits, int flags) {
  if (!limits || (flags & ~(MSNAP_RETIME_FIT | MSNAP_RETIME_COMMON))) return MSNAP_EINVAL;
  for (int q = 0; q < 4; ++q)
    if (!(limits[q] >= 0.0)) return MSNAP_EINVAL;      // negative or NaN
  return MSNAP_OK;
}
// ctx->limits_work: per-lane results [N M 4][2], then (retiming) peak [N][4], t_peak [N][4], status [N]
inline size_t lane_doubles(int N, int M) { return (size_t)N * M * 4 * 2; }
int launch_peaks(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, double *work, double *peak,
                 double *t_peak, int32_t *status);
int launch_time_scale(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, const double *scale,
                      double *coef_out, double *dur_out);
int launch_retime(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, const double *limits, int flags,
                  double *coef_out, double *dur_out, double *scale);

// pairwise and cross clearance (msnap_clearance.hip): one lane per (pair, slot), n_seg_a + n_seg_b - 1 slots per pair
// (pairwise: both are n_seg)
constexpr int kClearanceThreads = 256;
inline size_t clearance_lanes(int n_pairs, int Ma, int Mb) { return (size_t)n_pairs * (size_t)(Ma + Mb - 1); }
// ctx->clearance_work: per-lane results [lanes][3] doubles, then the flags [segs] int32 (pairwise: [N M]; cross: those
// of set A [n_a Ma], then of set B [n_b Mb])
inline size_t clearance_work_bytes(size_t lanes, size_t segs) {
  return lanes * 3 * sizeof(double) + segs * sizeof(int32_t);
}
// mesh clearance (msnap_mesh_clearance.hip): one lane per (drone, segment).  ctx->mesh_clearance_work: per-lane results
// [N M][3] doubles, then the flags [N M] int32
inline size_t mesh_clearance_work_bytes(int N, int M) {
  return (size_t)N * M * (3 * sizeof(double) + sizeof(int32_t));
}
// near pairs (msnap_pairs.hip).  ctx->pairs_work: the row image [n_samples][3][rows rounded up to whole blocks of 128]
// doubles, the keep bits [N][words] of 64-bit words, the rows' list offsets [N] long long, the rows' counts [N] int32
inline size_t near_pairs_words(int N) { return ((size_t)N + 63) / 64; }
inline size_t near_pairs_pitch(int N) { return ((size_t)N + 127) / 128 * 128; }
inline size_t near_pairs_work_bytes(int N, int S) {
  return near_pairs_pitch(N) * (size_t)S * 3 * sizeof(double) + (size_t)N * near_pairs_words(N) * 8 +
         (size_t)N * sizeof(long long) + (size_t)N * sizeof(int32_t);
}
// the grid of a launch with one thread per (drone, segment) (K9's and K11's flags, K11's lanes) fits a dim3
inline int check_walk_grid(int n_drones, int n_seg) {
  return ((size_t)n_drones * n_seg + kClearanceThreads - 1) / kClearanceThreads > 0x7fffffffu ? MSNAP_EINVAL : MSNAP_OK;
}
// path extent (msnap_extent.hip): one lane per (drone, segment, direction), one fold thread per (drone, direction).
// ctx->extent_work: per-lane results [N][K][M][3] doubles, then the flags [N M] int32
inline size_t extent_lanes(int N, int M, int K) { return (size_t)N * M * K; }
inline size_t extent_work_bytes(int N, int M, int K) {
  return extent_lanes(N, M, K) * 3 * sizeof(double) + (size_t)N * M * sizeof(int32_t);
}
inline int check_extent_grid(int n_drones, int n_seg, int n_dirs) {
  if ((extent_lanes(n_drones, n_seg, n_dirs) + kClearanceThreads - 1) / kClearanceThreads > 0x7fffffffu) return MSNAP_EINVAL;   // grid size
  return check_walk_grid(n_drones, n_seg);
}
int launch_path_extent(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int K, const double *dirs,
                       double *ext, double *t_ext, double *upper, int32_t *status);
// per set, and the lane grid of the two segment counts together (pairwise: the one set given twice)
inline int check_clearance_args(const msnap_ctx *ctx, int n_a, int n_seg_a, int n_b, int n_seg_b, int n_pairs) {
  if (!ctx || n_a < 0 || n_b < 0 || n_pairs < 0) return MSNAP_EINVAL;
  if (n_seg_a < 1 || n_seg_a > ctx->max_segments || n_seg_b < 1 || n_seg_b > ctx->max_segments) return MSNAP_ESEGMENTS;
  if ((clearance_lanes(n_pairs, n_seg_a, n_seg_b) + kClearanceThreads - 1) / kClearanceThreads > 0x7fffffffu) return MSNAP_EINVAL;   // grid size
  if (int rc = check_walk_grid(n_a, n_seg_a)) return rc;
  return check_walk_grid(n_b, n_seg_b);
}
}  // namespace msnap
