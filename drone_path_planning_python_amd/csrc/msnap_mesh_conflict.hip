// Conflict windows of a drone against a triangle mesh in continuous time: from when until when the path is closer to
// the mesh than a threshold (include/msnap.h, "mesh conflict windows").  The obstacle counterpart of
// K18 (msnap_conflict.hip): its time-ordered walk in both directions, with K11's distance, bound and lanes
// (msnap_mesh_bound.h, the text msnap_mesh_clearance.hip calls as well).
//
// Lane.  One per (drone, segment): the segment's x, y, z scaled to u in [0, 1].  The walk in both directions, the node
// rule and the lane's four numbers are msnap_window.h's (first_crossing, window_lane_tail): the bound is a distance,
// compared with the threshold; the attained values are squared distances, compared with threshold^2.  The node step here:
//   1. node_points: the control points, their box, the path's points at the node's start, middle and end;
//   2. the triangles in index order (wave-uniform: scalar loads).  One whose box lies threshold or more from the control
//      points' box (box_tri_lb2 >= threshold^2) is proven far on the node and left out -- the threshold is fixed, so
//      this needs no running best.  Of the others: the smallest support-plane bound (tri_node_bound) and the smallest
//      attained squared distance at each of the three points.
//
// Fold.  One thread per drone over its segments (msnap_window.h, fold_window); then the distance at t_first and at
// t_last -- msnap_eval_flat's lookup and Horner, every triangle in index order through the sweep's functions, strict
// `<` -- so that msnap_mesh_sweep of that one position returns d_first / d_last bit for bit and tri_first / tri_last
// is the lowest index that attains it.  Nothing crosses lanes but the trip count.
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_mesh_bound.h"
#include "msnap_wave.h"
#include "msnap_window.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;
// ctx->mesh_clearance_work: per-lane results [N M][4] doubles, then the flags [N M] int32
inline size_t mesh_conflict_work_bytes(int N, int M) {
  return (size_t)N * M * (kWindowLaneDoubles * sizeof(double) + sizeof(int32_t));
}

// one lane per (drone, segment): work[4 item ..] = the four times of the head, on the drone's clock
template <int NC>
__global__ void __launch_bounds__(kThreads)
mesh_conflict_lane_kernel(const double *__restrict__ coef, const double *__restrict__ dur,
                          const int32_t *__restrict__ flags, int N, int M, int n_tris, const double *__restrict__ tris,
                          double threshold, double t_res, double *__restrict__ work) {
  constexpr int D = NC - 1;       // degree of the positions
  const double inf = __builtin_inf();
  const size_t total = (size_t)N * M;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = item < total;
  const size_t d = in_range ? item / (size_t)M : 0;
  const int k = in_range ? (int)(item - d * (size_t)M) : 0;

  // one pass over the drone's durations: its flags, the lane's segment and where it starts (the running sums of
  // msnap_eval_flat); every lane makes M trips
  double acc = 0.0, start = 0.0, T = 1.0;
  int bad = 0;
  for (int i = 0; i < M; ++i) {
    const double Ti = in_range ? dur[d * M + i] : 1.0;
    bad |= in_range ? flags[d * M + i] : 0;
    if (i == k) { start = acc; T = Ti; }
    acc = acc + Ti;
  }
  const double E = start + T;
  const bool ok = in_range && bad == 0;

  // e[s][j]: axis s of the segment in u = t / T
  double e[3][D + 1];
  {
    const double *c = coef + (d * M + k) * 4 * NC;
    double hp = 1.0;
#pragma unroll
    for (int j = 0; j <= D; ++j) {
#pragma unroll
      for (int s = 0; s < 3; ++s) e[s][j] = ok ? c[s * NC + j] * hp : 0.0;
      hp *= T;
    }
  }

  const double L = threshold * threshold;
  // the node step: the smallest support-plane bound (a distance) and the smallest attained squared distances at the
  // node's three points, over the triangles that are not proven far on the node
  const auto values = [&](double a, double hh, bool active, double &bound, double (&g)[3]) {
    double b[3][D + 1], p[3][3], lo[3], hi[3];
    node_points<D>(e, a, hh, b, p, lo, hi);
    bound = g[0] = g[1] = g[2] = inf;
    for (int t = 0; t < n_tris; ++t) {
      const double *tri = tris + (size_t)t * 9;
      if (!tri_finite(tri)) continue;
      const bool need = active && !(box_tri_lb2(lo, hi, tri) >= L);      // not proven far on the node
      if (__ballot(need) == 0) continue;
      double d2[3];
      const double tb = tri_node_bound<D>(tri, b, p, d2);
      bound = need ? fmin(bound, tb) : bound;
#pragma unroll
      for (int q = 0; q < 3; ++q) g[q] = need ? fmin(g[q], d2[q]) : g[q];
    }
  };
  const auto walk = [&](double &hit, double &clear) { first_crossing(values, ok, T, threshold, L, t_res, hit, clear); };
  double out[kWindowLaneDoubles];
  window_lane_tail(e, ok, T, start, E, walk, out);

  if (!in_range) return;
#pragma unroll
  for (int q = 0; q < kWindowLaneDoubles; ++q) work[kWindowLaneDoubles * item + q] = out[q];
}

struct Outputs {
  double *t_clear_until, *t_first, *d_first;
  int32_t *tri_first;
  double *t_last, *d_last;
  int32_t *tri_last;
  double *t_clear_from;
  int32_t *status;
};

// one thread per drone: status, the fold of the segments, the distances through the sweep's functions
template <int NC>
__global__ void __launch_bounds__(kThreads)
mesh_conflict_fold_kernel(const double *__restrict__ coef, const double *__restrict__ dur,
                          const int32_t *__restrict__ flags, const double *__restrict__ work, int N, int M, int n_tris,
                          const double *__restrict__ tris, double *__restrict__ t_clear_until,
                          double *__restrict__ t_first, double *__restrict__ d_first, int32_t *__restrict__ tri_first,
                          double *__restrict__ t_last, double *__restrict__ d_last, int32_t *__restrict__ tri_last,
                          double *__restrict__ t_clear_from, int32_t *__restrict__ status) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= N) return;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  int bad = 0;
  for (int i = 0; i < M; ++i) bad |= flags[(size_t)d * M + i];
  const int st = status_of_flags(bad);
  double cu = nan, tf = nan, df = nan, tl = nan, dl = nan, cf = nan;
  int wf = -1, wl = -1;
  if (st == MSNAP_ST_OK) {
    cu = tf = inf;      // certified clear over the whole window
    tl = cf = -inf;
    fold_window(work + (size_t)d * M * kWindowLaneDoubles, M, cu, tf, tl, cf);
    df = dl = inf;
    if (tf < inf) {
#pragma unroll 1
      for (int q = 0; q < 2; ++q) {      // (one text of the evaluation for both ends)
        double x, y, z;
        int tw;
        position_at<NC>(coef, dur, (size_t)d * M, M, q == 0 ? tf : tl, x, y, z);
        const double v = mesh_distance_at(x, y, z, n_tris, tris, tw);
        df = q == 0 ? v : df;
        wf = q == 0 ? tw : wf;
        dl = q == 0 ? dl : v;
        wl = q == 0 ? wl : tw;
      }
    }
  }
  t_clear_until[d] = cu;
  t_first[d] = tf;
  d_first[d] = df;
  tri_first[d] = wf;
  t_last[d] = tl;
  d_last[d] = dl;
  tri_last[d] = wl;
  t_clear_from[d] = cf;
  status[d] = st;
}

template <int NC>
int launch(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int n_tris, const double *tris,
           double threshold, double t_res, void *scratch, const Outputs &o) {
  const size_t segs = (size_t)N * M;
  double *work = (double *)scratch;
  int32_t *flags = (int32_t *)(work + kWindowLaneDoubles * segs);
  hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, segs, flags);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((mesh_conflict_lane_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, (const int32_t *)flags, N, M, n_tris, tris, threshold, t_res, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((mesh_conflict_fold_kernel<NC>), dim3(blocks_of(N, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, (const int32_t *)flags, (const double *)work, N, M, n_tris, tris, o.t_clear_until,
                     o.t_first, o.d_first, o.tri_first, o.t_last, o.d_last, o.tri_last, o.t_clear_from, o.status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_mesh_conflict(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int n_tris,
                         const double *tris, double threshold, double t_res, const Outputs &o) {
  const int rc = ensure(ctx, ctx->mesh_clearance_work, mesh_conflict_work_bytes(N, M));
  if (rc) return rc;
  void *scratch = ctx->mesh_clearance_work.p;
  return ctx->order == 7 ? launch<8>(ctx, N, M, coef, dur, n_tris, tris, threshold, t_res, scratch, o)
                         : launch<10>(ctx, N, M, coef, dur, n_tris, tris, threshold, t_res, scratch, o);
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

static int mesh_conflict_args(const msnap_ctx *ctx, int n_drones, int n_seg, int n_tris, const void *tris,
                              double threshold, double t_res, std::initializer_list<const void *> ptrs) {
  if (!ctx || n_drones < 0 || n_tris < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (int rc = check_walk_grid(n_drones, n_seg)) return rc;
  if (!window_levels_valid(t_res, threshold)) return MSNAP_EINVAL;
  if (n_drones == 0) return kNoWork;
  if (n_tris > 0 && !tris) return MSNAP_EINVAL;
  return all_required(ptrs);
}

int msnap_mesh_conflict_window_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                      int n_tris, const double *tris, double threshold, double t_res,
                                      double *t_clear_until, double *t_first, double *d_first, int32_t *tri_first,
                                      double *t_last, double *d_last, int32_t *tri_last, double *t_clear_from,
                                      int32_t *status) {
  MSNAP_ENTER(ctx, mesh_conflict_args(ctx, n_drones, n_seg, n_tris, tris, threshold, t_res,
                                      {coef, dur, t_clear_until, t_first, d_first, tri_first, t_last, d_last, tri_last,
                                       t_clear_from, status}));
  return launch_mesh_conflict(ctx, n_drones, n_seg, coef, dur, n_tris, tris, threshold, t_res,
                              {t_clear_until, t_first, d_first, tri_first, t_last, d_last, tri_last, t_clear_from,
                               status});
}

int msnap_mesh_conflict_window(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                               int n_tris, const double *tris, double threshold, double t_res, double *t_clear_until,
                               double *t_first, double *d_first, int32_t *tri_first, double *t_last, double *d_last,
                               int32_t *tri_last, double *t_clear_from, int32_t *status) {
  MSNAP_ENTER(ctx, mesh_conflict_args(ctx, n_drones, n_seg, n_tris, tris, threshold, t_res,
                                      {coef, dur, t_clear_until, t_first, d_first, tri_first, t_last, d_last, tri_last,
                                       t_clear_from, status}));
  const size_t b_out = (size_t)n_drones * 8, b_int = (size_t)n_drones * 4;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(tris, (size_t)n_tris * 9 * 8), download(t_clear_until, b_out), download(t_first, b_out),
                      download(d_first, b_out), download(tri_first, b_int), download(t_last, b_out),
                      download(d_last, b_out), download(tri_last, b_int), download(t_clear_from, b_out),
                      download(status, b_int)},
                [&](const DevPtr *d) {
                  return launch_mesh_conflict(ctx, n_drones, n_seg, d[0], d[1], n_tris, d[2], threshold, t_res,
                                              {d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]});
                });
}

}  // extern "C"
