// Mesh clearance in continuous time: the certified minimum distance of each drone's whole path to a triangle mesh
// (include/msnap.h, "mesh clearance").  The distance function is the mesh sweep's (msnap_tri.h).
//
// Bound.  msnap_mesh_bound.h: per triangle the largest of three support-plane bounds from the node's Bernstein control
// points (tri_node_bound), the text K19's lane kernel calls as well.
//
// Lane.  One per (drone, segment): the segment's x, y, z scaled to u in [0, 1], then the walk of msnap_walk.h for a
// minimum; per node the control points and a loop over the triangles (wave-uniform: scalar loads), each first tried
// with box_tri_lb2 of the control points' box against the prune threshold, which leaves few.  A node's bound is the
// smallest over the triangles; the distances at its start, middle and end are attained values.  A node is pruned when
// bound >= L (1 - kPruneRel) - kPruneAbs, L the smallest attained distance; the lane carries what the walk proved.
//
// Fold.  One thread per drone over its segments: smallest attained value, then earliest absolute time; smallest bound.
// The distance is taken again at t_min -- msnap_eval_flat's lookup and Horner, every triangle in index order through
// the sweep's functions, strict `<` -- so that msnap_mesh_sweep of that one position returns min_dist bit for bit and
// tri_min is the lowest index that attains it.  Nothing crosses lanes but the trip count.
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_mesh_bound.h"
#include "msnap_walk.h"
#include "msnap_wave.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;
constexpr double kPruneRel = 1e-9;       // on the distance (msnap_clearance.hip's 2e-9 on the square)
constexpr double kPruneAbs = 1e-9;       // [m]: what lets a crossing (D = 0) close

// one lane per (drone, segment): work[3 item] = smallest attained SQUARED distance of the segment (+inf: no triangle,
// or a failed drone), [3 item + 1] = its absolute time, [3 item + 2] = the proven lower bound of the distance there
template <int NC>
__global__ void __launch_bounds__(kThreads)
mesh_clearance_lane_kernel(const double *__restrict__ coef, const double *__restrict__ dur,
                           const int32_t *__restrict__ flags, int N, int M, int n_tris,
                           const double *__restrict__ tris, double *__restrict__ work) {
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

  // branch and bound over the dyadic sub-intervals (msnap_walk.h); every lane runs the body while any lane is active
  double best = inf, best_u = 0.0;      // best: a squared distance; the proven bound: a distance
  WalkNode node;
  ProvenBound proven;
  bool active = ok;
  while (__ballot(active) != 0) {
    const double hh = node.h(), a = node.a();
    // control points b[s][i] of axis s on the node, its three points p[.][s] (x = 0, 1/2, 1) and the points' box
    double b[3][D + 1], p[3][3], lo[3], hi[3];
    node_points<D>(e, a, hh, b, p, lo, hi);
    // the threshold a triangle's box has to beat to be left out: the one the node is pruned against, from the attained
    // values so far (NaN while there is none: nothing is left out)
    const double sb0 = sqrt(best);
    const double thr0 = fma(-kPruneRel, sb0, sb0) - kPruneAbs;
    const double thr0sq = thr0 * thr0;
    double nb = best, nu = best_u;
    double bound = inf, skipped = inf;      // bound: a distance; skipped: the smallest squared box distance left out
    for (int t = 0; t < n_tris; ++t) {
      const double *tri = tris + (size_t)t * 9;
      if (!tri_finite(tri)) continue;
      const double lb2 = box_tri_lb2(lo, hi, tri);
      const bool need = active && !(thr0 > 0.0 && lb2 >= thr0sq);
      skipped = need ? skipped : fmin(skipped, lb2);
      if (__ballot(need) == 0) continue;
      double d2[3];
      const double tb = tri_node_bound<D>(tri, b, p, d2);
      // attained values, earlier first: a tie keeps the earlier time (and, in the fold, the lower triangle)
      if (need) take_attained<true>(d2, a, hh, nb, nu);
      bound = need ? fmin(bound, tb) : bound;
    }
    // (what was left out lies at least thr0 away: said again, so that a last-bit difference between the squared compare
    // above and this square root cannot split the node for it)
    bound = fmin(bound, fmax(sqrt(skipped), thr0));
    if (active) { best = nb; best_u = nu; }
    const double sb = sqrt(best);
    const bool split = bound < fma(-kPruneRel, sb, sb) - kPruneAbs && node.lvl < kMaxDepth;
    const bool finished = node.advance(split, active);
    const bool guard = proven.note(node, bound, split, finished, active);
    active = active && !(finished || guard);
  }

  if (!in_range) return;
  store_lane(work, item, ok, best, best_u, proven.low, T, start, E);
}

// one thread per drone: fold the segments (smaller value, then earlier time; smallest bound), status, and the distance
// again at t_min through the sweep's functions, every triangle in index order
template <int NC>
__global__ void __launch_bounds__(kThreads)
mesh_clearance_fold_kernel(const double *__restrict__ coef, const double *__restrict__ dur,
                           const int32_t *__restrict__ flags, const double *__restrict__ work, int N, int M, int n_tris,
                           const double *__restrict__ tris, double *__restrict__ min_dist, double *__restrict__ t_min,
                           int32_t *__restrict__ tri_min, double *__restrict__ lower, int32_t *__restrict__ status) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= N) return;
  const double nan = __builtin_nan("");
  int bad = 0;
  for (int i = 0; i < M; ++i) bad |= flags[(size_t)d * M + i];
  const int st = status_of_flags(bad);
  double md = nan, tm = nan, lo = nan;
  int tw = -1;
  if (st == MSNAP_ST_OK) {
    const double *w = work + (size_t)d * M * 3;
    double best, bt, low;
    fold_slots(w, M, best, bt, low);
    double x, y, z;
    position_at<NC>(coef, dur, (size_t)d * M, M, bt, x, y, z);
    md = mesh_distance_at(x, y, z, n_tris, tris, tw);
    tm = bt;
    lo = fmin(fmax(low, 0.0), md);      // (a distance is not negative, and an attained value bounds the infimum too)
  }
  min_dist[d] = md;
  t_min[d] = tm;
  tri_min[d] = tw;
  lower[d] = lo;
  status[d] = st;
}

template <int NC>
int launch(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int n_tris, const double *tris,
           void *scratch, double *min_dist, double *t_min, int32_t *tri_min, double *lower, int32_t *status) {
  const size_t segs = (size_t)N * M;
  double *work = (double *)scratch;
  int32_t *flags = (int32_t *)(work + 3 * segs);
  hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, segs, flags);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((mesh_clearance_lane_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, (const int32_t *)flags, N, M, n_tris, tris, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((mesh_clearance_fold_kernel<NC>), dim3(blocks_of(N, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, (const int32_t *)flags, (const double *)work, N, M, n_tris, tris, min_dist, t_min,
                     tri_min, lower, status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_mesh_clearance(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int n_tris,
                          const double *tris, double *min_dist, double *t_min, int32_t *tri_min, double *lower,
                          int32_t *status) {
  const int rc = ensure(ctx, ctx->mesh_clearance_work, mesh_clearance_work_bytes(N, M));
  if (rc) return rc;
  void *scratch = ctx->mesh_clearance_work.p;
  return ctx->order == 7
             ? launch<8>(ctx, N, M, coef, dur, n_tris, tris, scratch, min_dist, t_min, tri_min, lower, status)
             : launch<10>(ctx, N, M, coef, dur, n_tris, tris, scratch, min_dist, t_min, tri_min, lower, status);
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

// the entry points live beside their launcher, as msnap_clearance.hip's do
static int mesh_clearance_args(const msnap_ctx *ctx, int n_drones, int n_seg, int n_tris, const void *tris,
                               std::initializer_list<const void *> ptrs) {
  if (!ctx || n_drones < 0 || n_tris < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (int rc = check_walk_grid(n_drones, n_seg)) return rc;
  if (n_drones == 0) return kNoWork;
  if (n_tris > 0 && !tris) return MSNAP_EINVAL;
  return all_required(ptrs);
}

int msnap_mesh_clearance_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                int n_tris, const double *tris, double *min_dist, double *t_min, int32_t *tri_min,
                                double *lower, int32_t *status) {
  MSNAP_ENTER(ctx, mesh_clearance_args(ctx, n_drones, n_seg, n_tris, tris,
                                       {coef, dur, min_dist, t_min, tri_min, lower, status}));
  return launch_mesh_clearance(ctx, n_drones, n_seg, coef, dur, n_tris, tris, min_dist, t_min, tri_min, lower, status);
}

int msnap_mesh_clearance(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_tris,
                         const double *tris, double *min_dist, double *t_min, int32_t *tri_min, double *lower,
                         int32_t *status) {
  MSNAP_ENTER(ctx, mesh_clearance_args(ctx, n_drones, n_seg, n_tris, tris,
                                       {coef, dur, min_dist, t_min, tri_min, lower, status}));
  const size_t b_out = (size_t)n_drones * 8;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(tris, (size_t)n_tris * 9 * 8), download(min_dist, b_out), download(t_min, b_out),
                      download(tri_min, (size_t)n_drones * 4), download(lower, b_out),
                      download(status, (size_t)n_drones * 4)},
                [&](const DevPtr *d) {
                  return launch_mesh_clearance(ctx, n_drones, n_seg, d[0], d[1], n_tris, d[2], d[3], d[4], d[5], d[6],
                                               d[7]);
                });
}

}  // extern "C"
