// Clearance of two drones in continuous time: the certified minimum distance of drone a and drone b while both fly.
// One method, two entries (include/msnap.h), told apart by the template flag CROSS:
//   CROSS = false  msnap_pair_clearance (K9): both drones from ONE batch on ONE clock.  Set B is set A, every offset is
//                  the literal zero (no t0 is read, no 0.0 + x is formed), the window starts at 0, a == b is no pair.
//   CROSS = true   msnap_cross_clearance (K14): drone a of set A against drone b of set B, each set with its own
//                  segment count, each drone with its own start time t0 on a common clock (NULL: zeros).
// With A == B and zero offsets the CROSS instance performs K9's operations (an offset of 0.0 added to or subtracted from
// a time changes no bit of it).
//
// Clock.  Drone a is at P_a(t - t0_a[a]) at common time t.  Its knots on the common clock are fl(t0_a + acc_i), acc_i
// the running sums acc = acc + T of its durations (as peaks_fold_kernel and msnap_eval_flat form them); set B likewise.
// The window is [S, W], S = max(t0_a, t0_b), W = min(fl(t0_a + total_a), fl(t0_b + total_b)).  A drone that has landed
// is NOT held at its end point: what happens after the shorter path ends is out of scope here.
//
// Intervals.  Between consecutive knots of the two drones |p_a - p_b|^2 is one polynomial.  The end points inside the
// window are the Ma - 1 interior knots of a, the Mb - 1 interior knots of b and W itself: Ma + Mb - 1 slots, one lane
// per (pair, slot).  The lane's interval ends at its end point and starts at the largest end point below it or at S,
// ties ordered a's knots < b's knots < W -- so coincident knots (a shared grid) leave the later slot empty, a slot whose
// end point lies at or below S, or beyond W, is dead, and every live interval is found exactly once whichever drone is
// called a.  Both are found with two uniform loops over the durations of the two drones (every lane of a pair loads
// the same addresses).
//
// Lane.  Per axis x, y, z: Taylor shift of each drone's polynomial to ITS local time at the interval's start,
// fl(fl(start - t0) - knot) -- what msnap_eval_flat forms for the local time fl(start - t0) --, the DIFFERENCE of the
// two (before any square: near a minimum the distance carries the rounding of the difference, not of the positions),
// scaled by h^j to u in [0, 1].  g(u) = sum of the three squares, degree 2 order.  Then the walk of msnap_walk.h for a
// minimum: the smallest Bernstein coefficient of g as a lower bound, a node pruned when
// bound >= L (1 - kPruneRel) - kPruneAbs, L the smallest attained value; the lane carries what the walk proved.
//
// Fold.  One thread per pair over its slots: smallest attained value, then earliest time; smallest bound.  The attained
// value is evaluated again at t_min in the t domain -- msnap_eval_flat's segment lookup and Horner at the local times
// (CROSS: clamped, tau_x = min(max(fl(t_min - t0_x), 0), total_x)), the formation pass's
// fma(dz, dz, fma(dy, dy, dx dx)) -- so that eval_flat at t_min reproduces min_dist.  CROSS, W < S: +inf, NaN, +inf;
// W == S: no slot is live, the distance at S.  Nothing crosses lanes but the trip count: a pair's outputs do not depend
// on its place in the list, and (b, a) gives the bits of (a, b) (the difference changes sign exactly, every later
// quantity is even in it).
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_pair_interval.h"
#include "msnap_walk.h"
#include "msnap_wave.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;
constexpr double kPruneRel = 2e-9;       // on g = |.|^2: 1e-9 on the distance
constexpr double kPruneAbs = 1e-18;      // on g: A^2 with A = 1e-9 m (DESIGN.md §5 K9 has the depth arithmetic)

// PathSet, the clock rules and the interval set-up of a lane: msnap_pair_interval.h (shared with msnap_conflict.hip)

// one lane per (pair, slot): the triple of store_lane (msnap_walk.h)
template <int NC, bool CROSS>
__global__ void __launch_bounds__(kThreads)
pair_lane_kernel(const PathSet A, const PathSet B_, int n_pairs, const int32_t *__restrict__ pairs,
                 double *__restrict__ work) {
  constexpr int D = NC - 1;       // degree of the positions
  const PathSet &B = CROSS ? B_ : A;
  const double inf = __builtin_inf();
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = item < (size_t)n_pairs * (size_t)(A.m + B.m - 1);
  double e[3][D + 1];
  const LaneInterval iv = lane_interval<NC, CROSS>(A, B, n_pairs, pairs, item, e);
  const double h = iv.h, start = iv.start, E = iv.E;
  const bool ok = iv.ok;

  // branch and bound over the dyadic sub-intervals (msnap_walk.h); every lane runs the body while any lane is active
  double best = inf, best_u = 0.0;
  WalkNode node;
  ProvenBound proven;
  bool active = ok;
  while (__ballot(active) != 0) {
    const double hh = node.h(), a = node.a();
    double f[3][D + 1];
#pragma unroll
    for (int s = 0; s < 3; ++s) shift_scale<D>(e[s], a, hh, f[s]);
    const double bound = squares_bound<true, D>(f);
    double g[3];
    squares_at_ends_and_middle<D>(f, g);
    double nb = best, nu = best_u;
    take_attained<true>(g, a, hh, nb, nu);
    if (active) { best = nb; best_u = nu; }
    const bool split = bound < fma(-kPruneRel, best, best) - kPruneAbs && node.lvl < kMaxDepth;
    const bool finished = node.advance(split, active);
    const bool guard = proven.note(node, bound, split, finished, active);
    active = active && !(finished || guard);
  }

  if (!in_range) return;
  store_lane(work, item, ok, best, best_u, proven.low, h, start, E);
}

// one thread per pair: status, the window, the fold of the slots (smaller value, then earlier time; smallest bound),
// the attained value again in the t domain
template <int NC, bool CROSS>
__global__ void __launch_bounds__(kThreads)
pair_fold_kernel(const PathSet A, const PathSet B_, const double *__restrict__ work, int n_pairs,
                 const int32_t *__restrict__ pairs, double *__restrict__ min_dist, double *__restrict__ t_min,
                 double *__restrict__ lower, int32_t *__restrict__ status) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const PathSet &B = CROSS ? B_ : A;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
  const size_t da = (size_t)a * A.m, db = (size_t)b * B.m;
  double ta, tb, totA, totB;      // (CROSS only: the clamp's)
  const int st = pair_status<CROSS>(A, B, a, b, ta, tb, totA, totB);
  double md = nan, tm = nan, lo = nan;
  const double S = fmax(ta, tb);
  if (st == MSNAP_ST_OK && CROSS && fmin(ta + totA, tb + totB) < S) {      // the drones never fly at the same time
    md = inf;
    lo = inf;
  } else if (st == MSNAP_ST_OK) {
    const int slots = A.m + B.m - 1;
    double best, bt, low;
    fold_slots(work + (size_t)p * slots * 3, slots, best, bt, low);
    if (CROSS && !(best < inf)) bt = S;      // no live slot: W == S, the one instant
    md = pair_distance_at<NC, CROSS>(A, B, da, db, ta, tb, totA, totB, bt);
    tm = bt;
    lo = fmin(sqrt(fmax(low, 0.0)), md);      // (an attained value bounds the infimum too)
  }
  min_dist[p] = md;
  t_min[p] = tm;
  lower[p] = lo;
  status[p] = st;
}

template <int NC, bool CROSS>
int launch(msnap_ctx *ctx, PathSet A, PathSet B, int n_pairs, const int32_t *pairs, void *scratch, double *min_dist,
           double *t_min, double *lower, int32_t *status) {
  const size_t lanes = clearance_lanes(n_pairs, A.m, B.m), segs_a = (size_t)A.n * A.m;
  double *work = (double *)scratch;
  int32_t *flags[2] = {(int32_t *)(work + 3 * lanes), nullptr};
  flags[1] = CROSS ? flags[0] + segs_a : flags[0];
  PathSet *sets[2] = {&A, &B};
  for (int s = 0; s < (CROSS ? 2 : 1); ++s) {       // K9's set B is its set A: one flags launch
    const size_t segs = (size_t)sets[s]->n * sets[s]->m;
    if (!segs) continue;
    hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                       sets[s]->coef, sets[s]->dur, segs, flags[s]);
    MSNAP_HIP(ctx, hipGetLastError());
  }
  A.flags = flags[0];
  B.flags = flags[1];
  hipLaunchKernelGGL((pair_lane_kernel<NC, CROSS>), dim3(blocks_of(lanes, kThreads)), dim3(kThreads), 0, ctx->stream,
                     A, B, n_pairs, pairs, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((pair_fold_kernel<NC, CROSS>), dim3(blocks_of(n_pairs, kThreads)), dim3(kThreads), 0, ctx->stream,
                     A, B, (const double *)work, n_pairs, pairs, min_dist, t_min, lower, status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// cross = false: B is A given again (the K9 instances read only A)
int launch_clearance(msnap_ctx *ctx, bool cross, const PathSet &A, const PathSet &B, int n_pairs, const int32_t *pairs,
                     double *min_dist, double *t_min, double *lower, int32_t *status) {
  const size_t segs = (size_t)A.n * A.m + (cross ? (size_t)B.n * B.m : 0);
  const int rc = ensure(ctx, ctx->clearance_work, clearance_work_bytes(clearance_lanes(n_pairs, A.m, B.m), segs));
  if (rc) return rc;
  void *scratch = ctx->clearance_work.p;
  if (ctx->order == 7)
    return cross ? launch<8, true>(ctx, A, B, n_pairs, pairs, scratch, min_dist, t_min, lower, status)
                 : launch<8, false>(ctx, A, B, n_pairs, pairs, scratch, min_dist, t_min, lower, status);
  return cross ? launch<10, true>(ctx, A, B, n_pairs, pairs, scratch, min_dist, t_min, lower, status)
               : launch<10, false>(ctx, A, B, n_pairs, pairs, scratch, min_dist, t_min, lower, status);
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

// the entry points live beside their launcher, as msnap_timeopt.hip's do
static int clearance_args(const msnap_ctx *ctx, int n_a, int n_seg_a, int n_b, int n_seg_b, int n_pairs,
                          std::initializer_list<const void *> ptrs) {
  if (int rc = check_clearance_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs)) return rc;
  if (n_pairs == 0) return kNoWork;
  return all_required(ptrs);
}

int msnap_pair_clearance_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                int n_pairs, const int32_t *pairs, double *min_dist, double *t_min, double *lower,
                                int32_t *status) {
  MSNAP_ENTER(ctx, clearance_args(ctx, n_drones, n_seg, n_drones, n_seg, n_pairs,
                                  {coef, dur, pairs, min_dist, t_min, lower, status}));
  const PathSet A = {n_drones, n_seg, coef, dur, nullptr, nullptr};
  return launch_clearance(ctx, false, A, A, n_pairs, pairs, min_dist, t_min, lower, status);
}

int msnap_pair_clearance(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_pairs,
                         const int32_t *pairs, double *min_dist, double *t_min, double *lower, int32_t *status) {
  MSNAP_ENTER(ctx, clearance_args(ctx, n_drones, n_seg, n_drones, n_seg, n_pairs,
                                  {coef, dur, pairs, min_dist, t_min, lower, status}));
  const size_t b_out = (size_t)n_pairs * 8;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(pairs, (size_t)n_pairs * 2 * 4), download(min_dist, b_out), download(t_min, b_out),
                      download(lower, b_out), download(status, (size_t)n_pairs * 4)},
                [&](const DevPtr *d) {
                  const PathSet A = {n_drones, n_seg, d[0], d[1], nullptr, nullptr};
                  return launch_clearance(ctx, false, A, A, n_pairs, d[2], d[3], d[4], d[5], d[6]);
                });
}

int msnap_cross_clearance_device(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                                 const double *t0_a, int n_b, int n_seg_b, const double *coef_b, const double *dur_b,
                                 const double *t0_b, int n_pairs, const int32_t *pairs, double *min_dist, double *t_min,
                                 double *lower, int32_t *status) {
  MSNAP_ENTER(ctx, clearance_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs,
                                  {coef_a, dur_a, coef_b, dur_b, pairs, min_dist, t_min, lower, status}));
  return launch_clearance(ctx, true, {n_a, n_seg_a, coef_a, dur_a, t0_a, nullptr},
                          {n_b, n_seg_b, coef_b, dur_b, t0_b, nullptr}, n_pairs, pairs, min_dist, t_min, lower, status);
}

int msnap_cross_clearance(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                          const double *t0_a, int n_b, int n_seg_b, const double *coef_b, const double *dur_b,
                          const double *t0_b, int n_pairs, const int32_t *pairs, double *min_dist, double *t_min,
                          double *lower, int32_t *status) {
  MSNAP_ENTER(ctx, clearance_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs,
                                  {coef_a, dur_a, coef_b, dur_b, pairs, min_dist, t_min, lower, status}));
  const size_t b_out = (size_t)n_pairs * 8;
  return staged(ctx, {upload(coef_a, coef_bytes(ctx, n_a, n_seg_a)), upload(dur_a, dur_bytes(n_a, n_seg_a)),
                      upload(t0_a, t0_a ? (size_t)n_a * 8 : 0), upload(coef_b, coef_bytes(ctx, n_b, n_seg_b)),
                      upload(dur_b, dur_bytes(n_b, n_seg_b)), upload(t0_b, t0_b ? (size_t)n_b * 8 : 0),
                      upload(pairs, (size_t)n_pairs * 2 * 4), download(min_dist, b_out), download(t_min, b_out),
                      download(lower, b_out), download(status, (size_t)n_pairs * 4)},
                [&](const DevPtr *d) {
                  const double *da = t0_a ? (const double *)d[2] : nullptr, *db = t0_b ? (const double *)d[5] : nullptr;
                  return launch_clearance(ctx, true, {n_a, n_seg_a, d[0], d[1], da, nullptr},
                                          {n_b, n_seg_b, d[3], d[4], db, nullptr}, n_pairs, d[6], d[7], d[8], d[9], d[10]);
                });
}

}  // extern "C"
