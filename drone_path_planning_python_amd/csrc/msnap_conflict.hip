// Conflict windows of two drones in continuous time: from when until when the pair is closer than a threshold
// (include/msnap.h, "conflict windows").  Two entries, told apart by the template flag CROSS exactly as
// msnap_clearance.hip's: msnap_pair_conflict_window (one batch, one clock) and msnap_cross_conflict_window (two sets on
// shifted clocks).  The window [S, W], the knots, the slots, the tie order and the live / dead rules are K9's: the lane
// set-up is msnap_pair_interval.h's lane_interval, the one text both lane kernels call.
//
// Lane.  g(u) = sum of the squares of the three difference polynomials on the lane's interval, L = threshold^2, for
// the bound and for the attained values.  The walk in both directions, the node rule and the lane's four numbers are
// msnap_window.h's (first_crossing, window_lane_tail); the node step here: shift_scale, the smallest Bernstein
// coefficient of g on the node (squares_bound<true>), g at 0, 1/2, 1.
// A lane cannot know that an earlier slot already holds the first conflict: later slots are walked in full.
//
// Fold.  One thread per pair over its slots (msnap_window.h, fold_window); then the distances at t_first and t_last in
// the t domain (pair_distance_at: msnap_eval_flat reproduces them).  Status, W < S and W == S as pair_fold_kernel.
// Nothing crosses lanes but the trip count.
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_pair_interval.h"
#include "msnap_wave.h"
#include "msnap_window.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;
// ctx->clearance_work: per-lane results [lanes][4] doubles, then the flags as msnap_clearance.hip lays them out
inline size_t conflict_work_bytes(size_t lanes, size_t segs) {
  return lanes * kWindowLaneDoubles * sizeof(double) + segs * sizeof(int32_t);
}

// one lane per (pair, slot): work[4 item ..] = the four times of the head, on the common clock
template <int NC, bool CROSS>
__global__ void __launch_bounds__(kThreads)
conflict_lane_kernel(const PathSet A, const PathSet B_, int n_pairs, const int32_t *__restrict__ pairs, double L,
                     double t_res, double *__restrict__ work) {
  constexpr int D = NC - 1;
  const PathSet &B = CROSS ? B_ : A;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = item < (size_t)n_pairs * (size_t)(A.m + B.m - 1);
  double e[3][D + 1];
  const LaneInterval iv = lane_interval<NC, CROSS>(A, B, n_pairs, pairs, item, e);

  // the node step: g = the sum of the squares of the three difference polynomials, its smallest Bernstein coefficient
  const auto values = [&](double a, double hh, bool, double &bound, double (&g)[3]) {
    double f[3][D + 1];
#pragma unroll
    for (int s = 0; s < 3; ++s) shift_scale<D>(e[s], a, hh, f[s]);
    bound = squares_bound<true, D>(f);
    squares_at_ends_and_middle<D>(f, g);
  };
  const auto walk = [&](double &hit, double &clear) { first_crossing(values, iv.ok, iv.h, L, L, t_res, hit, clear); };
  double out[kWindowLaneDoubles];
  window_lane_tail(e, iv.ok, iv.h, iv.start, iv.E, walk, out);

  if (!in_range) return;
#pragma unroll
  for (int q = 0; q < kWindowLaneDoubles; ++q) work[kWindowLaneDoubles * item + q] = out[q];
}

// one thread per pair: status, the window, the fold of the slots, the distances in the t domain
template <int NC, bool CROSS>
__global__ void __launch_bounds__(kThreads)
conflict_fold_kernel(const PathSet A, const PathSet B_, const double *__restrict__ work, int n_pairs,
                     const int32_t *__restrict__ pairs, double threshold, double *__restrict__ t_clear_until,
                     double *__restrict__ t_first, double *__restrict__ d_first, double *__restrict__ t_last,
                     double *__restrict__ d_last, double *__restrict__ t_clear_from, int32_t *__restrict__ status) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const PathSet &B = CROSS ? B_ : A;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
  const size_t da = (size_t)a * A.m, db = (size_t)b * B.m;
  double ta, tb, totA, totB;      // (CROSS only: the clamp's)
  const int st = pair_status<CROSS>(A, B, a, b, ta, tb, totA, totB);
  double cu = nan, tf = nan, df = nan, tl = nan, dl = nan, cf = nan;
  if (st == MSNAP_ST_OK) {
    const double S = fmax(ta, tb), Wend = CROSS ? fmin(ta + totA, tb + totB) : inf;
    cu = tf = inf;      // certified clear over the whole window
    tl = cf = -inf;
    const bool instant = CROSS && Wend == S;      // no slot is live: the one instant decides
    if (instant) {
      cu = tf = tl = cf = S;
    } else if (!(Wend < S)) {
      const int slots = A.m + B.m - 1;
      fold_window(work + (size_t)p * slots * kWindowLaneDoubles, slots, cu, tf, tl, cf);
    }
    df = dl = inf;
    if (tf < inf) {
#pragma unroll 1
      for (int q = 0; q < 2; ++q) {      // (one text of the evaluation for both ends)
        const double d = pair_distance_at<NC, CROSS>(A, B, da, db, ta, tb, totA, totB, q == 0 ? tf : tl);
        df = q == 0 ? d : df;
        dl = q == 0 ? dl : d;
      }
    }
    if (instant && !(df < threshold)) {      // clear at that instant: certified clear
      cu = tf = df = dl = inf;
      tl = cf = -inf;
    }
  }
  t_clear_until[p] = cu;
  t_first[p] = tf;
  d_first[p] = df;
  t_last[p] = tl;
  d_last[p] = dl;
  t_clear_from[p] = cf;
  status[p] = st;
}

struct Outputs {
  double *t_clear_until, *t_first, *d_first, *t_last, *d_last, *t_clear_from;
  int32_t *status;
};

template <int NC, bool CROSS>
int launch(msnap_ctx *ctx, PathSet A, PathSet B, int n_pairs, const int32_t *pairs, double threshold, double t_res,
           void *scratch, const Outputs &o) {
  const size_t lanes = clearance_lanes(n_pairs, A.m, B.m), segs_a = (size_t)A.n * A.m;
  double *work = (double *)scratch;
  int32_t *flags[2] = {(int32_t *)(work + kWindowLaneDoubles * lanes), nullptr};
  flags[1] = CROSS ? flags[0] + segs_a : flags[0];
  PathSet *sets[2] = {&A, &B};
  for (int s = 0; s < (CROSS ? 2 : 1); ++s) {
    const size_t segs = (size_t)sets[s]->n * sets[s]->m;
    if (!segs) continue;
    hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                       sets[s]->coef, sets[s]->dur, segs, flags[s]);
    MSNAP_HIP(ctx, hipGetLastError());
  }
  A.flags = flags[0];
  B.flags = flags[1];
  hipLaunchKernelGGL((conflict_lane_kernel<NC, CROSS>), dim3(blocks_of(lanes, kThreads)), dim3(kThreads), 0,
                     ctx->stream, A, B, n_pairs, pairs, threshold * threshold, t_res, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((conflict_fold_kernel<NC, CROSS>), dim3(blocks_of(n_pairs, kThreads)), dim3(kThreads), 0,
                     ctx->stream, A, B, (const double *)work, n_pairs, pairs, threshold, o.t_clear_until, o.t_first,
                     o.d_first, o.t_last, o.d_last, o.t_clear_from, o.status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// cross = false: B is A given again (those instances read only A)
int launch_conflict(msnap_ctx *ctx, bool cross, const PathSet &A, const PathSet &B, int n_pairs, const int32_t *pairs,
                    double threshold, double t_res, const Outputs &o) {
  const size_t segs = (size_t)A.n * A.m + (cross ? (size_t)B.n * B.m : 0);
  const int rc = ensure(ctx, ctx->clearance_work, conflict_work_bytes(clearance_lanes(n_pairs, A.m, B.m), segs));
  if (rc) return rc;
  void *scratch = ctx->clearance_work.p;
  if (ctx->order == 7)
    return cross ? launch<8, true>(ctx, A, B, n_pairs, pairs, threshold, t_res, scratch, o)
                 : launch<8, false>(ctx, A, B, n_pairs, pairs, threshold, t_res, scratch, o);
  return cross ? launch<10, true>(ctx, A, B, n_pairs, pairs, threshold, t_res, scratch, o)
               : launch<10, false>(ctx, A, B, n_pairs, pairs, threshold, t_res, scratch, o);
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

static int conflict_args(const msnap_ctx *ctx, int n_a, int n_seg_a, int n_b, int n_seg_b, int n_pairs,
                         double threshold, double t_res, std::initializer_list<const void *> ptrs) {
  if (int rc = check_clearance_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs)) return rc;
  if (!window_levels_valid(t_res, threshold)) return MSNAP_EINVAL;
  if (n_pairs == 0) return kNoWork;
  return all_required(ptrs);
}

int msnap_pair_conflict_window_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                      int n_pairs, const int32_t *pairs, double threshold, double t_res,
                                      double *t_clear_until, double *t_first, double *d_first, double *t_last,
                                      double *d_last, double *t_clear_from, int32_t *status) {
  MSNAP_ENTER(ctx, conflict_args(ctx, n_drones, n_seg, n_drones, n_seg, n_pairs, threshold, t_res,
                                 {coef, dur, pairs, t_clear_until, t_first, d_first, t_last, d_last, t_clear_from,
                                  status}));
  const PathSet A = {n_drones, n_seg, coef, dur, nullptr, nullptr};
  return launch_conflict(ctx, false, A, A, n_pairs, pairs, threshold, t_res,
                         {t_clear_until, t_first, d_first, t_last, d_last, t_clear_from, status});
}

int msnap_pair_conflict_window(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                               int n_pairs, const int32_t *pairs, double threshold, double t_res,
                               double *t_clear_until, double *t_first, double *d_first, double *t_last, double *d_last,
                               double *t_clear_from, int32_t *status) {
  MSNAP_ENTER(ctx, conflict_args(ctx, n_drones, n_seg, n_drones, n_seg, n_pairs, threshold, t_res,
                                 {coef, dur, pairs, t_clear_until, t_first, d_first, t_last, d_last, t_clear_from,
                                  status}));
  const size_t b_out = (size_t)n_pairs * 8;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(pairs, (size_t)n_pairs * 2 * 4), download(t_clear_until, b_out), download(t_first, b_out),
                      download(d_first, b_out), download(t_last, b_out), download(d_last, b_out),
                      download(t_clear_from, b_out), download(status, (size_t)n_pairs * 4)},
                [&](const DevPtr *d) {
                  const PathSet A = {n_drones, n_seg, d[0], d[1], nullptr, nullptr};
                  return launch_conflict(ctx, false, A, A, n_pairs, d[2], threshold, t_res,
                                         {d[3], d[4], d[5], d[6], d[7], d[8], d[9]});
                });
}

int msnap_cross_conflict_window_device(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                                       const double *t0_a, int n_b, int n_seg_b, const double *coef_b,
                                       const double *dur_b, const double *t0_b, int n_pairs, const int32_t *pairs,
                                       double threshold, double t_res, double *t_clear_until, double *t_first,
                                       double *d_first, double *t_last, double *d_last, double *t_clear_from,
                                       int32_t *status) {
  MSNAP_ENTER(ctx, conflict_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs, threshold, t_res,
                                 {coef_a, dur_a, coef_b, dur_b, pairs, t_clear_until, t_first, d_first, t_last, d_last,
                                  t_clear_from, status}));
  return launch_conflict(ctx, true, {n_a, n_seg_a, coef_a, dur_a, t0_a, nullptr},
                         {n_b, n_seg_b, coef_b, dur_b, t0_b, nullptr}, n_pairs, pairs, threshold, t_res,
                         {t_clear_until, t_first, d_first, t_last, d_last, t_clear_from, status});
}

int msnap_cross_conflict_window(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                                const double *t0_a, int n_b, int n_seg_b, const double *coef_b, const double *dur_b,
                                const double *t0_b, int n_pairs, const int32_t *pairs, double threshold, double t_res,
                                double *t_clear_until, double *t_first, double *d_first, double *t_last, double *d_last,
                                double *t_clear_from, int32_t *status) {
  MSNAP_ENTER(ctx, conflict_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs, threshold, t_res,
                                 {coef_a, dur_a, coef_b, dur_b, pairs, t_clear_until, t_first, d_first, t_last, d_last,
                                  t_clear_from, status}));
  const size_t b_out = (size_t)n_pairs * 8;
  return staged(ctx, {upload(coef_a, coef_bytes(ctx, n_a, n_seg_a)), upload(dur_a, dur_bytes(n_a, n_seg_a)),
                      upload(t0_a, t0_a ? (size_t)n_a * 8 : 0), upload(coef_b, coef_bytes(ctx, n_b, n_seg_b)),
                      upload(dur_b, dur_bytes(n_b, n_seg_b)), upload(t0_b, t0_b ? (size_t)n_b * 8 : 0),
                      upload(pairs, (size_t)n_pairs * 2 * 4), download(t_clear_until, b_out), download(t_first, b_out),
                      download(d_first, b_out), download(t_last, b_out), download(d_last, b_out),
                      download(t_clear_from, b_out), download(status, (size_t)n_pairs * 4)},
                [&](const DevPtr *d) {
                  const double *da = t0_a ? (const double *)d[2] : nullptr, *db = t0_b ? (const double *)d[5] : nullptr;
                  return launch_conflict(ctx, true, {n_a, n_seg_a, d[0], d[1], da, nullptr},
                                         {n_b, n_seg_b, d[3], d[4], db, nullptr}, n_pairs, d[6], threshold, t_res,
                                         {d[7], d[8], d[9], d[10], d[11], d[12], d[13]});
                });
}

}  // extern "C"
