// Clearance between two path sets on shifted clocks: the certified minimum distance of drone a of set A and drone b
// of set B while both fly, each set with its own segment count, each drone with its own start time on a common clock
// (include/msnap.h, "cross clearance").  msnap_clearance.hip (K9) is the same method for two drones
// of ONE batch on ONE clock; its kernels stay as they are, and with A == B, equal segment counts and zero offsets every
// operation here is the one K9 performs (an offset of 0.0 added to or subtracted from a time changes no bit of it).
//
// Clock.  Drone a is at P_a(t - t0_a[a]) at common time t.  Its knots on the common clock are fl(t0_a + acc_i), acc_i
// the running sums acc = acc + T of its durations; set B likewise.  The window is [S, W], S = max(t0_a, t0_b),
// W = min(fl(t0_a + total_a), fl(t0_b + total_b)).  A drone that has landed is NOT held at its end point.
//
// Intervals.  The end points inside the window are the Ma - 1 interior knots of a, the Mb - 1 interior knots of b and W
// itself: Ma + Mb - 1 slots, one lane per (pair, slot).  The lane's interval ends at its end point and starts at the
// largest end point below it or at S, ties ordered a's knots < b's knots < W.  A slot whose end point lies at or below
// S, or beyond W, is dead.  Both are found with uniform loops over the Ma and the Mb durations (every lane of a pair
// loads the same addresses).
//
// Lane.  Per axis: Taylor shift of each drone's segment to ITS local time at the interval's start,
// fl(fl(start - t0) - knot) -- what msnap_eval_flat forms for the local time fl(start - t0) --, the difference of the
// two, scaled by h^j.  Then msnap_walk.h's walk with K9's prune constants.
//
// Fold.  One thread per pair: fold_slots, then the attained value again through position_at at the clamped local times
// tau_x = min(max(fl(t_min - t0_x), 0), total_x).  W < S: +inf, NaN, +inf.  W == S: no slot is live; the distance at S.
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_walk.h"
#include "msnap_wave.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;
constexpr double kPruneRel = 2e-9;       // K9's: on g = |.|^2, 1e-9 on the distance
constexpr double kPruneAbs = 1e-18;      // on g: A^2 with A = 1e-9 m

__device__ __forceinline__ bool cross_in_range(int a, int b, int Na, int Nb) {
  return a >= 0 && b >= 0 && a < Na && b < Nb;
}

// one lane per (pair, slot): the triple of store_lane (msnap_walk.h)
template <int NC>
__global__ void __launch_bounds__(kThreads)
cross_clearance_lane_kernel(const double *__restrict__ coef_a, const double *__restrict__ dur_a,
                            const double *__restrict__ t0_a, const int32_t *__restrict__ flags_a, int Na, int Ma,
                            const double *__restrict__ coef_b, const double *__restrict__ dur_b,
                            const double *__restrict__ t0_b, const int32_t *__restrict__ flags_b, int Nb, int Mb,
                            int n_pairs, const int32_t *__restrict__ pairs, double *__restrict__ work) {
  constexpr int D = NC - 1;       // degree of the positions
  const double inf = __builtin_inf();
  const int slots = Ma + Mb - 1;
  const size_t total = (size_t)n_pairs * slots;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = item < total;
  const size_t p = in_range ? item / (size_t)slots : 0;
  const int k = (int)(item - p * (size_t)slots);
  const int a0 = in_range ? pairs[2 * p] : 0, b0 = in_range ? pairs[2 * p + 1] : 0;
  const bool pair_ok = in_range && cross_in_range(a0, b0, Na, Nb);
  const size_t da = pair_ok ? (size_t)a0 * Ma : 0, db = pair_ok ? (size_t)b0 * Mb : 0;
  const double ta = (pair_ok && t0_a) ? t0_a[a0] : 0.0, tb = (pair_ok && t0_b) ? t0_b[b0] : 0.0;
  // the slot's end point: an interior knot of a (kind 0), of b (kind 1), or the window's end (kind 2)
  const int kind = k < Ma - 1 ? 0 : (k < Ma + Mb - 2 ? 1 : 2);
  const int own = kind == 0 ? k : k - (Ma - 1);

  // first pass over the durations: the totals, the slot's end point, the drones' flags
  double accA = 0.0, accB = 0.0, E = 0.0;
  int bad = (isfinite(ta) && isfinite(tb)) ? 0 : 2;
  for (int i = 0; i < Ma; ++i) {
    const double Ta = pair_ok ? dur_a[da + i] : 1.0;
    bad |= pair_ok ? flags_a[da + i] : 0;
    accA = accA + Ta;
    if (kind == 0 && i == own) E = ta + accA;
  }
  for (int i = 0; i < Mb; ++i) {
    const double Tb = pair_ok ? dur_b[db + i] : 1.0;
    bad |= pair_ok ? flags_b[db + i] : 0;
    accB = accB + Tb;
    if (kind == 1 && i == own) E = tb + accB;
  }
  const double S = fmax(ta, tb);
  const double Wend = fmin(ta + accA, tb + accB);
  if (kind == 2) E = Wend;
  const bool valid = pair_ok && bad == 0;

  // second pass: the interval's start (the largest end point below E, or S; ties: a's knots < b's knots < the
  // window's end) and the segment of each drone that holds it (first i with E <= knot_i)
  double start = S, offA = 0.0, offB = 0.0;
  int segA = Ma - 1, segB = Mb - 1;
  bool foundA = false, foundB = false;
  accA = 0.0;
  accB = 0.0;
  for (int i = 0; i < Ma; ++i) {
    const double Ta = valid ? dur_a[da + i] : 1.0;
    const double prevA = accA;
    accA = accA + Ta;
    const double kA = ta + accA;
    const bool belowA = kind == 0 ? kA < E : kA <= E;
    if (i < Ma - 1 && belowA) start = fmax(start, kA);
    if (!foundA && E <= kA) { segA = i; offA = prevA; foundA = true; }
  }
  for (int i = 0; i < Mb; ++i) {
    const double Tb = valid ? dur_b[db + i] : 1.0;
    const double prevB = accB;
    accB = accB + Tb;
    const double kB = tb + accB;
    const bool belowB = kind == 2 ? kB <= E : kB < E;
    if (i < Mb - 1 && belowB) start = fmax(start, kB);
    if (!foundB && E <= kB) { segB = i; offB = prevB; foundB = true; }
  }
  const double h = E - start;
  const bool ok = valid && E <= Wend && h > 0.0;

  // e[s][j]: the difference polynomial of axis s on the interval, in u
  double e[3][D + 1];
  {
    const double la = (start - ta) - offA, lb = (start - tb) - offB;
    const double *ca = coef_a + (da + segA) * 4 * NC, *cb = coef_b + (db + segB) * 4 * NC;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      double pa[NC], pb[NC];
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        pa[j] = ok ? ca[s * NC + j] : 0.0;
        pb[j] = ok ? cb[s * NC + j] : 0.0;
      }
#pragma unroll
      for (int kk = 0; kk < D; ++kk)
#pragma unroll
        for (int j = D - 1; j >= kk; --j) {
          pa[j] = fma(la, pa[j + 1], pa[j]);
          pb[j] = fma(lb, pb[j + 1], pb[j]);
        }
      double hp = 1.0;
#pragma unroll
      for (int j = 0; j <= D; ++j) {
        e[s][j] = ok ? (pa[j] - pb[j]) * hp : 0.0;
        hp *= h;
      }
    }
  }

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

// one thread per pair: status, the window, the fold of the slots, the attained value again in the t domain
template <int NC>
__global__ void __launch_bounds__(kThreads)
cross_clearance_fold_kernel(const double *__restrict__ coef_a, const double *__restrict__ dur_a,
                            const double *__restrict__ t0_a, const int32_t *__restrict__ flags_a, int Na, int Ma,
                            const double *__restrict__ coef_b, const double *__restrict__ dur_b,
                            const double *__restrict__ t0_b, const int32_t *__restrict__ flags_b, int Nb, int Mb,
                            const double *__restrict__ work, int n_pairs, const int32_t *__restrict__ pairs,
                            double *__restrict__ min_dist, double *__restrict__ t_min, double *__restrict__ lower,
                            int32_t *__restrict__ status) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
  int st = MSNAP_ST_OK;
  double ta = 0.0, tb = 0.0, totA = 0.0, totB = 0.0;
  if (!cross_in_range(a, b, Na, Nb)) {
    st = MSNAP_ST_PAIR;
  } else {
    ta = t0_a ? t0_a[a] : 0.0;
    tb = t0_b ? t0_b[b] : 0.0;
    int bad = (isfinite(ta) && isfinite(tb)) ? 0 : 2;
    for (int i = 0; i < Ma; ++i) {
      bad |= flags_a[(size_t)a * Ma + i];
      totA = totA + dur_a[(size_t)a * Ma + i];
    }
    for (int i = 0; i < Mb; ++i) {
      bad |= flags_b[(size_t)b * Mb + i];
      totB = totB + dur_b[(size_t)b * Mb + i];
    }
    st = (bad & 2) ? MSNAP_ST_NONFINITE : ((bad & 1) ? MSNAP_ST_TIMES : MSNAP_ST_OK);
  }
  double md = nan, tm = nan, lo = nan;
  if (st == MSNAP_ST_OK) {
    const double S = fmax(ta, tb), Wend = fmin(ta + totA, tb + totB);
    if (Wend < S) {             // the drones never fly at the same time
      md = inf;
      lo = inf;
    } else {
      const int slots = Ma + Mb - 1;
      const double *w = work + (size_t)p * slots * 3;
      double best, bt, low;
      fold_slots(w, slots, best, bt, low);
      if (!(best < inf)) bt = S;      // no live slot: Wend == S, the one instant
      const double tauA = fmin(fmax(bt - ta, 0.0), totA), tauB = fmin(fmax(bt - tb, 0.0), totB);
      double xa, ya, za, xb, yb, zb;
      position_at<NC>(coef_a, dur_a, (size_t)a * Ma, Ma, tauA, xa, ya, za);
      position_at<NC>(coef_b, dur_b, (size_t)b * Mb, Mb, tauB, xb, yb, zb);
      const double dx = xa - xb, dy = ya - yb, dz = za - zb;
      md = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
      tm = bt;
      lo = fmin(sqrt(fmax(low, 0.0)), md);      // (an attained value bounds the infimum too)
    }
  }
  min_dist[p] = md;
  t_min[p] = tm;
  lower[p] = lo;
  status[p] = st;
}

struct PathSet {
  int n, m;
  const double *coef, *dur, *t0;
};

template <int NC>
int launch(msnap_ctx *ctx, const PathSet &A, const PathSet &B, int n_pairs, const int32_t *pairs, void *scratch,
           double *min_dist, double *t_min, double *lower, int32_t *status) {
  const size_t lanes = cross_clearance_lanes(n_pairs, A.m, B.m);
  const size_t segs_a = (size_t)A.n * A.m, segs_b = (size_t)B.n * B.m;
  double *work = (double *)scratch;
  int32_t *flags_a = (int32_t *)(work + 3 * lanes), *flags_b = flags_a + segs_a;
  if (segs_a) {
    hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs_a, kThreads)), dim3(kThreads), 0, ctx->stream,
                       A.coef, A.dur, segs_a, flags_a);
    MSNAP_HIP(ctx, hipGetLastError());
  }
  if (segs_b) {
    hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs_b, kThreads)), dim3(kThreads), 0, ctx->stream,
                       B.coef, B.dur, segs_b, flags_b);
    MSNAP_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL((cross_clearance_lane_kernel<NC>), dim3(blocks_of(lanes, kThreads)), dim3(kThreads), 0,
                     ctx->stream, A.coef, A.dur, A.t0, (const int32_t *)flags_a, A.n, A.m, B.coef, B.dur, B.t0,
                     (const int32_t *)flags_b, B.n, B.m, n_pairs, pairs, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((cross_clearance_fold_kernel<NC>), dim3(blocks_of(n_pairs, kThreads)), dim3(kThreads), 0,
                     ctx->stream, A.coef, A.dur, A.t0, (const int32_t *)flags_a, A.n, A.m, B.coef, B.dur, B.t0,
                     (const int32_t *)flags_b, B.n, B.m, (const double *)work, n_pairs, pairs, min_dist, t_min, lower,
                     status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_cross_clearance(msnap_ctx *ctx, const PathSet &A, const PathSet &B, int n_pairs, const int32_t *pairs,
                           double *min_dist, double *t_min, double *lower, int32_t *status) {
  const int rc = ensure(ctx, ctx->cross_clearance_work, cross_clearance_work_bytes(A.n, A.m, B.n, B.m, n_pairs));
  if (rc) return rc;
  void *scratch = ctx->cross_clearance_work.p;
  return ctx->order == 7 ? launch<8>(ctx, A, B, n_pairs, pairs, scratch, min_dist, t_min, lower, status)
                         : launch<10>(ctx, A, B, n_pairs, pairs, scratch, min_dist, t_min, lower, status);
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

static int cross_args(const msnap_ctx *ctx, int n_a, int n_seg_a, int n_b, int n_seg_b, int n_pairs,
                      std::initializer_list<const void *> ptrs) {
  if (int rc = check_cross_clearance_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs)) return rc;
  if (n_pairs == 0) return kNoWork;
  for (const void *p : ptrs)
    if (!p) return MSNAP_EINVAL;
  return MSNAP_OK;
}

int msnap_cross_clearance_device(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                                 const double *t0_a, int n_b, int n_seg_b, const double *coef_b, const double *dur_b,
                                 const double *t0_b, int n_pairs, const int32_t *pairs, double *min_dist, double *t_min,
                                 double *lower, int32_t *status) {
  MSNAP_ENTER(ctx, cross_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs,
                              {coef_a, dur_a, coef_b, dur_b, pairs, min_dist, t_min, lower, status}));
  return launch_cross_clearance(ctx, {n_a, n_seg_a, coef_a, dur_a, t0_a}, {n_b, n_seg_b, coef_b, dur_b, t0_b}, n_pairs,
                                pairs, min_dist, t_min, lower, status);
}

int msnap_cross_clearance(msnap_ctx *ctx, int n_a, int n_seg_a, const double *coef_a, const double *dur_a,
                          const double *t0_a, int n_b, int n_seg_b, const double *coef_b, const double *dur_b,
                          const double *t0_b, int n_pairs, const int32_t *pairs, double *min_dist, double *t_min,
                          double *lower, int32_t *status) {
  MSNAP_ENTER(ctx, cross_args(ctx, n_a, n_seg_a, n_b, n_seg_b, n_pairs,
                              {coef_a, dur_a, coef_b, dur_b, pairs, min_dist, t_min, lower, status}));
  const size_t b_out = (size_t)n_pairs * 8;
  return staged(ctx, {upload(coef_a, coef_bytes(ctx, n_a, n_seg_a)), upload(dur_a, dur_bytes(n_a, n_seg_a)),
                      upload(t0_a, t0_a ? (size_t)n_a * 8 : 0), upload(coef_b, coef_bytes(ctx, n_b, n_seg_b)),
                      upload(dur_b, dur_bytes(n_b, n_seg_b)), upload(t0_b, t0_b ? (size_t)n_b * 8 : 0),
                      upload(pairs, (size_t)n_pairs * 2 * 4), download(min_dist, b_out), download(t_min, b_out),
                      download(lower, b_out), download(status, (size_t)n_pairs * 4)},
                [&](const DevPtr *d) {
                  const double *da = t0_a ? (const double *)d[2] : nullptr, *db = t0_b ? (const double *)d[5] : nullptr;
                  return launch_cross_clearance(ctx, {n_a, n_seg_a, d[0], d[1], da}, {n_b, n_seg_b, d[3], d[4], db},
                                                n_pairs, d[6], d[7], d[8], d[9], d[10]);
                });
}

}  // extern "C"
