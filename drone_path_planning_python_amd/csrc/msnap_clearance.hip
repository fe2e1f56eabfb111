// Pairwise clearance in continuous time: the certified minimum distance of two drones of one batch while both fly
// (include/msnap.h, "pairwise clearance").
//
// Window.  Knot times are the running sums acc = acc + T of each drone (as peaks_fold_kernel and msnap_eval_flat form
// them); the window of a pair is [0, W], W = min of the two totals.  A drone that has landed is NOT held at its end
// point: what happens after the shorter path ends is out of scope here.
//
// Intervals.  Between consecutive knots of the two drones |p_a(t) - p_b(t)|^2 is one polynomial.  The end points
// inside the window are the M - 1 interior knots of a, the M - 1 interior knots of b and W itself: 2 M - 1 slots, one
// lane per (pair, slot).  The lane's interval ends at its end point and starts at the largest end point below it, ties
// ordered a's knots < b's knots < W -- so coincident knots (a shared grid) leave the later slot empty, a slot whose end
// point lies beyond W is dead, and every live interval is found exactly once whichever drone is called a.  Both are
// found with uniform loops over the M durations (every lane of a pair loads the same addresses).
//
// Lane.  Per axis x, y, z: Taylor shift of each drone's polynomial to its local offset at the interval's start, the
// DIFFERENCE of the two (before any square: near a minimum the distance carries the rounding of the difference, not
// of the positions), scaled by h^j to u in [0, 1].  g(u) = sum of the three squares, degree 2 order.  Then the walk of
// msnap_walk.h for a minimum: the smallest Bernstein coefficient of g as a lower bound, a node pruned when
// bound >= L (1 - kPruneRel) - kPruneAbs, L the smallest attained value; the lane carries what the walk proved.
//
// Fold.  One thread per pair over its slots: smallest attained value, then earliest absolute time; smallest bound.
// The attained value is evaluated again at t_min in the t domain -- msnap_eval_flat's segment lookup and Horner, the
// formation pass's fma(dz, dz, fma(dy, dy, dx dx)) -- so that eval_flat at t_min reproduces min_dist.  Nothing crosses
// lanes but the trip count: a pair's outputs do not depend on its place in the list, and (b, a) gives the bits of
// (a, b) (the difference changes sign exactly, every later quantity is even in it).
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_walk.h"
#include "msnap_wave.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;
constexpr double kPruneRel = 2e-9;       // on g = |.|^2: 1e-9 on the distance
constexpr double kPruneAbs = 1e-18;      // on g: A^2 with A = 1e-9 m (DESIGN.md §5 K9 has the depth arithmetic)

__device__ __forceinline__ bool pair_in_range(int a, int b, int N) {
  return a >= 0 && b >= 0 && a < N && b < N && a != b;
}

// one lane per (pair, slot): work[3 item] = smallest attained g of the slot's interval (+inf: an empty or dead slot, or
// a failed pair), [3 item + 1] = its absolute time, [3 item + 2] = the proven lower bound of g there (+inf likewise)
template <int NC>
__global__ void __launch_bounds__(kThreads)
clearance_lane_kernel(const double *__restrict__ coef, const double *__restrict__ dur,
                      const int32_t *__restrict__ flags, int N, int M, int n_pairs, const int32_t *__restrict__ pairs,
                      double *__restrict__ work) {
  constexpr int D = NC - 1;       // degree of the positions
  const double inf = __builtin_inf();
  const int slots = 2 * M - 1;
  const size_t total = (size_t)n_pairs * slots;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = item < total;
  const size_t p = in_range ? item / (size_t)slots : 0;
  const int k = (int)(item - p * (size_t)slots);
  const int a0 = in_range ? pairs[2 * p] : 0, b0 = in_range ? pairs[2 * p + 1] : 0;
  const bool pair_ok = in_range && pair_in_range(a0, b0, N);
  const size_t da = pair_ok ? (size_t)a0 * M : 0, db = pair_ok ? (size_t)b0 * M : 0;
  // the slot's end point: an interior knot of a (kind 0), of b (kind 1), or the window's end (kind 2)
  const int kind = k < M - 1 ? 0 : (k < 2 * M - 2 ? 1 : 2);
  const int own = kind == 0 ? k : k - (M - 1);

  // first pass over the durations: the totals, the slot's end point, the drones' flags
  double accA = 0.0, accB = 0.0, E = 0.0;
  int bad = 0;
  for (int i = 0; i < M; ++i) {
    const double Ta = pair_ok ? dur[da + i] : 1.0, Tb = pair_ok ? dur[db + i] : 1.0;
    bad |= pair_ok ? (flags[da + i] | flags[db + i]) : 0;
    accA = accA + Ta;
    accB = accB + Tb;
    if (kind == 0 && i == own) E = accA;
    if (kind == 1 && i == own) E = accB;
  }
  const double Wend = fmin(accA, accB);
  if (kind == 2) E = Wend;
  const bool valid = pair_ok && bad == 0;

  // second pass: the interval's start (the largest end point below E; ties: a's knots < b's knots < the window's
  // end) and the segment of each drone that holds it, by msnap_eval_flat's lookup (first i with E <= acc_i)
  double start = 0.0, offA = 0.0, offB = 0.0;
  int segA = M - 1, segB = M - 1;
  bool foundA = false, foundB = false;
  accA = 0.0;
  accB = 0.0;
  for (int i = 0; i < M; ++i) {
    const double Ta = valid ? dur[da + i] : 1.0, Tb = valid ? dur[db + i] : 1.0;
    const double prevA = accA, prevB = accB;
    accA = accA + Ta;
    accB = accB + Tb;
    const bool interior = i < M - 1;
    const bool belowA = kind == 0 ? accA < E : accA <= E;
    const bool belowB = kind == 2 ? accB <= E : accB < E;
    if (interior && belowA) start = fmax(start, accA);
    if (interior && belowB) start = fmax(start, accB);
    if (!foundA && E <= accA) { segA = i; offA = prevA; foundA = true; }
    if (!foundB && E <= accB) { segB = i; offB = prevB; foundB = true; }
  }
  const double h = E - start;
  const bool ok = valid && E <= Wend && h > 0.0;

  // e[s][j]: the difference polynomial of axis s on the interval, in u
  double e[3][D + 1];
  {
    const double la = start - offA, lb = start - offB;
    const double *ca = coef + (da + segA) * 4 * NC, *cb = coef + (db + segB) * 4 * NC;
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

// one thread per pair: fold the slots (smaller value, then earlier time; smallest bound), status, the attained value
// again in the t domain
template <int NC>
__global__ void __launch_bounds__(kThreads)
clearance_fold_kernel(const double *__restrict__ coef, const double *__restrict__ dur,
                      const int32_t *__restrict__ flags, const double *__restrict__ work, int N, int M, int n_pairs,
                      const int32_t *__restrict__ pairs, double *__restrict__ min_dist, double *__restrict__ t_min,
                      double *__restrict__ lower, int32_t *__restrict__ status) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const double nan = __builtin_nan("");
  const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
  int st = MSNAP_ST_OK;
  if (!pair_in_range(a, b, N)) {
    st = MSNAP_ST_PAIR;
  } else {
    int bad = 0;
    for (int i = 0; i < M; ++i) bad |= flags[(size_t)a * M + i] | flags[(size_t)b * M + i];
    st = (bad & 2) ? MSNAP_ST_NONFINITE : ((bad & 1) ? MSNAP_ST_TIMES : MSNAP_ST_OK);
  }
  double md = nan, tm = nan, lo = nan;
  if (st == MSNAP_ST_OK) {
    const int slots = 2 * M - 1;
    const double *w = work + (size_t)p * slots * 3;
    double best, bt, low;
    fold_slots(w, slots, best, bt, low);
    double xa, ya, za, xb, yb, zb;
    position_at<NC>(coef, dur, (size_t)a * M, M, bt, xa, ya, za);
    position_at<NC>(coef, dur, (size_t)b * M, M, bt, xb, yb, zb);
    const double dx = xa - xb, dy = ya - yb, dz = za - zb;
    md = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
    tm = bt;
    lo = fmin(sqrt(fmax(low, 0.0)), md);      // (an attained value bounds the infimum too)
  }
  min_dist[p] = md;
  t_min[p] = tm;
  lower[p] = lo;
  status[p] = st;
}

template <int NC>
int launch(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int n_pairs, const int32_t *pairs,
           void *scratch, double *min_dist, double *t_min, double *lower, int32_t *status) {
  const size_t lanes = clearance_lanes(n_pairs, M), segs = (size_t)N * M;
  double *work = (double *)scratch;
  int32_t *flags = (int32_t *)(work + 3 * lanes);
  if (segs) {
    hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                       coef, dur, segs, flags);
    MSNAP_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL((clearance_lane_kernel<NC>), dim3(blocks_of(lanes, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, (const int32_t *)flags, N, M, n_pairs, pairs, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((clearance_fold_kernel<NC>), dim3(blocks_of(n_pairs, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, (const int32_t *)flags, (const double *)work, N, M, n_pairs, pairs, min_dist, t_min,
                     lower, status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_pair_clearance(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int n_pairs,
                          const int32_t *pairs, double *min_dist, double *t_min, double *lower, int32_t *status) {
  const int rc = ensure(ctx, ctx->clearance_work, clearance_work_bytes(N, M, n_pairs));
  if (rc) return rc;
  void *scratch = ctx->clearance_work.p;
  return ctx->order == 7
             ? launch<8>(ctx, N, M, coef, dur, n_pairs, pairs, scratch, min_dist, t_min, lower, status)
             : launch<10>(ctx, N, M, coef, dur, n_pairs, pairs, scratch, min_dist, t_min, lower, status);
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

// the entry points live beside their launcher, as msnap_timeopt.hip's do
static int clearance_args(const msnap_ctx *ctx, int n_drones, int n_seg, int n_pairs,
                          std::initializer_list<const void *> ptrs) {
  if (int rc = check_clearance_args(ctx, n_drones, n_seg, n_pairs)) return rc;
  if (n_pairs == 0) return kNoWork;
  for (const void *p : ptrs)
    if (!p) return MSNAP_EINVAL;
  return MSNAP_OK;
}

int msnap_pair_clearance_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                int n_pairs, const int32_t *pairs, double *min_dist, double *t_min, double *lower,
                                int32_t *status) {
  MSNAP_ENTER(ctx, clearance_args(ctx, n_drones, n_seg, n_pairs, {coef, dur, pairs, min_dist, t_min, lower, status}));
  return launch_pair_clearance(ctx, n_drones, n_seg, coef, dur, n_pairs, pairs, min_dist, t_min, lower, status);
}

int msnap_pair_clearance(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_pairs,
                         const int32_t *pairs, double *min_dist, double *t_min, double *lower, int32_t *status) {
  MSNAP_ENTER(ctx, clearance_args(ctx, n_drones, n_seg, n_pairs, {coef, dur, pairs, min_dist, t_min, lower, status}));
  const size_t b_out = (size_t)n_pairs * 8;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(pairs, (size_t)n_pairs * 2 * 4), download(min_dist, b_out), download(t_min, b_out),
                      download(lower, b_out), download(status, (size_t)n_pairs * 4)},
                [&](const DevPtr *d) {
                  return launch_pair_clearance(ctx, n_drones, n_seg, d[0], d[1], n_pairs, d[2], d[3], d[4], d[5], d[6]);
                });
}

}  // extern "C"
