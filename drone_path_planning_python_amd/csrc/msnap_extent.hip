// Path extent in continuous time: the certified support function sup_t n.p(t) of each drone's whole path in given
// directions n (include/msnap.h, "path extent").  Directions +-x, +-y, +-z give the certified
// bounding box of a path, the normals of half-spaces n.x <= b a convex geofence.
//
// Bound.  On a sub-interval of a segment the scalar polynomial q = n.p has its Bernstein coefficients as control
// points, so the largest of them bounds q from above on the whole sub-interval.  Negation is exact in fp64, so the lane
// walks the MINIMUM of m = -q with the helpers K9 and K11 use (ProvenBound, store_lane): the node's bound is the
// smallest Bernstein coefficient of m, and upper = -(what the walk proved for m).
//
// Lane.  One per (drone, segment, direction): m_j = -(n_x c_xj + n_y c_yj + n_z c_zj) T^j in u = t / T in [0, 1], then
// the walk of msnap_walk.h; the values at a node's start, middle and end are attained values.  A node is pruned when
// bound >= L - kPruneRel |L| - kPruneAbs, L the smallest attained value of m so far (b - rel |b| grows with b, so a
// node pruned against an earlier L stays pruned against the last one).  A lane that has nothing to walk -- a failed
// drone, a direction that is not finite -- carries zero polynomials and keeps the loop's shape.
//
// Fold.  One thread per (drone, direction) over the drone's segments.  Each lane's time is evaluated again in the t
// domain -- msnap_eval_flat's lookup and Horner, then (n_x x + n_y y) + n_z z with every operation rounded once -- so
// that ext is what a caller computes from msnap_eval_flat at t_ext, bit for bit: larger value, then earlier absolute
// time.  upper is the largest lane bound, raised to ext if rounding put it below.  Nothing crosses lanes but the trip
// count.
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_walk.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;
constexpr double kPruneRel = 1e-9;       // on the value n.p, relative to |best|
constexpr double kPruneAbs = 1e-9;       // in the units of n.p: what lets a support value of 0 close

__device__ __forceinline__ bool dir_finite(const double *__restrict__ n) {
  return isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]);
}

// one lane per (drone, segment, direction), item = (drone M + segment) K + direction: lanes of one segment sit side by
// side and read the same coefficients.  The result goes to slot (drone K + direction) M + segment, so that a fold
// thread reads a contiguous row: work[3 slot] = the smallest attained value of m = -n.p on the segment (+inf: a lane
// without one), [3 slot + 1] = its absolute time, [3 slot + 2] = the proven lower bound of m there
template <int NC>
__global__ void __launch_bounds__(kThreads)
extent_lane_kernel(const double *__restrict__ coef, const double *__restrict__ dur, const int32_t *__restrict__ flags,
                   int N, int M, int K, const double *__restrict__ dirs, double *__restrict__ work) {
  constexpr int D = NC - 1;       // degree of the positions
  constexpr BernsteinWeights<D> W{};
  const double inf = __builtin_inf();
  const size_t total = (size_t)N * M * K;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = item < total;
  const size_t seg = in_range ? item / (size_t)K : 0;       // drone M + segment
  const int dir = in_range ? (int)(item - seg * (size_t)K) : 0;
  const size_t d = seg / (size_t)M;
  const int k = (int)(seg - d * (size_t)M);

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
  const double nx = in_range ? dirs[3 * dir] : 0.0, ny = in_range ? dirs[3 * dir + 1] : 0.0,
               nz = in_range ? dirs[3 * dir + 2] : 0.0;
  const bool ok = in_range && bad == 0 && isfinite(nx) && isfinite(ny) && isfinite(nz);

  // e[j]: m = -n.p of the segment in u = t / T (zero polynomial: the lane walks nothing but keeps the loop's shape)
  double e[D + 1];
  {
    const double *c = coef + seg * 4 * NC;
    double hp = 1.0;
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      const double q = ok ? fma(nz, c[2 * NC + j], fma(ny, c[NC + j], nx * c[j])) : 0.0;
      e[j] = ok ? -(q * hp) : 0.0;
      hp *= T;
    }
  }

  // branch and bound over the dyadic sub-intervals (msnap_walk.h); every lane runs the body while any lane is active
  double best = inf, best_u = 0.0;
  WalkNode node;
  ProvenBound proven;
  bool active = ok;
  while (__ballot(active) != 0) {
    const double hh = node.h(), a = node.a();
    double f[D + 1], at[3];
    shift_scale<D>(e, a, hh, f);
    values_at_ends_and_middle<D>(f, at);
    // the smallest Bernstein coefficient of m on the node
    double bound = f[0];
#pragma unroll
    for (int i = 1; i <= D; ++i) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j <= i; ++j) v = fma(W.w[i][j], f[j], v);
      bound = fmin(bound, v);
    }
    double nb = best, nu = best_u;
    take_attained<true>(at, a, hh, nb, nu);
    if (active) { best = nb; best_u = nu; }
    const bool split = bound < fma(-kPruneRel, fabs(best), best) - kPruneAbs && node.lvl < kMaxDepth;
    const bool finished = node.advance(split, active);
    const bool guard = proven.note(node, bound, split, finished, active);
    active = active && !(finished || guard);
  }

  if (!in_range) return;
  store_lane(work, (d * (size_t)K + dir) * (size_t)M + k, ok, best, best_u, proven.low, T, start, E);
}

// one thread per (drone, direction): the lanes' times evaluated again in the t domain (larger value, then earlier
// time), the largest lane bound, status (written by the drone's first direction)
template <int NC>
__global__ void __launch_bounds__(kThreads)
extent_fold_kernel(const double *__restrict__ coef, const double *__restrict__ dur, const int32_t *__restrict__ flags,
                   const double *__restrict__ work, int N, int M, int K, const double *__restrict__ dirs,
                   double *__restrict__ ext, double *__restrict__ t_ext, double *__restrict__ upper,
                   int32_t *__restrict__ status) {
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= (size_t)N * K) return;
  const size_t d = item / (size_t)K;
  const int dir = (int)(item - d * (size_t)K);
  const double nan = __builtin_nan("");
  int bad = 0;
  for (int i = 0; i < M; ++i) bad |= flags[d * M + i];
  const int st = status_of_flags(bad);
  double ev = nan, et = nan, up = nan;
  const double *n = dirs + 3 * dir;
  if (st == MSNAP_ST_OK && dir_finite(n)) {
#pragma clang fp contract(off)
    const double *w = work + item * (size_t)M * 3;
    double low = __builtin_inf();
    ev = -__builtin_inf();
    et = 0.0;
    for (int k = 0; k < M; ++k) {
      const double t = w[3 * k + 1];
      double x, y, z;
      position_at<NC>(coef, dur, d * M, M, t, x, y, z);
      const double v = (n[0] * x + n[1] * y) + n[2] * z;
      if (v > ev || (v == ev && t < et)) {
        ev = v;
        et = t;
      }
      low = fmin(low, w[3 * k + 2]);
    }
    up = fmax(-low, ev);      // (an attained value bounds the supremum from below: upper is never under it)
  }
  ext[item] = ev;
  t_ext[item] = et;
  upper[item] = up;
  if (dir == 0) status[d] = st;
}

template <int NC>
int launch(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int K, const double *dirs,
           void *scratch, double *ext, double *t_ext, double *upper, int32_t *status) {
  const size_t segs = (size_t)N * M, lanes = extent_lanes(N, M, K);
  double *work = (double *)scratch;
  int32_t *flags = (int32_t *)(work + 3 * lanes);
  hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                     coef, dur, segs, flags);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((extent_lane_kernel<NC>), dim3(blocks_of(lanes, kThreads)), dim3(kThreads), 0, ctx->stream, coef,
                     dur, (const int32_t *)flags, N, M, K, dirs, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((extent_fold_kernel<NC>), dim3(blocks_of((size_t)N * K, kThreads)), dim3(kThreads), 0,
                     ctx->stream, coef, dur, (const int32_t *)flags, (const double *)work, N, M, K, dirs, ext, t_ext,
                     upper, status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

}  // namespace

int launch_path_extent(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, int K, const double *dirs,
                       double *ext, double *t_ext, double *upper, int32_t *status) {
  const int rc = ensure(ctx, ctx->extent_work, extent_work_bytes(N, M, K));
  if (rc) return rc;
  void *scratch = ctx->extent_work.p;
  return ctx->order == 7 ? launch<8>(ctx, N, M, coef, dur, K, dirs, scratch, ext, t_ext, upper, status)
                         : launch<10>(ctx, N, M, coef, dur, K, dirs, scratch, ext, t_ext, upper, status);
}

}  // namespace msnap

using namespace msnap;

extern "C" {

// the entry points live beside their launcher, as msnap_mesh_clearance.hip's do
static int path_extent_args(const msnap_ctx *ctx, int n_drones, int n_seg, int n_dirs,
                            std::initializer_list<const void *> ptrs) {
  if (!ctx || n_drones < 0 || n_dirs < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (int rc = check_extent_grid(n_drones, n_seg, n_dirs)) return rc;
  if (n_drones == 0 || n_dirs == 0) return kNoWork;
  return all_required(ptrs);
}

int msnap_path_extent_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                             int n_dirs, const double *dirs, double *ext, double *t_ext, double *upper,
                             int32_t *status) {
  MSNAP_ENTER(ctx, path_extent_args(ctx, n_drones, n_seg, n_dirs, {coef, dur, dirs, ext, t_ext, upper, status}));
  return launch_path_extent(ctx, n_drones, n_seg, coef, dur, n_dirs, dirs, ext, t_ext, upper, status);
}

int msnap_path_extent(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_dirs,
                      const double *dirs, double *ext, double *t_ext, double *upper, int32_t *status) {
  MSNAP_ENTER(ctx, path_extent_args(ctx, n_drones, n_seg, n_dirs, {coef, dur, dirs, ext, t_ext, upper, status}));
  const size_t b_out = (size_t)n_drones * n_dirs * 8;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(dirs, (size_t)n_dirs * 3 * 8), download(ext, b_out), download(t_ext, b_out),
                      download(upper, b_out), download(status, (size_t)n_drones * 4)},
                [&](const DevPtr *d) {
                  return launch_path_extent(ctx, n_drones, n_seg, d[0], d[1], n_dirs, d[2], d[3], d[4], d[5], d[6]);
                });
}

}  // extern "C"
