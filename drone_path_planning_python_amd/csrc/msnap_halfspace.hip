// Half-space windows of a path in continuous time: from when until when a drone is outside a half-space n.x <= b
// (include/msnap.h, "half-space windows").  The time-resolved sibling of msnap_path_extent (K12), as
// msnap_pair_conflict_window (K18) is of msnap_pair_clearance: K12's scalar polynomial n.p, K18's time-ordered walk.
//
// Lane.  One per (query, segment), a query being a (drone, plane) with a range [S, W] of its own.  The lane's interval
// is the part of its segment inside the range, [max(S, start_k), min(W, E_k)], of length h; m = -(n.p) on it in
// u in [0, 1]: K12's fused dot product of the segment's coefficients, the Taylor shift to the interval's start, the
// scaling by h^j (msnap_pair_interval.h's slots are rescaled the same way).  The walk in both directions, the node rule
// and the lane's four numbers are msnap_window.h's (first_crossing, window_lane_tail), with "outside" for its conflict
// and "inside" for its clear, against the level L = -b, which never enters the coefficients; the node step here: m at
// the node's start, middle and end and its smallest Bernstein coefficient.  A lane that has nothing to walk -- an index
// out of range, a failed drone, a plane that is not finite, a segment outside the range -- carries the zero polynomial
// and keeps the loop's shape.
// A lane cannot know that an earlier segment already holds the first exit: later segments are walked in full.
//
// Fold.  One thread per query over its segments (msnap_window.h, fold_window); then n.p at t_first and t_last in the t
// domain -- msnap_eval_flat's lookup and Horner, then (n_x x + n_y y) + n_z z with every operation rounded once, as
// K12's fold forms ext.  Status, W < S and W == S as conflict_fold_kernel.  Nothing crosses lanes but the trip count.
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_window.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;

inline size_t halfspace_lanes(int n_queries, int M) { return (size_t)n_queries * (size_t)M; }
// ctx->extent_work: per-lane results [lanes][4] doubles (a conflict: outside; clear: inside), then the flags [N M] int32
inline size_t halfspace_work_bytes(size_t lanes, size_t segs) {
  return lanes * kWindowLaneDoubles * sizeof(double) + segs * sizeof(int32_t);
}

// what a call reads: the batch, the planes [K][4] = (n, b), the queries [Q][2] = (drone, plane), the ranges ([Q] each,
// or null: 0 and the whole flight)
struct HalfspaceCall {
  int N, M, K, Q;
  const double *coef, *dur, *planes;
  const int32_t *queries;
  const double *t_from, *t_to;
  const int32_t *flags;
};

__device__ __forceinline__ bool query_in_range(const HalfspaceCall &c, int d, int pl) {
  return d >= 0 && pl >= 0 && d < c.N && pl < c.K;
}

// one lane per (query, segment): work[4 item ..] = the four times of the head, absolute
template <int NC>
__global__ void __launch_bounds__(kThreads)
halfspace_lane_kernel(const HalfspaceCall c, double t_res, double *__restrict__ work) {
  constexpr int D = NC - 1;       // degree of the positions
  const int M = c.M;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = item < (size_t)c.Q * (size_t)M;
  const size_t q = in_range ? item / (size_t)M : 0;
  const int k = (int)(item - q * (size_t)M);
  const int d0 = in_range ? c.queries[2 * q] : 0, pl0 = in_range ? c.queries[2 * q + 1] : 0;
  const bool query_ok = in_range && query_in_range(c, d0, pl0);
  const size_t d = query_ok ? (size_t)d0 : 0, pl = query_ok ? (size_t)pl0 : 0;

  // one pass over the drone's durations: its flags, the lane's segment and where it starts (the running sums of
  // msnap_eval_flat), the total; every lane makes M trips
  double acc = 0.0, start = 0.0, T = 1.0;
  int bad = 0;
  for (int i = 0; i < M; ++i) {
    const double Ti = query_ok ? c.dur[d * M + i] : 1.0;
    bad |= query_ok ? c.flags[d * M + i] : 0;
    if (i == k) { start = acc; T = Ti; }
    acc = acc + Ti;
  }
  const double E = start + T;
  const double tf = (query_ok && c.t_from) ? c.t_from[q] : 0.0, tt = (query_ok && c.t_to) ? c.t_to[q] : acc;
  const double S = fmax(tf, 0.0), Wend = fmin(tt, acc);
  const double nx = query_ok ? c.planes[4 * pl] : 0.0, ny = query_ok ? c.planes[4 * pl + 1] : 0.0,
               nz = query_ok ? c.planes[4 * pl + 2] : 0.0, b = query_ok ? c.planes[4 * pl + 3] : 0.0;
  const bool valid = query_ok && bad == 0 && isfinite(tf) && isfinite(tt) && isfinite(nx) && isfinite(ny) &&
                     isfinite(nz) && isfinite(b);
  // the part of the segment inside the range
  const double lo = fmax(S, start), hi = fmin(Wend, E), h = hi - lo;
  const bool ok = valid && h > 0.0;

  // m = -n.p on the interval, in u (zero polynomial: the lane walks nothing but keeps the loop's shape)
  double e[1][D + 1];
  {
    double(&m)[D + 1] = e[0];
    const double *cf = c.coef + (d * M + (size_t)k) * 4 * NC;
    const double la = lo - start;
#pragma unroll
    for (int j = 0; j <= D; ++j) m[j] = ok ? fma(nz, cf[2 * NC + j], fma(ny, cf[NC + j], nx * cf[j])) : 0.0;
#pragma unroll
    for (int kk = 0; kk < D; ++kk)
#pragma unroll
      for (int j = D - 1; j >= kk; --j) m[j] = fma(la, m[j + 1], m[j]);
    double hp = 1.0;
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      m[j] = ok ? -(m[j] * hp) : 0.0;
      hp *= h;
    }
  }
  const double L = -b;

  // the node step: m at the node's start, middle and end, and its smallest Bernstein coefficient on the node
  const auto values = [&](double a, double hh, bool, double &bound, double (&g)[3]) {
    constexpr BernsteinWeights<D> Wb{};
    double f[D + 1];
    shift_scale<D>(e[0], a, hh, f);
    values_at_ends_and_middle<D>(f, g);
    bound = f[0];
#pragma unroll
    for (int i = 1; i <= D; ++i) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j <= i; ++j) v = fma(Wb.w[i][j], f[j], v);
      bound = fmin(bound, v);
    }
  };
  const auto walk = [&](double &hit, double &clear) { first_crossing(values, ok, h, L, L, t_res, hit, clear); };
  double out[kWindowLaneDoubles];
  window_lane_tail(e, ok, h, lo, hi, walk, out);

  if (!in_range) return;
#pragma unroll
  for (int j = 0; j < kWindowLaneDoubles; ++j) work[kWindowLaneDoubles * item + j] = out[j];
}

struct Outputs {
  double *t_inside_until, *t_first, *v_first, *t_last, *v_last, *t_inside_from;
  int32_t *status;
};

// one thread per query: status, the range, the fold of the segments, the values in the t domain
template <int NC>
__global__ void __launch_bounds__(kThreads)
halfspace_fold_kernel(const HalfspaceCall c, const double *__restrict__ work, const Outputs o) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (size_t)c.Q) return;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const int M = c.M;
  const int d = c.queries[2 * q], pl = c.queries[2 * q + 1];
  int st = MSNAP_ST_PAIR;
  double iu = nan, tf = nan, vf = nan, tl = nan, vl = nan, ifr = nan;
  if (query_in_range(c, d, pl)) {
    const size_t d0 = (size_t)d * M;
    const double from = c.t_from ? c.t_from[q] : 0.0;
    double total = 0.0;
    int bad = 0;
    for (int i = 0; i < M; ++i) {
      bad |= c.flags[d0 + i];
      total = total + c.dur[d0 + i];
    }
    const double to = c.t_to ? c.t_to[q] : total;
    bad |= (isfinite(from) && isfinite(to)) ? 0 : 2;
    st = status_of_flags(bad);
    const double *n = c.planes + 4 * (size_t)pl;
    if (st == MSNAP_ST_OK && isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]) && isfinite(n[3])) {
#pragma clang fp contract(off)
      const double S = fmax(from, 0.0), Wend = fmin(to, total), b = n[3];
      iu = tf = inf;      // certified inside over the whole range
      tl = ifr = -inf;
      const bool instant = Wend == S;      // no lane is live: the one instant decides
      if (instant) {
        iu = tf = tl = ifr = S;
      } else if (!(Wend < S)) {
        fold_window(work + q * (size_t)M * kWindowLaneDoubles, M, iu, tf, tl, ifr);
      }
      vf = vl = -inf;
      if (tf < inf) {
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {      // (one text of the evaluation for both ends)
          double x, y, z;
          position_at<NC>(c.coef, c.dur, d0, M, e == 0 ? tf : tl, x, y, z);
          const double v = (n[0] * x + n[1] * y) + n[2] * z;
          vf = e == 0 ? v : vf;
          vl = e == 0 ? vl : v;
        }
      }
      if (instant && !(vf > b)) {      // inside at that instant: certified inside
        iu = tf = inf;
        vf = vl = tl = ifr = -inf;
      }
    }
  }
  o.t_inside_until[q] = iu;
  o.t_first[q] = tf;
  o.v_first[q] = vf;
  o.t_last[q] = tl;
  o.v_last[q] = vl;
  o.t_inside_from[q] = ifr;
  o.status[q] = st;
}

template <int NC>
int launch(msnap_ctx *ctx, HalfspaceCall c, double t_res, void *scratch, const Outputs &o) {
  const size_t lanes = halfspace_lanes(c.Q, c.M), segs = (size_t)c.N * c.M;
  double *work = (double *)scratch;
  int32_t *flags = (int32_t *)(work + kWindowLaneDoubles * lanes);
  if (segs) {
    hipLaunchKernelGGL((clearance_flags_kernel<NC>), dim3(blocks_of(segs, kThreads)), dim3(kThreads), 0, ctx->stream,
                       c.coef, c.dur, segs, flags);
    MSNAP_HIP(ctx, hipGetLastError());
  }
  c.flags = flags;
  hipLaunchKernelGGL((halfspace_lane_kernel<NC>), dim3(blocks_of(lanes, kThreads)), dim3(kThreads), 0, ctx->stream, c,
                     t_res, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL((halfspace_fold_kernel<NC>), dim3(blocks_of((size_t)c.Q, kThreads)), dim3(kThreads), 0,
                     ctx->stream, c, (const double *)work, o);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_halfspace(msnap_ctx *ctx, const HalfspaceCall &c, double t_res, const Outputs &o) {
  const int rc = ensure(ctx, ctx->extent_work, halfspace_work_bytes(halfspace_lanes(c.Q, c.M), (size_t)c.N * c.M));
  if (rc) return rc;
  void *scratch = ctx->extent_work.p;
  return ctx->order == 7 ? launch<8>(ctx, c, t_res, scratch, o) : launch<10>(ctx, c, t_res, scratch, o);
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

static int halfspace_args(const msnap_ctx *ctx, int n_drones, int n_seg, int n_planes, const double *planes,
                          int n_queries, double t_res, std::initializer_list<const void *> ptrs) {
  if (!ctx || n_drones < 0 || n_planes < 0 || n_queries < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if ((halfspace_lanes(n_queries, n_seg) + kThreads - 1) / kThreads > 0x7fffffffu) return MSNAP_EINVAL;   // grid size
  if (int rc = check_walk_grid(n_drones, n_seg)) return rc;
  if (!window_levels_valid(t_res) || (n_planes > 0 && !planes)) return MSNAP_EINVAL;
  if (n_queries == 0) return kNoWork;
  return all_required(ptrs);
}

int msnap_halfspace_window_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                  int n_planes, const double *planes, int n_queries, const int32_t *queries,
                                  const double *t_from, const double *t_to, double t_res, double *t_inside_until,
                                  double *t_first, double *v_first, double *t_last, double *v_last,
                                  double *t_inside_from, int32_t *status) {
  MSNAP_ENTER(ctx, halfspace_args(ctx, n_drones, n_seg, n_planes, planes, n_queries, t_res,
                                  {coef, dur, queries, t_inside_until, t_first, v_first, t_last, v_last, t_inside_from,
                                   status}));
  return launch_halfspace(ctx, {n_drones, n_seg, n_planes, n_queries, coef, dur, planes, queries, t_from, t_to, nullptr},
                          t_res, {t_inside_until, t_first, v_first, t_last, v_last, t_inside_from, status});
}

int msnap_halfspace_window(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, int n_planes,
                           const double *planes, int n_queries, const int32_t *queries, const double *t_from,
                           const double *t_to, double t_res, double *t_inside_until, double *t_first, double *v_first,
                           double *t_last, double *v_last, double *t_inside_from, int32_t *status) {
  MSNAP_ENTER(ctx, halfspace_args(ctx, n_drones, n_seg, n_planes, planes, n_queries, t_res,
                                  {coef, dur, queries, t_inside_until, t_first, v_first, t_last, v_last, t_inside_from,
                                   status}));
  const size_t b_out = (size_t)n_queries * 8;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(planes, (size_t)n_planes * 4 * 8), upload(queries, (size_t)n_queries * 2 * 4),
                      upload(t_from, t_from ? b_out : 0), upload(t_to, t_to ? b_out : 0),
                      download(t_inside_until, b_out), download(t_first, b_out), download(v_first, b_out),
                      download(t_last, b_out), download(v_last, b_out), download(t_inside_from, b_out),
                      download(status, (size_t)n_queries * 4)},
                [&](const DevPtr *d) {
                  const double *from = t_from ? (const double *)d[4] : nullptr,
                               *to = t_to ? (const double *)d[5] : nullptr;
                  return launch_halfspace(ctx, {n_drones, n_seg, n_planes, n_queries, d[0], d[1], d[2], d[3], from, to,
                                                nullptr},
                                          t_res, {d[6], d[7], d[8], d[9], d[10], d[11], d[12]});
                });
}

}  // extern "C"
