// Dynamic limits: certified speed / acceleration / jerk / yaw-rate peaks of the piecewise polynomials and the uniform
// retiming that meets given limits (include/msnap.h, "dynamic limits").
//
// Peaks.  One lane per (drone, segment, quantity).  Quantity q differentiates r = q + 1 times (yaw rate: r = 1 on the
// yaw axis) and forms g(u) = |p^(r)(T u)|^2 on u in [0, 1], a polynomial of degree 2 (order - r) -- the lanes all carry
// degree 2 (order - 1) so that the code is the same in every lane.  The sup of g is found by the walk of msnap_walk.h
// for a maximum: the largest Bernstein coefficient of g bounds it on a sub-interval, which is pruned when that bound is
// <= L (1 + kPruneRel) + kPruneAbs, L the largest attained value.  (This walk carries no proven bound: a lane that
// meets kMaxNodes just ends.)  The lane's best time is then evaluated in the t domain with the derivative Horner of
// msnap_eval_flat (so that eval_flat at t_peak reproduces the peak), and a second launch folds the segments of each
// drone: larger value, then earlier absolute time.
//
// Retiming.  Both orders impose homogeneous conditions (derivatives 1..khalf-1 zero at both ends, continuity inside),
// so the minimiser for the times k t is the same path run k times slower: c_j -> c_j k^-j, T -> k T.  The per-drone
// k comes from the four peaks; one workgroup folds the swarm's maximum for a common k.
#include <math.h>

#include "msnap_walk.h"
#include "msnap_wave.h"

namespace msnap {
namespace {

constexpr double kPruneRel = 1e-9;       // on g = |.|^2: 5e-10 on the norm (contract: 1e-9)
constexpr double kPruneAbs = 1e-26;      // on g: 1e-13 on the norm (contract: 1e-12)
constexpr int kThreads = kLimitsThreads;

// d[0..NC-2] = coefficients of the first, second or third derivative (r) of c, in the order of msnap_eval_flat's
// horner_derivs ((i + 1) * previous[i + 1]); the tail beyond the derivative's degree is zero
template <int NC>
__device__ __forceinline__ void derivative(const double (&c)[NC], int r, double (&d)[NC - 1]) {
#pragma clang fp contract(off)
  double d1[NC - 1], d2[NC - 2], d3[NC - 3];
#pragma unroll
  for (int i = 0; i < NC - 1; ++i) d1[i] = (double)(i + 1) * c[i + 1];
#pragma unroll
  for (int i = 0; i < NC - 2; ++i) d2[i] = (double)(i + 1) * d1[i + 1];
#pragma unroll
  for (int i = 0; i < NC - 3; ++i) d3[i] = (double)(i + 1) * d2[i + 1];
#pragma unroll
  for (int i = 0; i < NC - 1; ++i) {
    const double v2 = i < NC - 2 ? d2[i] : 0.0, v3 = i < NC - 3 ? d3[i] : 0.0;
    d[i] = r == 1 ? d1[i] : (r == 2 ? v2 : v3);
  }
}

// one lane per (drone, segment, quantity): work[2 item] = sup of g over the segment's closed range (NaN: a non-finite
// coefficient or duration; -1: a duration <= 0), work[2 item + 1] = local time of the attained value
template <int NC>
__global__ void __launch_bounds__(kThreads)
peaks_lane_kernel(const double *__restrict__ coef, const double *__restrict__ dur, int N, int M,
                  double *__restrict__ work) {
  constexpr int D = NC - 2;       // degree of the first derivative: every lane's component polynomials
  const size_t total = (size_t)N * M * 4;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = item < total;
  const size_t seg = in_range ? item >> 2 : 0;
  const int q = (int)(item & 3);
  const int r = q < 3 ? q + 1 : 1;
  const double T = in_range ? dur[seg] : 0.0;

  // component polynomials in u: e[s][j] = d_r[j] T^j (slot s: axis s of x, y, z, or the yaw axis alone)
  double e[3][D + 1];
  bool finite = isfinite(T);
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const bool used = in_range && (q < 3 || s == 0);
    const int axis = q < 3 ? s : 3;
    double c[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      c[j] = used ? coef[(seg * 4 + axis) * NC + j] : 0.0;
      finite = finite && isfinite(c[j]);
    }
    double d[NC - 1];
    derivative<NC>(c, r, d);
    double tp = 1.0;
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      e[s][j] = d[j] * tp;
      tp *= T;
    }
  }
  const bool ok = in_range && finite && T > 0.0;
  if (!ok) {      // (zero polynomials: the lane walks nothing but keeps the loop's shape)
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int j = 0; j <= D; ++j) e[s][j] = 0.0;
  }

  // branch and bound over the dyadic sub-intervals (msnap_walk.h); every lane runs the body while any lane is active
  double best = -1.0, best_u = 0.0;
  WalkNode node;
  bool active = ok;
  while (__ballot(active) != 0) {
    const double h = node.h(), a = node.a();
    double f[3][D + 1];
#pragma unroll
    for (int s = 0; s < 3; ++s) shift_scale<D>(e[s], a, h, f[s]);
    const double bound = squares_bound<false, D>(f);
    double g[3];
    squares_at_ends_and_middle<D>(f, g);
    double nb = best, nu = best_u;
    take_attained<false>(g, a, h, nb, nu);
    if (active) { best = nb; best_u = nu; }
    const bool split = bound > fma(best, kPruneRel, best) + kPruneAbs && node.lvl < kMaxDepth;
    const bool done = node.advance(split, active) || node.nodes >= kMaxNodes;
    active = active && !done;
  }

  if (!in_range) return;
  double gv, tl;
  if (!ok) {
    gv = finite ? -1.0 : __builtin_nan("");
    tl = __builtin_nan("");
  } else {
    // the attained value again, at t = T u in the t domain -- msnap_eval_flat's arithmetic
#pragma clang fp contract(off)
    tl = T * best_u;
    gv = 0.0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int axis = q < 3 ? s : 3;
      double c[NC];
#pragma unroll
      for (int j = 0; j < NC; ++j) c[j] = (q < 3 || s == 0) ? coef[(seg * 4 + axis) * NC + j] : 0.0;
      double d[NC - 1];
      derivative<NC>(c, r, d);
      double v = 0.0;
#pragma unroll
      for (int j = NC - 2; j >= 0; --j) v = v * tl + d[j];
      gv = gv + v * v;
    }
  }
  work[2 * item] = gv;
  work[2 * item + 1] = tl;
}

// one thread per drone: fold the segments (larger value, then earlier absolute time), sqrt, status
__global__ void __launch_bounds__(kThreads)
peaks_fold_kernel(const double *__restrict__ dur, const double *__restrict__ work, int N, int M,
                  double *__restrict__ peak, double *__restrict__ t_peak, int32_t *__restrict__ status) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= N) return;
  double best[4] = {-1.0, -1.0, -1.0, -1.0}, bt[4] = {0.0, 0.0, 0.0, 0.0};
  bool nonfinite = false, times = false;
  double acc = 0.0;
  for (int i = 0; i < M; ++i) {
    const size_t seg = (size_t)d * M + i;
    const double T = dur[seg];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double g = work[2 * (seg * 4 + q)];
      const double t = acc + work[2 * (seg * 4 + q) + 1];
      nonfinite = nonfinite || isnan(g);
      times = times || g < 0.0;
      if (g > best[q] || (g == best[q] && t < bt[q])) {
        best[q] = g;
        bt[q] = t;
      }
    }
    acc = acc + T;
  }
  const int st = nonfinite ? MSNAP_ST_NONFINITE : (times ? MSNAP_ST_TIMES : MSNAP_ST_OK);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    peak[(size_t)d * 4 + q] = st ? __builtin_nan("") : sqrt(best[q]);
    t_peak[(size_t)d * 4 + q] = st ? __builtin_nan("") : bt[q];
  }
  status[d] = st;
}

// per-drone factor k from the four peaks (include/msnap.h); NaN for a failed drone
__global__ void __launch_bounds__(kThreads)
retime_factor_kernel(const double *__restrict__ peak, const int32_t *__restrict__ status, int N, double v_lim,
                     double a_lim, double j_lim, double y_lim, int fit, double *__restrict__ scale) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= N) return;
  const double margin = 1.0 + 2e-9;
  const double *p = peak + (size_t)d * 4;
  double k = 0.0;
  if (v_lim > 0.0 && isfinite(v_lim)) k = fmax(k, p[0] * margin / v_lim);
  if (a_lim > 0.0 && isfinite(a_lim)) k = fmax(k, sqrt(p[1] * margin / a_lim));
  if (j_lim > 0.0 && isfinite(j_lim)) k = fmax(k, cbrt(p[2] * margin / j_lim));
  if (y_lim > 0.0 && isfinite(y_lim)) k = fmax(k, p[3] * margin / y_lim);
  if (fit) k = k > 0.0 ? k : 1.0;
  else k = fmax(k, 1.0);
  scale[d] = status[d] ? __builtin_nan("") : k;
}

// one workgroup: the largest finite factor of the call, written back to every drone that has one (max is exact: the
// order of the fold does not change the result)
__global__ void __launch_bounds__(1024)
retime_common_kernel(int N, double *__restrict__ scale) {
  __shared__ double part[1024];
  double m = __builtin_nan("");
  uniform_for<int>(threadIdx.x, N, blockDim.x, [&](int d) { m = fmax(m, scale[d]); });
  part[threadIdx.x] = m;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + w]);
    __syncthreads();
  }
  const double k = part[0];
  uniform_for<int>(threadIdx.x, N, blockDim.x, [&](int d) {
    if (!isnan(scale[d])) scale[d] = k;
  });
}

// one thread per (drone, segment, axis): c_j -> c_j r^j with r = 1/k, T -> k T; a scale that is not finite and
// positive copies the drone unchanged (in place allowed: every thread reads only what it writes)
template <int NC>
__global__ void __launch_bounds__(kThreads)
time_scale_kernel(const double *coef, const double *dur, const double *__restrict__ scale, int N, int M,
                  double *coef_out, double *dur_out) {
  const size_t total = (size_t)N * M * 4;
  const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= total) return;
  const size_t seg = item >> 2;
  const int d = (int)(seg / (size_t)M);
  const double k0 = scale[d];
  const bool use = isfinite(k0) && k0 > 0.0;
  const double k = use ? k0 : 1.0, rk = use ? 1.0 / k0 : 1.0;
  double c[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) c[j] = coef[item * NC + j];
  double p = 1.0;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    coef_out[item * NC + j] = use ? c[j] * p : c[j];
    p *= rk;
  }
  if ((item & 3) == 0) {
    const double T = dur[seg];
    dur_out[seg] = use ? T * k : T;
  }
}

}  // namespace

int launch_peaks(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, double *work, double *peak,
                 double *t_peak, int32_t *status) {
  const size_t lanes = (size_t)N * M * 4;
  if (ctx->order == 7)
    hipLaunchKernelGGL((peaks_lane_kernel<8>), dim3(blocks_of(lanes, kThreads)), dim3(kThreads), 0, ctx->stream, coef,
                       dur, N, M, work);
  else
    hipLaunchKernelGGL((peaks_lane_kernel<10>), dim3(blocks_of(lanes, kThreads)), dim3(kThreads), 0, ctx->stream, coef,
                       dur, N, M, work);
  MSNAP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(peaks_fold_kernel, dim3(blocks_of(N, kThreads)), dim3(kThreads), 0, ctx->stream, dur,
                     (const double *)work, N, M, peak, t_peak, status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_time_scale(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, const double *scale,
                      double *coef_out, double *dur_out) {
  const size_t items = (size_t)N * M * 4;
  if (ctx->order == 7)
    hipLaunchKernelGGL((time_scale_kernel<8>), dim3(blocks_of(items, kThreads)), dim3(kThreads), 0, ctx->stream, coef,
                       dur, scale, N, M, coef_out, dur_out);
  else
    hipLaunchKernelGGL((time_scale_kernel<10>), dim3(blocks_of(items, kThreads)), dim3(kThreads), 0, ctx->stream, coef,
                       dur, scale, N, M, coef_out, dur_out);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_retime(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, const double *limits, int flags,
                  double *coef_out, double *dur_out, double *scale) {
  const size_t lane = lane_doubles(N, M);
  int rc = ensure(ctx, ctx->limits_work, (lane + (size_t)N * 8 + (size_t)(N + 1) / 2) * sizeof(double));
  if (rc) return rc;
  double *work = (double *)ctx->limits_work.p;
  double *peak = work + lane, *t_peak = peak + (size_t)N * 4;
  int32_t *status = (int32_t *)(t_peak + (size_t)N * 4);
  if ((rc = launch_peaks(ctx, N, M, coef, dur, work, peak, t_peak, status))) return rc;
  hipLaunchKernelGGL(retime_factor_kernel, dim3(blocks_of(N, kThreads)), dim3(kThreads), 0, ctx->stream,
                     (const double *)peak, (const int32_t *)status, N, limits[0], limits[1], limits[2], limits[3],
                     (flags & MSNAP_RETIME_FIT) ? 1 : 0, scale);
  MSNAP_HIP(ctx, hipGetLastError());
  if (flags & MSNAP_RETIME_COMMON) {
    hipLaunchKernelGGL(retime_common_kernel, dim3(1), dim3(1024), 0, ctx->stream, N, scale);
    MSNAP_HIP(ctx, hipGetLastError());
  }
  return launch_time_scale(ctx, N, M, coef, dur, scale, coef_out, dur_out);
}

}  // namespace msnap
