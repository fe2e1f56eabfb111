// What the certified walks over a path share (msnap_clearance.hip, msnap_mesh_clearance.hip): the Bernstein weights, the
// per-(drone, segment) flags launch and the position of a drone at an absolute time.  Internal linkage: each
// translation unit instantiates its own kernels.
#pragma once

#include <math.h>

#include "msnap_internal.h"

namespace msnap {
namespace {

constexpr int kThreads = kClearanceThreads;

constexpr double binom(int n, int k) {
  double r = 1.0;
  for (int j = 1; j <= k; ++j) r = r * (double)(n - k + j) / (double)j;
  return r;
}

// power basis -> Bernstein basis of degree n on [0, 1]: b_i = sum_{k <= i} C(i, k) / C(n, k) a_k
template <int n>
struct BernsteinWeights {
  double w[n + 1][n + 1];
  constexpr BernsteinWeights() : w() {
    for (int i = 0; i <= n; ++i)
      for (int k = 0; k <= i; ++k) w[i][k] = binom(i, k) / binom(n, k);
  }
};

// one thread per (drone, segment): 2 for a non-finite coefficient (any axis) or duration, else 1 for a duration <= 0
template <int NC>
__global__ void __launch_bounds__(kThreads)
clearance_flags_kernel(const double *__restrict__ coef, const double *__restrict__ dur, size_t segs,
                       int32_t *__restrict__ flags) {
  const size_t seg = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= segs) return;
  const double T = dur[seg];
  bool finite = isfinite(T);
#pragma unroll
  for (int j = 0; j < 4 * NC; ++j) finite = finite && isfinite(coef[seg * 4 * NC + j]);
  flags[seg] = !finite ? 2 : (T > 0.0 ? 0 : 1);
}

// position of one drone at absolute time t: msnap_eval_flat's lookup (first segment with t <= acc + T) and Horner
template <int NC>
__device__ __forceinline__ void position_at(const double *__restrict__ coef, const double *__restrict__ dur, size_t d0,
                                            int M, double t, double &x, double &y, double &z) {
#pragma clang fp contract(off)
  double acc = 0.0;
  int seg = -1;
  for (int i = 0; i < M; ++i) {
    const double Ti = dur[d0 + i];
    if (seg < 0) {
      if (t <= acc + Ti) seg = i;
      else acc = acc + Ti;
    }
  }
  seg = seg < 0 ? M - 1 : seg;
  const double tl = t - acc;
  const double *c = coef + (d0 + seg) * 4 * NC;
  x = y = z = 0.0;
#pragma unroll
  for (int j = NC - 1; j >= 0; --j) {
    x = x * tl + c[j];
    y = y * tl + c[NC + j];
    z = z * tl + c[2 * NC + j];
  }
}

}  // namespace
}  // namespace msnap
