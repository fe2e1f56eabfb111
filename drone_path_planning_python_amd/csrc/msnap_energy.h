// Per-segment quantities of the time allocation (K8): a segment's cost and the derivative of the optimal cost by its
// duration, from the segment's monomial coefficients.  Shared by msnap_timeopt.hip and msnap_snap_cost_grad (msnap_aux.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace msnap {

constexpr double factorial(int n) {
  double r = 1.0;
  for (int j = 2; j <= n; ++j) r *= (double)j;
  return r;
}

// int_0^T (p^(K))^2 dt of one segment, the arithmetic of snap_cost_kernel (msnap_aux.hip)
template <int K>
__device__ __forceinline__ double segment_cost(const double (&c)[2 * K], double T) {
  double f[K];                      // f[q] = (K+q)!/q! * c[K+q]
#pragma unroll
  for (int q = 0; q < K; ++q) f[q] = (factorial(K + q) / factorial(q)) * c[K + q];
  double tp[2 * K];                 // T^e, e = 1 .. 2K-1
  tp[0] = 1.0;
#pragma unroll
  for (int e = 1; e < 2 * K; ++e) tp[e] = tp[e - 1] * T;
  double acc = 0.0;
#pragma unroll
  for (int p = 0; p < K; ++p)
#pragma unroll
    for (int q = 0; q < K; ++q) acc += f[p] * f[q] * (tp[p + q + 1] / (double)(p + q + 1));
  return acc;
}

// The conserved Ostrogradsky energy of a minimiser of int (x^(K))^2 between fixed end states, at the segment's start
// (x^(q)(0) = q! c_q):  E = (K! c_K)^2 + 2 sum_{m=1..K-1} (-1)^m (K-m)! c_{K-m} (K+m)! c_{K+m}, summed in that order.
// dJ*/dT_i = -E_i when c is the solve's result (include/msnap.h, "time allocation").
template <int K>
__device__ __forceinline__ double ostrogradsky_energy(const double (&c)[2 * K]) {
  double e = (factorial(K) * factorial(K)) * (c[K] * c[K]);
#pragma unroll
  for (int m = 1; m < K; ++m) {
    const double k2 = ((m & 1) ? -2.0 : 2.0) * factorial(K - m) * factorial(K + m);
    e += (k2 * c[K - m]) * c[K + m];
  }
  return e;
}

}  // namespace msnap
