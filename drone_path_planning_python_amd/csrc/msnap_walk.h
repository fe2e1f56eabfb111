// The certified walk over a path, and what its four instances share: peaks_lane_kernel (msnap_limits.hip, K7: a
// supremum), pair_lane_kernel (msnap_clearance.hip, K9 and, with CROSS, K14: a minimum between two drones),
// mesh_clearance_lane_kernel (msnap_mesh_clearance.hip, K11: a minimum against a mesh) and extent_lane_kernel
// (msnap_extent.hip, K12: a supremum in a direction, walked as the minimum of the negated polynomial).  DESIGN.md §5 K7
// has the method.  The time-ordered walks for a first crossing use WalkNode and the node helpers, not the bookkeeping
// of a minimum: msnap_window.h has that walk (first_crossing) and what else K18 (msnap_conflict.hip), K19
// (msnap_mesh_conflict.hip) and K20 (msnap_halfspace.hip) share.
//
// Walk.  Branch and bound over the dyadic sub-intervals [idx 2^-lvl, (idx + 1) 2^-lvl] of u in [0, 1].  Per node:
//   1. shift_scale: the Taylor shift of each component polynomial to the node's start, then the scaling by 2^-lvl
//      (exact), so that the node is x in [0, 1];
//   2. a bound of the quantity over the node (K7, K9: squares_bound; K11, K12: their own, from the control points);
//   3. attained values at x = 0, 1/2, 1 (values_at_ends_and_middle, squares_at_ends_and_middle), kept by take_attained:
//      the better value, then the earlier time;
//   4. split, or prune against the best attained value (the kernel's own kPruneRel, kPruneAbs), down to kMaxDepth;
//   5. WalkNode::advance: the next node, stackless -- a child, or the next sibling of the deepest ancestor that has
//      one, found with one count of trailing ones.
// The loop is wave-uniform: `while (__ballot(active) != 0)`, every lane runs the same body while any lane
// of the wave has nodes, every per-lane commit is a select under `if (active)`.  A lane must never leave it alone.
// K9, K11 and K12 also carry what the walk has proven (ProvenBound) and write one (value, time, bound) triple per lane
// (store_lane); K9 and K11 fold a row of them with fold_slots.
//
// Also here: the per-(drone, segment) flags launch and the position of a drone at an absolute time (K9, K11, K12).
// Internal linkage: each translation unit instantiates its own kernels, and names its own kThreads.
#pragma once

#include <math.h>

#include "msnap_internal.h"

namespace msnap {
namespace {

constexpr int kMaxDepth = 40;            // sub-intervals of 2^-40: below that the bound is rounding noise
constexpr int kMaxNodes = 4096;          // nodes per lane: a guard on the loop, never met by a smooth path

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

// the walk's position: node idx of level lvl is [idx 2^-lvl, (idx + 1) 2^-lvl]; nodes counts the visited ones
struct WalkNode {
  unsigned long long idx = 0;
  int lvl = 0, nodes = 0;

  __device__ __forceinline__ double h() const { return ldexp(1.0, -lvl); }
  __device__ __forceinline__ double a() const { return (double)idx * h(); }
  // to the next node: a child, or (pruned / at the depth cap) the next sibling of the deepest ancestor that has one.
  // Every lane calls it; only an active one moves.  True when there was no next node: the walk is complete.
  __device__ __forceinline__ bool advance(bool split, bool active) {
    const int up = __builtin_ctzll(~idx);           // trailing ones of idx: levels to climb (idx < 2^lvl: up <= lvl)
    const unsigned long long idx_next = split ? idx << 1 : (idx >> up) + 1;
    const int lvl_next = split ? lvl + 1 : lvl - up;
    ++nodes;
    const bool finished = !split && up == lvl;
    if (active) {
      idx = idx_next;
      lvl = lvl_next;
    }
    return finished;
  }
};

// What a walk for a minimum has proven: the smallest bound of every node it pruned or stopped at (depth cap), and of
// the root's bound if the node guard ends the walk with nodes left unvisited.
struct ProvenBound {
  double low = __builtin_inf(), root = __builtin_inf();

  // after node.advance of a node with this bound; true when the guard ends the walk
  __device__ __forceinline__ bool note(const WalkNode &node, double bound, bool split, bool finished, bool active) {
    const bool first = node.nodes == 1;
    const bool guard = !finished && node.nodes >= kMaxNodes;      // nodes are left unvisited: only the root's bound holds
    if (active) {
      root = first ? bound : root;
      low = split ? low : fmin(low, bound);
      low = guard ? fmin(low, root) : low;
    }
    return guard;
  }
};

// f(x) = e(a + hh x): Taylor shift to a, then the exact scaling by hh = 2^-lvl
template <int D>
__device__ __forceinline__ void shift_scale(const double (&e)[D + 1], double a, double hh, double (&f)[D + 1]) {
#pragma unroll
  for (int j = 0; j <= D; ++j) f[j] = e[j];
#pragma unroll
  for (int kk = 0; kk < D; ++kk)
#pragma unroll
    for (int j = D - 1; j >= kk; --j) f[j] = fma(a, f[j + 1], f[j]);
  double hp = hh;
#pragma unroll
  for (int j = 1; j <= D; ++j) {
    f[j] *= hp;
    hp *= hh;
  }
}

// f(0), f(1/2), f(1)
template <int D>
__device__ __forceinline__ void values_at_ends_and_middle(const double (&f)[D + 1], double (&v)[3]) {
  double vm = 0.0, v1 = 0.0;
#pragma unroll
  for (int j = D; j >= 0; --j) {
    vm = fma(vm, 0.5, f[j]);
    v1 = v1 + f[j];
  }
  v[0] = f[0];
  v[1] = vm;
  v[2] = v1;
}

// g = f_0^2 + f_1^2 + f_2^2 at x = 0, 1/2, 1
template <int D>
__device__ __forceinline__ void squares_at_ends_and_middle(const double (&f)[3][D + 1], double (&g)[3]) {
  g[0] = g[1] = g[2] = 0.0;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    double v[3];
    values_at_ends_and_middle<D>(f[s], v);
#pragma unroll
    for (int q = 0; q < 3; ++q) g[q] = fma(v[q], v[q], g[q]);
  }
}

// g = f_0^2 + f_1^2 + f_2^2 in the power basis, then its smallest (is_min) or largest Bernstein coefficient: a bound
// of g over x in [0, 1]
template <bool is_min, int D>
__device__ __forceinline__ double squares_bound(const double (&f)[3][D + 1]) {
  constexpr int n = 2 * D;
  constexpr BernsteinWeights<n> W{};
  double G[n + 1];
#pragma unroll
  for (int j = 0; j <= n; ++j) G[j] = 0.0;
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int i = 0; i <= D; ++i)
#pragma unroll
      for (int j = 0; j <= D; ++j) G[i + j] = fma(f[s][i], f[s][j], G[i + j]);
  double bound = G[0];
#pragma unroll
  for (int i = 1; i <= n; ++i) {
    double b = 0.0;
#pragma unroll
    for (int j = 0; j <= i; ++j) b = fma(W.w[i][j], G[j], b);
    bound = is_min ? fmin(bound, b) : fmax(bound, b);
  }
  return bound;
}

// the attained values g at the start, middle and end of the node [a, a + hh] (earlier first) against the best so far:
// the better value, then the earlier time
template <bool is_min>
__device__ __forceinline__ void take_attained(const double (&g)[3], double a, double hh, double &nb, double &nu) {
  const double u[3] = {a, fma(0.5, hh, a), a + hh};
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if ((is_min ? g[q] < nb : g[q] > nb) || (g[q] == nb && u[q] < nu)) {
      nb = g[q];
      nu = u[q];
    }
}

// a lane's result: work[3 item] = its smallest attained value (+inf: a lane without one), [3 item + 1] = the absolute
// time of it, from best_u in [0, 1] of the lane's range [start, E] of length h, [3 item + 2] = its proven lower bound
__device__ __forceinline__ void store_lane(double *__restrict__ work, size_t item, bool ok, double best, double best_u,
                                           double low, double h, double start, double E) {
  const double inf = __builtin_inf();
  const double tm = fmin(fma(h, best_u, start), E);
  work[3 * item] = ok ? best : inf;
  work[3 * item + 1] = ok ? tm : 0.0;
  work[3 * item + 2] = ok ? low : inf;
}

// fold cnt such triples at w: smaller value, then earlier time; smallest bound
__device__ __forceinline__ void fold_slots(const double *__restrict__ w, int cnt, double &best, double &bt,
                                           double &low) {
  best = __builtin_inf();
  bt = 0.0;
  low = __builtin_inf();
  for (int k = 0; k < cnt; ++k) {
    const double g = w[3 * k], t = w[3 * k + 1];
    if (g < best || (g == best && t < bt)) {
      best = g;
      bt = t;
    }
    low = fmin(low, w[3 * k + 2]);
  }
}

// one thread per (drone, segment): 2 for a non-finite coefficient (any axis) or duration, else 1 for a duration <= 0
template <int NC>
__global__ void __launch_bounds__(kClearanceThreads)
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

// the status of a path (or of a pair of them) from the OR of its segments' flags: non-finite goes before the times
__device__ __forceinline__ int status_of_flags(int bad) {
  return (bad & 2) ? MSNAP_ST_NONFINITE : ((bad & 1) ? MSNAP_ST_TIMES : MSNAP_ST_OK);
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
