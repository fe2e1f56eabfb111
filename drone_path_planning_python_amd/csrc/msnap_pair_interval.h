// What the lane kernels over a pair of drones share: pair_lane_kernel (msnap_clearance.hip, K9 and K14: the minimum
// distance) and conflict_lane_kernel (msnap_conflict.hip, K18: the first and last crossing of a level).  One text of
//   - the two path sets and the clock rules (CROSS = false: one batch on one clock, every offset the literal zero);
//   - the interval set-up of a lane: one lane per (pair, slot), Ma + Mb - 1 slots, the slot's end point E, the
//     interval's start (the largest end point below E, or S; ties a's knots < b's knots < W), the segment of each drone
//     that holds it, and the difference polynomial e[3][D + 1] of the two drones on the interval, in u in [0, 1];
//   - the distance of the pair at a common-clock time, formed in the t domain (the folds' attained values).
// msnap_clearance.hip's head has the method.  Internal linkage, as msnap_walk.h.
#pragma once

#include <math.h>

#include "msnap_walk.h"

namespace msnap {
namespace {

// n drones of m segments; t0 [n]: the drones' start times on the common clock (NULL: zeros; CROSS only); flags [n m]:
// clearance_flags_kernel's, filled in by the launcher
struct PathSet {
  int n, m;
  const double *coef, *dur, *t0;
  const int32_t *flags;
};

template <bool CROSS>
__device__ __forceinline__ bool pair_in_range(int a, int b, int Na, int Nb) {
  return a >= 0 && b >= 0 && a < Na && b < Nb && (CROSS || a != b);
}
// a drone's local time on the common clock, and back
template <bool CROSS>
__device__ __forceinline__ double on_clock(double t0, double local) { return CROSS ? t0 + local : local; }
template <bool CROSS>
__device__ __forceinline__ double local_time(double t, double t0) { return CROSS ? t - t0 : t; }

// a lane's interval [start, E] of length h; ok: the lane is live (a valid pair, E inside the window, h > 0)
struct LaneInterval {
  double start, E, h;
  bool ok;
};

// The set-up of lane `item` of A.m + B.m - 1 slots per pair: the interval and e[s][j], the difference polynomial of
// axis s on it, in u (zeros for a lane that is not live).  Every lane of a wave calls it (uniform loops).
template <int NC, bool CROSS>
__device__ __forceinline__ LaneInterval lane_interval(const PathSet &A, const PathSet &B, int n_pairs,
                                                      const int32_t *__restrict__ pairs, size_t item,
                                                      double (&e)[3][NC]) {
  constexpr int D = NC - 1;       // degree of the positions
  const int slots = A.m + B.m - 1;
  const size_t total = (size_t)n_pairs * slots;
  const bool in_range = item < total;
  const size_t p = in_range ? item / (size_t)slots : 0;
  const int k = (int)(item - p * (size_t)slots);
  const int a0 = in_range ? pairs[2 * p] : 0, b0 = in_range ? pairs[2 * p + 1] : 0;
  const bool pair_ok = in_range && pair_in_range<CROSS>(a0, b0, A.n, B.n);
  const size_t da = pair_ok ? (size_t)a0 * A.m : 0, db = pair_ok ? (size_t)b0 * B.m : 0;
  const double ta = (CROSS && pair_ok && A.t0) ? A.t0[a0] : 0.0, tb = (CROSS && pair_ok && B.t0) ? B.t0[b0] : 0.0;
  // the slot's end point: an interior knot of a (kind 0), of b (kind 1), or the window's end (kind 2)
  const int kind = k < A.m - 1 ? 0 : (k < A.m + B.m - 2 ? 1 : 2);
  const int own = kind == 0 ? k : k - (A.m - 1);

  // first pass over the durations, both drones in one loop (their loads are in flight together; a set with fewer
  // segments sits out the last rounds): the totals, the slot's end point, the drones' flags
  const int Mmax = max(A.m, B.m);
  double accA = 0.0, accB = 0.0, E = 0.0;
  int bad = (!CROSS || (isfinite(ta) && isfinite(tb))) ? 0 : 2;
  for (int i = 0; i < Mmax; ++i) {
    const bool inA = i < A.m, inB = i < B.m;
    const double Ta = (pair_ok && inA) ? A.dur[da + i] : 1.0, Tb = (pair_ok && inB) ? B.dur[db + i] : 1.0;
    bad |= (pair_ok && inA) ? A.flags[da + i] : 0;
    bad |= (pair_ok && inB) ? B.flags[db + i] : 0;
    accA = inA ? accA + Ta : accA;
    accB = inB ? accB + Tb : accB;
    if (kind == 0 && i == own) E = on_clock<CROSS>(ta, accA);
    if (kind == 1 && i == own) E = on_clock<CROSS>(tb, accB);
  }
  const double S = CROSS ? fmax(ta, tb) : 0.0;
  const double Wend = fmin(on_clock<CROSS>(ta, accA), on_clock<CROSS>(tb, accB));
  if (kind == 2) E = Wend;
  const bool valid = pair_ok && bad == 0;

  // second pass: the interval's start (the largest end point below E, or S; ties: a's knots < b's knots < the
  // window's end) and the segment of each drone that holds it, by msnap_eval_flat's lookup (first i with E <= knot_i)
  double start = S, offA = 0.0, offB = 0.0;
  int segA = A.m - 1, segB = B.m - 1;
  bool foundA = false, foundB = false;
  accA = 0.0;
  accB = 0.0;
  for (int i = 0; i < Mmax; ++i) {
    const bool inA = i < A.m, inB = i < B.m;
    const double Ta = (valid && inA) ? A.dur[da + i] : 1.0, Tb = (valid && inB) ? B.dur[db + i] : 1.0;
    const double prevA = accA, prevB = accB;
    accA = inA ? accA + Ta : accA;
    accB = inB ? accB + Tb : accB;
    const double kA = on_clock<CROSS>(ta, accA), kB = on_clock<CROSS>(tb, accB);
    const bool belowA = kind == 0 ? kA < E : kA <= E;
    const bool belowB = kind == 2 ? kB <= E : kB < E;
    if (i < A.m - 1 && belowA) start = fmax(start, kA);
    if (i < B.m - 1 && belowB) start = fmax(start, kB);
    if (inA && !foundA && E <= kA) { segA = i; offA = prevA; foundA = true; }
    if (inB && !foundB && E <= kB) { segB = i; offB = prevB; foundB = true; }
  }
  const double h = E - start;
  const bool ok = valid && E <= Wend && h > 0.0;

  // e[s][j]: the difference polynomial of axis s on the interval, in u
  {
    const double la = local_time<CROSS>(start, ta) - offA, lb = local_time<CROSS>(start, tb) - offB;
    const double *ca = A.coef + (da + segA) * 4 * NC, *cb = B.coef + (db + segB) * 4 * NC;
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
  return {start, E, h, ok};
}

// |P_a - P_b| at common-clock time t, in the t domain: msnap_eval_flat's segment lookup and Horner at the local times
// (CROSS: clamped, tau_x = min(max(fl(t - t0_x), 0), total_x)), the formation pass's fma(dz, dz, fma(dy, dy, dx dx))
template <int NC, bool CROSS>
__device__ __forceinline__ double pair_distance_at(const PathSet &A, const PathSet &B, size_t da, size_t db, double ta,
                                                   double tb, double totA, double totB, double t) {
  const double tauA = CROSS ? fmin(fmax(t - ta, 0.0), totA) : t, tauB = CROSS ? fmin(fmax(t - tb, 0.0), totB) : t;
  double xa, ya, za, xb, yb, zb;
  position_at<NC>(A.coef, A.dur, da, A.m, tauA, xa, ya, za);
  position_at<NC>(B.coef, B.dur, db, B.m, tauB, xb, yb, zb);
  const double dx = xa - xb, dy = ya - yb, dz = za - zb;
  return sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
}

// the status of a pair and, CROSS only, its offsets and the two totals (what the clamp and the window need)
template <bool CROSS>
__device__ __forceinline__ int pair_status(const PathSet &A, const PathSet &B, int a, int b, double &ta, double &tb,
                                           double &totA, double &totB) {
  ta = tb = totA = totB = 0.0;
  if (!pair_in_range<CROSS>(a, b, A.n, B.n)) return MSNAP_ST_PAIR;
  const size_t da = (size_t)a * A.m, db = (size_t)b * B.m;
  if (CROSS) {
    ta = A.t0 ? A.t0[a] : 0.0;
    tb = B.t0 ? B.t0[b] : 0.0;
  }
  int bad = (isfinite(ta) && isfinite(tb)) ? 0 : 2;
  for (int i = 0; i < A.m; ++i) {
    bad |= A.flags[da + i];
    if (CROSS) totA = totA + A.dur[da + i];
  }
  for (int i = 0; i < B.m; ++i) {
    bad |= B.flags[db + i];
    if (CROSS) totB = totB + B.dur[db + i];
  }
  return status_of_flags(bad);
}

}  // namespace
}  // namespace msnap
