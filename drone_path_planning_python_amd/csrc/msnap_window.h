// What a time-ordered window certifier is made of: the walk for a first crossing, the lane tail that runs it in both
// directions, and the fold of the lanes' numbers.  Three units are built from it: msnap_conflict.hip (K18: the squared
// distance of a pair against threshold^2), msnap_mesh_conflict.hip (K19: the distance to a mesh against a threshold) and
// msnap_halfspace.hip (K20: a scalar polynomial against a level).  Each brings its lane set-up, its node step and, in the
// fold, its status, its range and the values at the two ends.  DESIGN.md §5 K18 has the method.
//
// Lane.  The forward walk visits the dyadic nodes [a, a + hh] of u in [0, 1] left to right (msnap_walk.h,
// WalkNode::advance).  Per node the unit's step gives a proven lower bound of the quantity on the node and its attained
// values g at the node's start, middle and end; then
//   1. the bound is at or above its level: the node is proven clear -- on to the next sibling;
//   2. else g(0) < L: the conflict begins at a (every earlier node was proven clear or noted as undecided): the walk ends;
//   3. else h hh <= t_res or lvl == kMaxDepth: a leaf.  g(1/2) < L or g(1) < L: the earlier of the two is the first
//      conflict found, the walk ends.  Otherwise the leaf is undecided: its a is kept if it is the earliest, and on;
//   4. else split.
// The node guard kMaxNodes ends the walk with everything from the current a on undecided.  There is no prune slack: a
// node is clear when its fp64 bound says so, and the allowance r of include/msnap.h covers the rounding of that bound.
// A lane carries two numbers per direction: the time of the conflict it found (none: +inf) and the time up to which it
// proved the path clear -- the smaller of the first undecided a and the a of the node that held the conflict (none of
// either: +inf).  The backward walk is the same body on e(1 - u); its times map back as hi - h u, and its two numbers are
// the latest conflict found and the time from which the path is proven clear (none: -inf).
//
// The loop is wave-uniform, as msnap_walk.h prescribes: every lane of the wave calls first_crossing and
// window_lane_tail, a lane that has nothing to walk among them, and a lane never leaves the loop alone.
// Internal linkage, as msnap_walk.h.
#pragma once

#include "msnap_walk.h"

namespace msnap {
namespace {

constexpr int kWindowLaneDoubles = 4;      // per lane: conflict found forward, clear until, found backward, clear from

// The walk for the first crossing from u = 0 on.  values(a, hh, active, bound, g): the unit's node step on [a, a + hh]
// (active: for a step that culls wave-uniformly).  The bound is compared with bound_level, the attained values with L:
// the same number, or a distance and its square.  h: the lane's length in seconds.  hit: the u of the crossing found
// (+inf: none); clear: the u up to which the quantity is proven at or above its level (+inf: the whole lane).
template <class Values>
__device__ __forceinline__ void first_crossing(Values &&values, bool ok, double h, double bound_level, double L,
                                               double t_res, double &hit, double &clear) {
  const double inf = __builtin_inf();
  hit = inf;
  clear = inf;
  WalkNode node;
  bool active = ok;
  while (__ballot(active) != 0) {
    const double hh = node.h(), a = node.a();
    double bound, g[3];
    values(a, hh, active, bound, g);
    const bool open = !(bound >= bound_level);                          // not proven clear (a NaN bound proves nothing)
    const bool at_start = open && g[0] < L;
    const bool leaf = h * hh <= t_res || node.lvl >= kMaxDepth;
    const bool in_mid = g[1] < L, at_end = g[2] < L;
    const bool found = at_start || (open && leaf && (in_mid || at_end));
    const bool undecided = open && !found && leaf;
    const bool split = open && !found && !leaf;
    const double at = at_start ? a : (in_mid ? fma(0.5, hh, a) : a + hh);
    const bool finished = node.advance(split, active);
    const bool guard = !finished && node.nodes >= kMaxNodes;            // nodes are left unvisited: undecided from a on
    if (active) {
      hit = found ? at : hit;
      clear = (found || undecided || guard) ? fmin(clear, a) : clear;
    }
    active = active && !(found || finished || guard);
  }
}

// e(u) -> e(1 - u): the Taylor shift by 1, then the odd coefficients negated
template <int NC>
__device__ __forceinline__ void reverse(double (&e)[NC]) {
  constexpr int D = NC - 1;
#pragma unroll
  for (int kk = 0; kk < D; ++kk)
#pragma unroll
    for (int j = D - 1; j >= kk; --j) e[j] = e[j + 1] + e[j];
#pragma unroll
  for (int j = 1; j <= D; j += 2) e[j] = -e[j];
}

// The end of a lane kernel: walk(hit, clear), the unit's call of first_crossing on the rows e, forward and then on the
// reversed rows (e is left reversed); u -> absolute time on the lane's interval [lo, hi] of length h: lo + h u forward,
// hi - h u backward, kept inside the interval; out: the lane's four numbers.
template <int R, int NC, class Walk>
__device__ __forceinline__ void window_lane_tail(double (&e)[R][NC], bool ok, double h, double lo, double hi,
                                                 Walk &&walk, double (&out)[kWindowLaneDoubles]) {
  const double inf = __builtin_inf();
#pragma unroll 1
  for (int dir = 0; dir < 2; ++dir) {
    if (dir == 1) {
#pragma unroll
      for (int s = 0; s < R; ++s) reverse(e[s]);
    }
    double hit, clear;
    walk(hit, clear);
    const double th = dir == 0 ? fmin(fma(h, hit, lo), hi) : fmax(fma(-h, hit, hi), lo);
    const double tc = dir == 0 ? fmin(fma(h, clear, lo), hi) : fmax(fma(-h, clear, hi), lo);
    const double none = dir == 0 ? inf : -inf;
    out[2 * dir] = (ok && hit < inf) ? th : none;
    out[2 * dir + 1] = (ok && clear < inf) ? tc : none;
  }
}

// Fold cnt lanes' numbers at w into the caller's initial values: the earliest and the latest conflict found, the
// earliest clear-until and the latest clear-from.  Then one set of conflict times for both directions: a time found by
// either walk counts for both ends (so that tf <= tl whatever the rounding of the two walks), and the clear times are
// clamped to them.
__device__ __forceinline__ void fold_window(const double *__restrict__ w, int cnt, double &cu, double &tf, double &tl,
                                            double &cf) {
  const double inf = __builtin_inf();
  for (int k = 0; k < cnt; ++k) {
    tf = fmin(tf, w[kWindowLaneDoubles * k]);
    cu = fmin(cu, w[kWindowLaneDoubles * k + 1]);
    tl = fmax(tl, w[kWindowLaneDoubles * k + 2]);
    cf = fmax(cf, w[kWindowLaneDoubles * k + 3]);
  }
  const double lo = fmin(tf, tl > -inf ? tl : inf), hi = fmax(tl, tf < inf ? tf : -inf);
  tf = lo;
  tl = hi;
  cu = fmin(cu, tf);
  cf = fmax(cf, tl);
}

}  // namespace
}  // namespace msnap
