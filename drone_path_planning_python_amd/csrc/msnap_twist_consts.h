// The Hermite constants of the small-batch (twisted) solve as a table in constant memory.
//
// An fp64 constant that is no inline operand costs a lone in-order wave two s_mov_b32 issue slots wherever the
// compiler materialises it.  The twisted kernel instead fetches them with scalar loads whose flight lies under work
// that is there anyway: the sweep set (HSS / HEE / HSE of Sweep<K>::knot_geom_xp and end_side) under the input loads,
// the recovery set (CS / CE / INVFACT of recover_segment) under the merge.
//
// The table holds every DISTINCT value once, sign included: a magnitude with a negation in the expression gives the
// same number, but the compiler is free to move the negation onto the other operand or the result, and the sign bit of
// a failed drone's NaN outputs follows it (tests/test_twist_bits_gpu.py holds those bits).  The values that are inline
// operands (0.5, 1, 2, 4 and their negatives) stay literals.  Both parts are built here, at compile time, from the HermiteConsts<K> values themselves: an entry is bit for bit the literal
// it replaces (tests/c_abi/twist_consts_dump.cpp prints both; this header is plain C++17 for that reason).
#pragma once

#include "msnap_consts.h"

namespace msnap {

template <int K>
struct TwistConstMap {
  static constexpr int NU = K - 1;
  static constexpr int kMaxSweep = 5 * K * K, kMaxRec = 2 * K * K + K;   // (upper bounds; the counts are n_sweep, n_rec)
  // code of one constant: 0 = stays a literal, slot + 1 = table entry
  int hss[K][K] = {}, hee[K][K] = {}, hse[K][K] = {};   // slots of `sweep`
  int cs[K][K] = {}, ce[K][K] = {}, inv[K] = {};        // slots of `rec`
  double sweep[kMaxSweep] = {}, rec[kMaxRec] = {};
  int n_sweep = 0, n_rec = 0;

  static constexpr bool inline_operand(double v) {
    const double m = v < 0 ? -v : v;
    return m == 0.5 || m == 1.0 || m == 2.0 || m == 4.0;
  }
  static constexpr int place(double v, double *tab, int &n) {
    if (inline_operand(v)) return 0;
    int s = 0;
    while (s < n && tab[s] != v) ++s;
    if (s == n) tab[n++] = v;
    return s + 1;
  }
  constexpr TwistConstMap() {
    using C = HermiteConsts<K>;
    // exactly the entries the bodies read, in the order they read them
    for (int n = 1; n <= NU; ++n) {
      for (int m = 1; m <= n; ++m) {
        hss[n][m] = place(C::HSS[n][m], sweep, n_sweep);
        hee[n][m] = place(C::HEE[n][m], sweep, n_sweep);
      }
      hse[n][0] = place(C::HSE[n][0], sweep, n_sweep);
      hee[n][0] = place(C::HEE[n][0], sweep, n_sweep);
      for (int m = 1; m <= NU; ++m) hse[n][m] = place(C::HSE[n][m], sweep, n_sweep);
    }
    for (int n = 1; n < K; ++n) inv[n] = place(C::INVFACT[n], rec, n_rec);
    for (int m = 0; m < K; ++m) {
      ce[m][0] = place(C::CE[m][0], rec, n_rec);
      for (int n = 1; n < K; ++n) {
        cs[m][n] = place(C::CS[m][n], rec, n_rec);
        ce[m][n] = place(C::CE[m][n], rec, n_rec);
      }
    }
  }
};

template <int K>
struct TwistMapOf {
  static constexpr TwistConstMap<K> map{};
};

// the image in constant memory: sweep set and recovery set of order 7 (K = 4), then of order 9 (K = 5), each padded
// to a multiple of 8 doubles so that every set starts on a 64-byte line and is read by whole s_load_dwordx16 / x8
constexpr int twist_pad8(int n) { return (n + 7) / 8 * 8; }
template <int K>
constexpr int twist_set_words() {   // both sets of one order, padded
  return twist_pad8(TwistMapOf<K>::map.n_sweep) + twist_pad8(TwistMapOf<K>::map.n_rec);
}
template <int K>
struct TwistConstLayout {
  static_assert(K == 4 || K == 5, "the twisted solve has order 7 and order 9 instances");
  static constexpr int n_sweep = TwistMapOf<K>::map.n_sweep, n_rec = TwistMapOf<K>::map.n_rec;
  static constexpr int sweep_at = (K == 4) ? 0 : twist_set_words<4>();
  static constexpr int rec_at = sweep_at + twist_pad8(n_sweep);
  static constexpr int end = rec_at + twist_pad8(n_rec);
};
constexpr int kTwistConstWords = TwistConstLayout<5>::end;

struct alignas(64) TwistConstImage {   // (an aggregate: a device variable takes a constant initialiser, no constructor)
  double v[kTwistConstWords];
};
template <int K>
constexpr void twist_image_fill(TwistConstImage &t) {
  using L = TwistConstLayout<K>;
  for (int s = 0; s < L::n_sweep; ++s) t.v[L::sweep_at + s] = TwistMapOf<K>::map.sweep[s];
  for (int s = 0; s < L::n_rec; ++s) t.v[L::rec_at + s] = TwistMapOf<K>::map.rec[s];
}
constexpr TwistConstImage twist_const_image() {
  TwistConstImage t{};
  twist_image_fill<4>(t);
  twist_image_fill<5>(t);
  return t;
}

}  // namespace msnap
