// Prints, for the orders the small-batch solve serves, every Hermite constant its bodies read: where it comes from
// (the literal, or a slot of the constant-memory image of msnap_twist_consts.h) and the bits of both.  Plain C++17,
// no GPU runtime: tests/test_twist_consts_cpu.py compiles it with g++ and requires the two columns equal.
//   line:  <order K> <array> <n> <m> <code: 0 literal, slot + 1> <bits of HermiteConsts<K>> <bits the kernel uses>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "msnap_twist_consts.h"

using namespace msnap;

static const TwistConstImage g_image = twist_const_image();

static unsigned long long bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return (unsigned long long)b;
}

template <int K>
static void row(const char *name, int n, int m, int code, double lit, int set_at) {
  const double used = code == 0 ? lit : g_image.v[set_at + code - 1];
  std::printf("%d %s %d %d %d %016llx %016llx\n", K, name, n, m, code, bits(lit), bits(used));
}

template <int K>
static void dump() {
  using C = HermiteConsts<K>;
  using L = TwistConstLayout<K>;
  constexpr const TwistConstMap<K> &mp = TwistMapOf<K>::map;
  // layout <K> <sweep set: entries, first slot> <recovery set: entries, first slot> <doubles in the image>
  std::printf("layout %d %d %d %d %d %d\n", K, L::n_sweep, L::sweep_at, L::n_rec, L::rec_at, kTwistConstWords);
  for (int n = 1; n < K; ++n) {
    for (int m = 1; m <= n; ++m) {
      row<K>("HSS", n, m, mp.hss[n][m], C::HSS[n][m], L::sweep_at);
      row<K>("HEE", n, m, mp.hee[n][m], C::HEE[n][m], L::sweep_at);
    }
    row<K>("HSE", n, 0, mp.hse[n][0], C::HSE[n][0], L::sweep_at);
    row<K>("HEE", n, 0, mp.hee[n][0], C::HEE[n][0], L::sweep_at);
    for (int m = 1; m < K; ++m) row<K>("HSE", n, m, mp.hse[n][m], C::HSE[n][m], L::sweep_at);
    row<K>("INVFACT", n, 0, mp.inv[n], C::INVFACT[n], L::rec_at);
  }
  for (int m = 0; m < K; ++m) {
    row<K>("CE", m, 0, mp.ce[m][0], C::CE[m][0], L::rec_at);
    for (int n = 1; n < K; ++n) {
      row<K>("CS", m, n, mp.cs[m][n], C::CS[m][n], L::rec_at);
      row<K>("CE", m, n, mp.ce[m][n], C::CE[m][n], L::rec_at);
    }
  }
}

int main() {
  dump<4>();
  dump<5>();
  // the image itself, so that the test sees every slot is one of the values above and the padding is zero
  for (int i = 0; i < kTwistConstWords; ++i) std::printf("image %d %016llx\n", i, bits(g_image.v[i]));
  return 0;
}
