// From a run-time value to a compile-time one: the launchers' "one kernel instance per value in a range".
#pragma once

#include <type_traits>
#include <utility>

namespace msnap {

template <int LO, class F, int... I>
inline bool dispatch_range_at(int v, F &f, std::integer_sequence<int, I...>) {
  return ((v == LO + I ? (f(std::integral_constant<int, LO + I>{}), true) : false) || ...);
}

// calls f(std::integral_constant<int, v>{}) for the v in [LO, HI]; false, and no call, when v is outside.  f is a
// generic callable: it is instantiated for every value of the range, which is what states the set of instances
template <int LO, int HI, class F>
inline bool dispatch_range(int v, F &&f) {
  static_assert(LO <= HI, "empty range");
  return dispatch_range_at<LO>(v, f, std::make_integer_sequence<int, HI - LO + 1>{});
}

}  // namespace msnap
