// Cross-lane helpers of a 64-lane wave for fp64 values (the sampler, the pairwise pass, the mesh sweep, the GEMM) and
// the counted loop of every kernel whose lanes make different numbers of trips (uniform_for).
#pragma once

#include <hip/hip_runtime.h>

namespace msnap {

// v of lane (lane xor mask)
__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {
  const int lo = __shfl_xor(__double2loint(v), mask);
  const int hi = __shfl_xor(__double2hiint(v), mask);
  return __hiloint2double(hi, lo);
}

// v of lane (lane xor 4) without the LDS crossbar: the partners sit in one row of 16, four lanes apart, so two DPP row
// shifts under complementary bank masks (a bank = 4 lanes) deliver them -- lanes 0-3 and 8-11 of a row read four lanes
// up (row_shl:4, banks 0 and 2), lanes 4-7 and 12-15 four lanes down (row_shr:4, banks 1 and 3).  All 64 lanes active.
__device__ __forceinline__ int row_xor4_b32(int v) {
  const int up = __builtin_amdgcn_mov_dpp(v, 0x104, 0xF, 0x5, false);
  return __builtin_amdgcn_update_dpp(up, v, 0x114, 0xF, 0xA, false);
}
__device__ __forceinline__ double row_xor4_f64(double v) {
  const int lo = row_xor4_b32(__double2loint(v));
  const int hi = row_xor4_b32(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// fp64 min / max over the 64 lanes of a wave (every lane gets the result): four DPP stages inside
// the rows of 16 (lane xor 1, xor 2, mirror of 8, mirror of 16), two exchanges across the rows
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
template <bool MAX>
__device__ __forceinline__ double wave_minmax_f64(double v) {
  auto fold = [](double a, double b) { return MAX ? ((b > a) ? b : a) : ((b < a) ? b : a); };
  v = fold(v, dpp_f64<0xB1>(v));     // quad_perm [1,0,3,2]
  v = fold(v, dpp_f64<0x4E>(v));     // quad_perm [2,3,0,1]
  v = fold(v, dpp_f64<0x141>(v));    // row_half_mirror
  v = fold(v, dpp_f64<0x140>(v));    // row_mirror
  v = fold(v, __shfl_xor(v, 16));
  v = fold(v, __shfl_xor(v, 32));
  return v;
}
__device__ __forceinline__ double wave_min_f64(double v) { return wave_minmax_f64<false>(v); }
__device__ __forceinline__ double wave_max_f64(double v) { return wave_minmax_f64<true>(v); }
// The same butterflies with IEEE minNum / maxNum: a NaN operand is ignored, so a wave that mixes NaN and finite
// values ends with the extreme of the finite ones in EVERY lane (with the compare-and-select fold a lane holding
// NaN keeps it and its partner drops that subtree: the lanes would disagree); all-NaN stays NaN.
template <bool MAX>
__device__ __forceinline__ double wave_minmax_num_f64(double v) {
  auto fold = [](double a, double b) { return MAX ? __builtin_fmax(a, b) : __builtin_fmin(a, b); };
  v = fold(v, dpp_f64<0xB1>(v));
  v = fold(v, dpp_f64<0x4E>(v));
  v = fold(v, dpp_f64<0x141>(v));
  v = fold(v, dpp_f64<0x140>(v));
  v = fold(v, __shfl_xor(v, 16));
  v = fold(v, __shfl_xor(v, 32));
  return v;
}

// body(e) for e = base + first, base + first + stride, ... while e < count: THE counted loop of this library whenever
// the lanes' trip counts differ (lane-, thread- and grid-strided sweeps).  `count`, `stride` and `base` are
// wave-uniform, `first` < stride is the lane's offset (base: 0 for a workgroup-strided loop, the block's first element
// for a grid-stride one).  The loop variable and the trip test are WAVE-UNIFORM -- a scalar loop around a predicated
// body -- not `for (e = first; e < count; e += stride)`: a loop the lanes leave one by one ends with exec == 0, and
// the compiler put register-pressure copies of values that live across it (v_accvgpr_write_b32 of lane + 64 /
// lane + 128, solve_kernel_twin<5, 20>; the scratch spills of round 3's two-sided 16-segment instance) into that exit
// block IN FRONT of the instruction that restores exec -- they wrote no lane, the next tile's prefetch indices were
// garbage: "Memory access fault by GPU" (tools/check_exec_isa.py refuses a build with such a copy, and
// tests/test_abi.py one with a new loop of that shape).  `continue` in the body is `return`.
template <class I, class Body>
__device__ __forceinline__ void uniform_for(I first, I count, I stride, Body &&body, I base = 0) {
  for (I e0 = base; e0 < count; e0 += stride) {
    const I e = e0 + first;
    if (e < count) body(e);
  }
}

// the value of lane 0 as a compiler-visible wave-uniform value (after a wave reduction every lane holds
// the same number, but only this makes the branches and triangle loads that depend on it scalar)
__device__ __forceinline__ double uniform_f64(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

}  // namespace msnap
