// The register tile of the pairwise evaluators: 128 rows (two per lane) x NC wave-uniform columns, the running minima
// of d2 over the samples in registers.  Shared by the pairwise pass (msnap_collide.hip: collide_block folds the minima
// into row-side and column-side results) and the near-pair mask (msnap_pairs.hip: pairs_mask_kernel compares them with
// the pairs' limits), together with the distance itself, which every evaluator of the library takes from here.
// The tile's kernels run at 4 waves per SIMD, 128 VGPRs and no scratch (tools/kernel_meta.py): every construct below
// that looks roundabout records a measured regression.  gfx950, wave64.
#pragma once

#include <math.h>

#include "msnap_collide.h"

namespace msnap {

// The squared distance as include/msnap.h defines it (the differences rounded once by the caller), restated bit for
// bit by both oracles: it decides ties between equidistant formation neighbours.
__device__ __forceinline__ double pair_d2(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  return __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
}

// acc = min(acc, d2) by hand, for accumulators behind a register tie (ColChunk::wait, an opaque lane copy): there the
// compiler no longer knows the accumulator to be canonical and would put a v_max in front of every fmin -- an eighth
// instruction per pair and sample.  Neither operand can be a signalling NaN (d2 comes out of arithmetic, the
// accumulator out of earlier minima), and a quiet NaN loses, as fmin's would.
__device__ __forceinline__ void min_quiet(double &acc, double d2) {
  asm("v_min_f64 %0, %1, %0" : "+v"(acc) : "v"(d2));
}

// 6 samples of a column drone = 18 contiguous doubles in scalar registers.  The loads are issued by
// hand: next to LDS fences the compiler can no longer prove that the position arrays are not written
// and would fall back to vector loads of a uniform address.  SMEM returns out of order, so the only
// wait is lgkmcnt(0); it carries the registers as operands so that no use is scheduled above it.
typedef unsigned int u32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));
struct ColChunk {
  u32x16 a, b;
  u32x4s c;
  __device__ __forceinline__ void fetch(const double *p) {
    asm volatile("s_load_dwordx16 %0, %3, 0x0\n\ts_load_dwordx16 %1, %3, 0x40\n\ts_load_dwordx4 %2, %3, 0x80"
                 : "=&s"(a), "=&s"(b), "=&s"(c)
                 : "s"(p));
  }
  // `after` (a value the preceding arithmetic produces) pins the wait behind that arithmetic: without
  // it the compiler may sink the other register set's VALU work below this wait and lose the overlap
  __device__ __forceinline__ void wait(double &after) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a), "+s"(b), "+s"(c), "+v"(after));
  }
  // element i (a compile-time constant after unrolling) minus v, exactly rounded.  The difference is issued
  // by hand with the scalar register pair as the first operand: a lane owns two rows, and left to the
  // compiler a scalar value with two VALU users is first copied into vector registers (36 extra moves per
  // fetch).
  __device__ __forceinline__ double minus(int i, double v) const {
    const unsigned long long x =
        i < 8 ? ((unsigned long long)a[2 * i + 1] << 32) | a[2 * i]
              : i < 16 ? ((unsigned long long)b[2 * (i - 8) + 1] << 32) | b[2 * (i - 8)]
                       : ((unsigned long long)c[2 * (i - 16) + 1] << 32) | c[2 * (i - 16)];
    double d;
    asm("v_add_f64 %0, %1, -%2" : "=v"(d) : "s"(x), "v"(v));
    return d;
  }
};

// One or two samples behind the last whole chunk (91 = 15 x 6 + 1) go through a plain loop at the end; a longer
// remainder is a last chunk moved back to overlap its predecessor (a minimum does not mind seeing a sample twice),
// so that every chunk takes the wide scalar loads.  pair_tile_whole: the samples the chunks cover;
// pair_tile_chunks: the chunks of a path (S >= kSampleChunk).
__device__ __forceinline__ int pair_tile_whole(int S) {
  const int rem = S % kSampleChunk;
  return (rem == 1 || rem == 2) ? S - rem : S;
}
__device__ __forceinline__ int pair_tile_chunks(int S) { return (pair_tile_whole(S) + kSampleChunk - 1) / kSampleChunk; }

// acc[rr][jj] = min over the samples of sample part h of `sparts` of d2(row lane + 64 rr of the image prowT (pitch
// Rp), column cj + jj of pcol), for NC (even, <= kColBlock) consecutive columns of which `ncols` exist: straight-line
// code over the columns -- with a branch inside the column loop the scalar register sets cross basic blocks and the
// compiler copies every fetched value into vector registers (36 extra VALU moves per fetch) -- so a short block
// re-reads its last column instead of branching; the caller masks the columns behind ncols.
template <int NC>
__device__ __forceinline__ void pair_tile_minima(const double *__restrict__ prowT, int Rp,
                                                 const double *__restrict__ pcol, int S, int cj, int ncols, int lane,
                                                 int h, int sparts, double (&acc)[kRowsPerLane][NC]) {
#pragma clang fp contract(off)
  constexpr int CH = kSampleChunk, RPL = kRowsPerLane;
  const int stride = S * 3;
#pragma unroll
  for (int rr = 0; rr < RPL; ++rr)
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) acc[rr][jj] = INFINITY;
  const int Sw = pair_tile_whole(S);
  // sample part h of sparts takes its range of whole chunks (the last part also the plain remainder)
  const int nch = pair_tile_chunks(S);
  const int sc_begin = (int)((long long)nch * h / sparts) * CH, sc_end = (int)((long long)nch * (h + 1) / sparts) * CH;
  for (int sc = sc_begin; sc < sc_end; sc += CH) {
    const int s0 = (Sw - sc < CH) ? Sw - CH : sc;
    double row[RPL][CH][3];
    // the rows come from the transposed image [sample][xyz][row]: the 64 lanes of a load read 512
    // contiguous bytes (from the drone-major layout every lane would touch its own cache line, and with
    // several rows per lane the texture addresser, not the VALU, would set the pace: TA_BUSY 79 %)
    // (uniform base per load, lane offset in one register: no per-lane 64-bit address arithmetic)
    const double *pt = prowT + (size_t)s0 * 3 * Rp;
#pragma unroll
    for (int q = 0; q < CH; ++q)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double *pk = pt + (size_t)(3 * q + k) * Rp;
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) row[rr][q][k] = pk[lane + rr * kWave];
      }
    // one running pointer walks the block's columns; `nvalid` is made opaque per chunk so that the
    // per-column strides are not hoisted out of the sample loop into spilled scalar registers
    int nvalid = ncols;
    asm volatile("" : "+s"(nvalid));
    const double *pc = pcol + ((size_t)cj * S + s0) * 3;
    auto consume = [&](int jj, const ColChunk &k) {
#pragma unroll
      for (int q = 0; q < CH; ++q)
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
          const double dx = k.minus(3 * q + 0, row[rr][q][0]), dy = k.minus(3 * q + 1, row[rr][q][1]),
                       dz = k.minus(3 * q + 2, row[rr][q][2]);
          min_quiet(acc[rr][jj], pair_d2(dx, dy, dz));
        }
    };
    // two register sets alternate: the loads of column j+1 are issued right after the wait for
    // column j and fly during its RPL x 6 x 7 VALU operations
    ColChunk ca, cb;
    ca.fetch(pc);
#pragma unroll
    for (int jj = 0; jj < NC; jj += 2) {
      pc += (jj + 1 < nvalid) ? stride : 0;
      ca.wait(acc[RPL - 1][jj > 0 ? jj - 1 : 0]);
      cb.fetch(pc);
      consume(jj, ca);
      pc += (jj + 2 < nvalid) ? stride : 0;
      cb.wait(acc[RPL - 1][jj]);
      if (jj + 2 < NC) ca.fetch(pc);
      consume(jj + 1, cb);
    }
  }
  for (int s1 = (h == sparts - 1) ? Sw : S; s1 < S; ++s1) {
    const double *pt = prowT + (size_t)s1 * 3 * Rp;
    const double *px = pt, *py = pt + Rp, *pz = pt + 2 * (size_t)Rp;
    double rx[RPL], ry[RPL], rz[RPL];
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr) {
      rx[rr] = px[lane + rr * kWave];
      ry[rr] = py[lane + rr * kWave];
      rz[rr] = pz[lane + rr * kWave];
    }
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) {
      const double *pcs = pcol + ((size_t)(cj + (jj < ncols ? jj : ncols - 1)) * S + s1) * 3;
      const double cx = pcs[0], cy = pcs[1], cz = pcs[2];
#pragma unroll
      for (int rr = 0; rr < RPL; ++rr) {
        const double dx = cx - rx[rr], dy = cy - ry[rr], dz = cz - rz[rr];
        acc[rr][jj] = __builtin_fmin(pair_d2(dx, dy, dz), acc[rr][jj]);
      }
    }
  }
}

}  // namespace msnap
