// K1 -- which solve kernel instance a launch takes, and with what geometry: the decision of launch_solve_k
// (msnap_solve.hip) as plain C++.  No HIP here: a host compiler takes this header alone, and
// tests/c_abi/solve_plan_dump.cpp executes plan_solve for tests/test_solve_exact_cpu.py.  Every range, and every LDS
// and slab formula of the four families, is stated here and nowhere else; the launcher's dispatch takes its bounds
// from the same constants.
#pragma once

#include <stddef.h>
#include <stdio.h>

namespace msnap {

constexpr int kWave = 64;
constexpr int kDronesPerWave = 16;      // 16 drones x 4 axis-lanes = one wavefront
constexpr size_t kMaxLdsBytes = 160 * 1024;
constexpr int kTrPitch = 68;            // 16-byte slots per row of the output transpose image (msnap_sweep.h)

// doubles one 16-drone tile of the K1 solve keeps between its forward and backward
// sweep (1/T, G_i blocks, z_i vectors) -- LDS, or a global slab for very long paths
constexpr size_t solve_scratch_words(int khalf, int n_seg) {
  const size_t nu = (size_t)khalf - 1;
  const size_t M = (size_t)n_seg;
  const size_t knots = M > 0 ? M - 1 : 0;
  return 16 * M + 16 * nu * nu * knots + 64 * nu * knots;
}
// doubles of the LDS input stage (raw copy of the tile's waypoints and times)
constexpr size_t solve_input_words(int n_seg) { return (size_t)16 * (n_seg + 1) * 5; }
// output transpose image, NC/2 = K rows
constexpr size_t solve_tr_bytes(int khalf) { return (size_t)khalf * kTrPitch * 16; }

// ---- twist: solve_kernel_twist<K, H, M, NW>, one workgroup of NW waves per 8-drone tile ----
constexpr int kTwistDrones = 8;
constexpr int kTwistMaxSeg = 24;    // twisted variant, order 7: one instance per n_seg in 2..24
constexpr int kTwistMaxSeg9 = 12;   // order 9: 2..12
constexpr int twist_max_seg(int khalf) { return khalf == 4 ? kTwistMaxSeg : kTwistMaxSeg9; }
// knots of the longer side (the H of the instance)
constexpr int twist_half(int n_seg) { return (n_seg - 2) - (n_seg - 2) / 2; }
// inputs + z stash per wave (64 lanes x NU per knot; used by the long-path instances only, 4 x 16.5 KiB at M = 24)
constexpr size_t twist_lds_bytes(int khalf, int n_seg, int waves) {
  return ((size_t)kTwistDrones * (n_seg + 1) * 5 + (size_t)waves * 64 * (khalf - 1) * twist_half(n_seg)) * sizeof(double);
}

// ---- twin: solve_kernel_twin<K, M>, persistent waves over 8-drone tiles ----
// Output transposition image of the twin kernel: 5 rows (coefficient pairs) of kTwinTrPitch 16-byte slots.  A lane
// writes piece p at slot p * pitch + lane (8 contiguous lanes per LDS cycle: conflict-free for any pitch) and reads
// back, with store q, piece (a2, j2) = ((4q + j) / 5, (4q + j) % 5) of its own block at slot j2 * pitch + 4 * blk + a2.
// ds_read_b128 serves the lane groups {0-3, 12-15, 20-27}, ... (blocks 0, 3, 5, 6: all residues mod 4) and a slot
// covers 4 of the 64 banks, so the 16 slots of a group must differ mod 16: with pitch = 1 (mod 16) they are
// a2 + j2 + 4 * blk, distinct for every q (pitch 68 = 4 (mod 16), the one-sided kernels' choice for their flat
// read-back order, made 4 of them collide here: SQ_LDS_BANK_CONFLICT 2.0 of 9.9 M LDS cycles per launch).
constexpr int kTwinTrPitch = 65;
constexpr int kTwinTrWords = 5 * kTwinTrPitch * 2;   // in doubles
constexpr int kTwinDrones = 8;
constexpr int kTwinMaxSeg = 20;    // order 9: solve_kernel_twin for 4..20 segments.  13..20 segments do not fit the 256 registers of two
                                   // waves per SIMD (290..402 as built) and are instances for ONE wave per SIMD: the compiler keeps the
                                   // excess in accumulation registers (10..146; no scratch).  Against solve_kernel_reg<5, 20> (also one wave
                                   // per SIMD): 65 536 x 20: 136-143 against 187 us, 2^20 x 20: 1.80 against 2.32 ms = 54 % against 42 % of
                                   // the HBM peak, 8192 x 20: 19.6 against 32.1 us (profiles/r04_order9_long.txt); 13 segments tie at 2^20
constexpr int kTwinMaxSeg7 = 20;   // order 7 (19 and 20 segments: z of the first knots in LDS instead of registers)
constexpr int kTwinMinSeg = 4;     // both sides own (M - 2) / 2 >= 1 knots
constexpr int twin_max_seg(int khalf) { return khalf == 5 ? kTwinMaxSeg : kTwinMaxSeg7; }
constexpr size_t twin_lds_bytes(int khalf, int n_seg) {
  const size_t h = (size_t)(n_seg - 2) - (size_t)(n_seg - 2) / 2;     // knots of the longer side
  size_t g_words = h * (size_t)(khalf - 1) * kWave;           // h knots x NU rows x 16 (drone, side) blocks x 4 column slots
  if (khalf == 4 && n_seg >= 17) g_words += 4 * (size_t)(khalf - 1) * kWave;   // z of the first knots (kTwinZInLds)
  const size_t in_words = (size_t)kTwinDrones * (n_seg + 1) * 5;
  const size_t body = (khalf == 5 ? (size_t)kTwinTrWords : 0) + g_words;
  return (in_words > body ? in_words : body) * sizeof(double);
}

// ---- reg: solve_kernel_reg<K, kRegMaxSeg | kRegMaxSeg2>, run-time n_seg, persistent waves over 16-drone tiles ----
constexpr int kRegMaxSeg = 10;    // n_seg <= 10 takes the register-resident variant (2 waves per SIMD) ...
constexpr int kRegMaxSeg2 = 20;   // ... 11 <= n_seg <= 20 a second instance at one wave per SIMD
// input stage and transpose image share the front; behind them the G_i blocks of the interior knots
constexpr size_t reg_lds_bytes(int khalf, int n_seg) {
  const size_t nu = (size_t)khalf - 1;
  const size_t in_bytes = solve_input_words(n_seg) * sizeof(double);
  const size_t tr_bytes = solve_tr_bytes(khalf);
  return (in_bytes > tr_bytes ? in_bytes : tr_bytes) + 16 * nu * nu * (size_t)(n_seg > 2 ? n_seg - 2 : 0) * sizeof(double);
}

// ---- rolled: solve_kernel<K, GS>, any n_seg ----
// dynamic LDS of solve_kernel<K, false>: transpose image + stash + input stage.  Beyond kMaxLdsBytes the stash leaves
// LDS for a global slab of rolled_slab_bytes per workgroup (solve_kernel<K, true>, whose LDS is the image alone)
constexpr size_t rolled_lds_bytes(int khalf, int n_seg) {
  return solve_tr_bytes(khalf) + (solve_scratch_words(khalf, n_seg) + solve_input_words(n_seg)) * sizeof(double);
}
constexpr size_t rolled_slab_bytes(int khalf, int n_seg) { return solve_scratch_words(khalf, n_seg) * sizeof(double); }

// The slab is the rolled kernel's alone, and every other family's range ends where the rolled stash still fits LDS
// (the first slab lengths are 47 segments at order 7 and 34 at order 9): whether a launch uses the context's slab
// depends on the order and the segment count only, never on the batch size or the options (solve_uses_global_scratch)
constexpr int solve_max_unrolled_seg(int khalf) {
  int m = kRegMaxSeg2;
  if (twist_max_seg(khalf) > m) m = twist_max_seg(khalf);
  if (twin_max_seg(khalf) > m) m = twin_max_seg(khalf);
  return m;
}
static_assert(rolled_lds_bytes(4, solve_max_unrolled_seg(4) + 1) <= kMaxLdsBytes &&
              rolled_lds_bytes(5, solve_max_unrolled_seg(5) + 1) <= kMaxLdsBytes, "a slab below the end of the unrolled ranges");

// what the decision reads from the context: the chip's size and the launch-geometry options of msnap_set_option
struct SolveKnobs {
  int n_cu;
  int no_twist, no_twin;
  int twist_max_drones, twin_max_drones;   // 0: default
  int twist_waves;                         // 0: chosen per launch
  int solve_grid_waves;                    // 0: default
};

enum class SolveFamily { twist, twin, reg, rolled };

struct SolvePlan {
  SolveFamily family;
  // the instance: solve_kernel_twist<khalf, twist_half(seg), seg, waves>, solve_kernel_twin<khalf, seg>,
  // solve_kernel_reg<khalf, seg> (seg = kRegMaxSeg | kRegMaxSeg2), solve_kernel<khalf, slab_bytes > 0> (seg = 0)
  int khalf, seg;
  int waves;          // waves per tile = per workgroup (1 but for twist)
  int tiles;          // the kernel's tile count: 8-drone tiles for twist and twin, 16-drone tiles for reg and rolled
  int grid, block;    // workgroups, and lanes per workgroup = kWave * waves
  size_t lds_bytes;   // dynamic LDS
  size_t slab_bytes;  // of the context's global scratch slab; 0: none
};

// n_drones >= 1, n_seg >= 1 (launch_solve and the entry points' checks)
inline SolvePlan plan_solve(const SolveKnobs &k, int khalf, int n_drones, int n_seg) {
  const int K = khalf, N = n_drones, M = n_seg;
  const int ntiles = (N + kDronesPerWave - 1) / kDronesPerWave;
  SolvePlan p{};
  p.khalf = K;
  p.waves = 1;
  p.block = kWave;
  // up to one 8-drone wavefront per SIMD the two-sided kernel wins (measured crossover 8-10 k drones on 256 CUs)
  // (order 9 with an even segment count <= 10: the two-sided column-split throughput kernel already wins from one
  // 8-drone wave per CU on -- 4096 x 10: 9.2 against 11.2 us, 8192 x 10: 11.0 against 16.3 -- the straight-line
  // latency kernel below that: 1024 x 10: 7.1 against 7.4 us; tools/order_sizes.py)
  // (order 7, tools/order_sizes.py with PROBE_ORDER=7, 10 segments: 4096 drones 7.4 us against 8.6 (small-batch
  //  kernel) and 11.0 (solve_kernel_reg); 8192: 8.9 / 12.8 / 12.9; 16 384: 13.4 / - / 16.2; 32 768: 21.6 / - / 22.1;
  //  65 536: 42.0 / - / 43.4 (eager launches); 2^20: 0.70 ms against 0.634 -- beyond 256 drones per CU the 16-drone
  //  waves of solve_kernel_reg are ahead.  That holds for its two-waves-per-SIMD instance only: with 11..20 segments
  //  solve_kernel_reg<4, 20> is one wave per SIMD and the column-split kernel stays ahead at every size -- 262 144 x 20:
  //  335 against 370 us, 2^20 x 20: 1.357 against 1.407 ms (59 against 57 % of the HBM peak), 2^20 x 14: 0.941 against
  //  1.020 ms (profiles/r04_order7_long.txt))
  const bool twin_ok = (M >= kTwinMinSeg && M <= twin_max_seg(K) && !k.no_twin &&
                        (k.twin_max_drones > 0 ? N <= k.twin_max_drones
                                               : (K == 5 || N <= k.n_cu * 256 || M > kRegMaxSeg)));
  const int twist_max = k.twist_max_drones > 0 ? k.twist_max_drones : k.n_cu * (twin_ok ? 1 : 4) * kTwistDrones;
  if (M >= 2 && M <= twist_max_seg(K) && N <= twist_max && !k.no_twist) {
    // small batch: at most one wavefront per SIMD -- halve the dependent chain instead
    const int nt8 = (N + kTwistDrones - 1) / kTwistDrones;
    // waves per tile (msnap_set_option admits 0, 1, 2 and 4 only).  Measured on 256 CUs, us per step, one / two /
    // four waves (profiles/r05_twist_waves.txt): 256 x 10 (32 tiles) 4.41 / 4.31 / 4.30, 300 x 20 (38) 7.67 / 7.21 /
    // 7.08, order 9 256 x 10 6.03 / 5.78 / 5.82 -- but 1024 x 24 (128 tiles) 9.85 / 9.59 / 9.85 and 2048 x 10 (256
    // tiles) 5.71 / 5.89 / 6.06: four waves up to a quarter of the CUs' count in tiles, two up to half, one above
    const int want = k.twist_waves > 0 ? k.twist_waves : nt8 * 4 <= k.n_cu ? 4 : nt8 * 2 <= k.n_cu ? 2 : 1;
    const int nw = want == 4 || want == 2 ? want : 1;   // the instances there are
    p.family = SolveFamily::twist;
    p.seg = M;
    p.waves = nw;
    p.block = kWave * nw;
    p.lds_bytes = twist_lds_bytes(K, M, nw);
    // grid == tile count: one workgroup of nw waves per 8-drone tile (the kernel has no tile loop and no tile guard)
    p.tiles = p.grid = nt8;
    return p;
  }
  if (twin_ok) {
    // large batch, even segment count: two-sided column-split kernel
    const int nt8 = (N + kTwinDrones - 1) / kTwinDrones;
    int grid = k.n_cu * 8 * 8;
    if (k.solve_grid_waves > 0) grid = k.solve_grid_waves;
    if (grid > nt8) grid = nt8;
    p.family = SolveFamily::twin;
    p.seg = M;
    p.lds_bytes = twin_lds_bytes(K, M);
    p.tiles = nt8;
    p.grid = grid;
    return p;
  }
  if (M >= 2 && M <= kRegMaxSeg2) {   // (one segment: the rolled kernel below)
    // persistent waves (all resident at once) so that tile k+1's inputs can be prefetched during tile k
    const bool two_per_simd = (K <= 4 && M <= kRegMaxSeg);
    // Waves beyond the resident set (8 or 4 per CU) are started by the hardware as others retire, which
    // staggers the tiles' load / compute / store phases across the chip: 8x the resident set everywhere
    // (2^19..2^20 drones, order 7 M <= 10: 0.681 -> 0.647 ms, 4 tiles per wave still leave the cross-tile
    // prefetch its work; order 9 M > 10: 1.96 -> 1.55 ms; 65 536 drones, tools/reg_grid_probe.py: order 9
    // M <= 10 73.5 -> 71 us, order 7 M > 10 106 -> 101 us; the saturated launches of those two do not care).
    int grid = k.n_cu * (two_per_simd ? 8 : 4) * 8;
    if (k.solve_grid_waves > 0) grid = k.solve_grid_waves;   // msnap_set_option: tests walk several tiles per wave
    if (grid > ntiles) grid = ntiles;
    p.family = SolveFamily::reg;
    p.seg = M <= kRegMaxSeg ? kRegMaxSeg : kRegMaxSeg2;
    p.lds_bytes = reg_lds_bytes(K, M);
    p.tiles = ntiles;
    p.grid = grid;
    return p;
  }
  p.family = SolveFamily::rolled;
  p.tiles = ntiles;
  p.lds_bytes = rolled_lds_bytes(K, M);
  p.grid = ntiles;
  if (p.lds_bytes > kMaxLdsBytes) {
    // too many segments for LDS: same recurrence on a global scratch slab,
    // persistent grid so the slab stays bounded
    int grid = k.n_cu * 8;
    if (grid > ntiles) grid = ntiles;
    p.grid = grid;
    p.lds_bytes = solve_tr_bytes(K);
    p.slab_bytes = (size_t)grid * rolled_slab_bytes(K, M);
  }
  return p;
}

// the msnap_last_kernel string of a plan (tests and tools/prof_summary.py match on these)
inline int solve_plan_name(const SolvePlan &p, char *buf, size_t size) {
  switch (p.family) {
    case SolveFamily::twist:
      return snprintf(buf, size, "msnap::solve_kernel_twist<%d, %d, %d>", p.khalf, twist_half(p.seg), p.seg);
    case SolveFamily::twin:
      return snprintf(buf, size, "msnap::solve_kernel_twin<%d, %d>", p.khalf, p.seg);
    case SolveFamily::reg:
      return snprintf(buf, size, "msnap::solve_kernel_reg<%d, %d>", p.khalf, p.seg);
    default:
      return snprintf(buf, size, "msnap::solve_kernel<%d, %s>", p.khalf, p.slab_bytes > 0 ? "true" : "false");
  }
}

}  // namespace msnap
