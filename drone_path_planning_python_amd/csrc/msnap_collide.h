// What the pairwise pass (msnap_collide.hip) shares with the sampler (msnap_sample.hip), which can write the pass's
// row image or its boxes and sort keys, and with the C ABI (msnap_api.hip).
#pragma once

#include "msnap_internal.h"

namespace msnap {

// a kernel launch on ctx->stream followed by its error check (msnap_sample.hip, msnap_collide.hip)
#define MSNAP_LAUNCH(ctx, kernel, grid, block, lds, ...)                             \
  do {                                                                               \
    hipLaunchKernelGGL(kernel, grid, block, lds, (ctx)->stream, __VA_ARGS__);        \
    MSNAP_HIP(ctx, hipGetLastError());                                               \
  } while (0)

constexpr int kRowsPerLane = 2;   // (3 rows x 4-column blocks, 165 VGPRs, 3 waves per SIMD: 4096 x 91 in 346 us against 230)
constexpr int kRowBlock = kWave * kRowsPerLane;      // rows per row block: also the pitch granularity of the row image
constexpr int kColBlock = 8;      // column drones whose running minima a lane keeps in registers (per row)
constexpr int kSampleChunk = 6;   // samples per scalar fetch
constexpr int kKeyDrones = 4;      // drones (wavefronts) per workgroup of collide_key_kernel

constexpr int kCullMaxDrones = 16384;      // largest whole swarm that takes the broad phase (the rank count's words per lane)
constexpr int kCullMinDrones = 3072;       // smallest, by default ("collide_cull_min_drones")
constexpr int kCullGroupMaxDrones = 8192;  // largest whose group pairs are all given a list slot (524 800): the group evaluator
constexpr int kGroupCapLarge = 1 << 18;    // list slots of larger swarms (16 384 drones have 2.1 M group pairs): the group
                                           // evaluator runs while the survivors fit, the share evaluator behind it otherwise

// what the broad-phase kernels hand each other (int32 words in device memory; msnap_get_option reads kMetaTotal and
// kMetaGroups back)
enum : int {
  kMetaStart = 0,                           // [n_rb <= 128] first list position of row block I's survivors
  kMetaTotal = 128,                         // surviving shares (the list's length; zeroed by collide_key_kernel, reserved atomically by the selection)
  kMetaParts = kMetaTotal + 1,              // CullSplit lo, hi, x (the share evaluator, for the merge)
  kMetaGroups = 132,                        // surviving GROUP PAIRS (zeroed and reserved like kMetaTotal)
  kMetaWords = kMetaGroups + 2
};

// The sort key of the pairwise pass's broad phase (CollideCull, msnap_collide.hip): Morton code of the centre of a drone's path box
// on a 1 m x 1 m x 4 m lattice (paths are metres; 11 + 11 + 10 bits around the origin, clamped beyond +-1 km: a swarm
// inside one cell, or far out, sorts arbitrarily and less is culled -- the result does not depend on the order).
// A drone without a finite sample (lo > hi) gets the largest key and sorts to the end.
__device__ __forceinline__ unsigned long long spread3(unsigned long long v) {      // 21 bits -> every third bit
  v &= 0x1fffffull;
  v = (v | (v << 32)) & 0x1f00000000ffffull;
  v = (v | (v << 16)) & 0x1f0000ff0000ffull;
  v = (v | (v << 8)) & 0x100f00f00f00f00full;
  v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}
__device__ __forceinline__ unsigned drone_sort_key(const double (&lo)[3], const double (&hi)[3]) {
  unsigned long long kk = 0xffffffffull;
  if (lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2]) {
    const double cell[3] = {1.0, 1.0, 4.0}, half[3] = {1024.0, 1024.0, 512.0};
    unsigned long long q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double c = floor(0.5 * (lo[k] + hi[k]) / cell[k]) + half[k];
      c = c < 0.0 ? 0.0 : (c > 2.0 * half[k] - 1.0 ? 2.0 * half[k] - 1.0 : c);
      q[k] = (unsigned long long)c;
    }
    kk = spread3(q[0]) | (spread3(q[1]) << 1) | (spread3(q[2]) << 2);      // < 2^32 (z has 10 bits)
  }
  return (unsigned)kk;
}

// what the last broad-phase pass evaluated (device-side choice of collide_eval_kernel, restated on its counts)
bool collide_counts_by_groups(const msnap_ctx *ctx, int n_drones, int shares_surviving, int group_pairs_surviving);

// launchers (device pointers, asynchronous on ctx->stream)
// no_sym: the rows are not the slice of the columns at row_offset (one-sided evaluation, no broad phase)
int launch_formation_collide(msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                             const double *pos_rows, const double *pos_cols, double radius,
                             double *min_dist, int32_t *partner, int32_t *hit, const double *rows_t, bool no_sym);
bool formation_collide_takes_broad_phase(const msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                                         bool no_sym);
int launch_formation_collide_part(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos_all, int part,
                                  int n_parts, double *out_d2, int32_t *out_j);
int launch_formation_collide_finish(msnap_ctx *ctx, int n_drones, int n_parts, const void *parts, size_t part_stride,
                                    int row_offset, int n_rows, double radius, double *min_dist, int32_t *partner,
                                    int32_t *hit);
// the row image [E][Rp] of n_rows drone-major rows pos [n_rows][E] (collide_transpose_kernel); with `fill`, extra
// workgroups of the same launch set fill[0 .. fill_n) to -1
int launch_collide_transpose(msnap_ctx *ctx, const double *pos, int n_rows, int Rp, int E, double *out,
                             int32_t *fill = nullptr, size_t fill_n = 0);
// per drone the box [N][6] of its finite samples and its sort key [N] (collide_key_kernel)
int launch_collide_keys(msnap_ctx *ctx, const double *pos, int N, int S, double *box, unsigned *key);

}  // namespace msnap
