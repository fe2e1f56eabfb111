// Near pairs of a swarm: the sorted list of every unordered pair of drones whose sampled distance is below a per-pair
// limit (include/msnap.h, "near pairs").  gfx950, wave64.
//
// Distance.  d2_ij = min over the samples of pair_d2, the pairwise pass's expression (msnap_pair_tile.h) with its
// minNum rule: a non-finite sample never wins, a drone without a finite sample keeps d2 = +inf and is in no pair.
// Limit: lim_ij = (base + (speed_i + speed_j) gap) (1 + margin), every operation rounded once (__dadd_rn / __dmul_rn:
// the library builds with -ffp-contract=on).  Kept iff sqrt(d2_ij) < lim_ij.
//
// Mask pass.  The pairwise pass's register tile itself (pair_tile_minima, msnap_pair_tile.h): a wave owns a row block
// of 128 drones (two rows per lane) and 8 column drones, whose samples arrive through scalar loads in chunks of 6 and
// are scalar operands of the 7 operations per pair and sample; the rows come from a transposed image
// [sample][xyz][row].  Only the upper triangle is walked: row block I meets the column blocks from its own first one
// on.  At the end of a tile nothing is
// folded: each of the 2 x 8 minima is compared with its pair's limit and the lane stores, per row, ONE BYTE of the
// keep-bit matrix [N][ceil(N / 64)] of 64-bit words -- byte c of a row holds the columns 8 c .. 8 c + 7, so every byte
// has exactly one writer, and every byte of a row from its own diagonal word on is written (bits of columns <= row or
// >= N are zero): the matrix needs no clearing and no atomics.
// Counts.  A wave per row: popcount of the row's words from the diagonal word on.  One workgroup scans the <= 16 384
// counts into list offsets and writes the total.
// Emit.  A wave per row: 64 words at a time, a prefix sum of the popcounts places every set bit at offset[row] + its
// rank, so the list is in ascending (i, j) order whatever max_pairs is; a pair whose position is below max_pairs is
// written, with sqrt(d2) recomputed over the samples (kept pairs are few; a distance per candidate would be N^2
// doubles).  The minimum of a set does not depend on the order it is taken in: the recomputed d2 has the mask pass's
// bits.  Every loop is wave-uniform (uniform_for, or a loop on a ballot around a predicated body).
#include <math.h>

#include "msnap_api_util.h"
#include "msnap_collide.h"
#include "msnap_pair_tile.h"
#include "msnap_wave.h"

namespace msnap {
namespace {

constexpr int kColBlocksPerRowBlock = kRowBlock / kColBlock;      // the diagonal block's column blocks
constexpr int kRowWaves = 4;                                       // rows (waves) per workgroup of the count and emit kernels
constexpr int kScanThreads = 1024;
static_assert(kCullMaxDrones <= kScanThreads * 16, "the scan walks at most 16 rows per thread");
static_assert(kColBlock == 8, "one byte of the keep-bit matrix per column block");

struct PairLimit {
  const double *speed;      // [N] or null (zeros)
  double base, gap, scale;  // scale = 1 + margin, rounded once on the host
};

// the tile's 2 x 8 minima against their limits: one byte of keep bits per row
__device__ __forceinline__ void store_keep_bits(const double (&acc)[kRowsPerLane][kColBlock], const PairLimit &pl, int N,
                                                int I, int c, int ncols, int lane, size_t pitch_bytes,
                                                unsigned char *__restrict__ mask) {
  const int cj = c * kColBlock;
  double vj[kColBlock];
#pragma unroll
  for (int jj = 0; jj < kColBlock; ++jj) vj[jj] = pl.speed ? pl.speed[min(cj + jj, N - 1)] : 0.0;
#pragma unroll
  for (int rr = 0; rr < kRowsPerLane; ++rr) {
    const int r = I * kRowBlock + rr * kWave + lane;
    const bool live = r < N;
    const double vi = pl.speed ? pl.speed[live ? r : N - 1] : 0.0;
    unsigned bits = 0;
#pragma unroll
    for (int jj = 0; jj < kColBlock; ++jj) {
      const double lim = __dmul_rn(__dadd_rn(pl.base, __dmul_rn(__dadd_rn(vi, vj[jj]), pl.gap)), pl.scale);
      const bool keep = jj < ncols && cj + jj > r && sqrt(acc[rr][jj]) < lim;      // (a NaN limit keeps nothing)
      bits |= keep ? 1u << jj : 0u;
    }
    if (live) mask[(size_t)r * pitch_bytes + c] = (unsigned char)bits;
  }
}

// grid (column blocks of the matrix's whole words, row blocks), one wave each; n_samples >= kSampleChunk
__global__ void __launch_bounds__(kWave, 4)
pairs_mask_kernel(const double *__restrict__ prowT, const double *__restrict__ pcol, int N, int S, int Rp, PairLimit pl,
                  size_t pitch_bytes, unsigned char *__restrict__ mask) {
  constexpr int RPL = kRowsPerLane, NC = kColBlock;
  const int I = blockIdx.y, c = blockIdx.x;
  if (c < I * kColBlocksPerRowBlock) return;      // left of the diagonal block: the pair belongs to the other row
  const int lane = threadIdx.x;
  const int cj = c * NC;
  const int ncols = min(N - cj, NC);
  double acc[RPL][NC];
  if (ncols <= 0) {      // the last word's bytes behind the last drone
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr)
#pragma unroll
      for (int jj = 0; jj < NC; ++jj) acc[rr][jj] = INFINITY;
    store_keep_bits(acc, pl, N, I, c, 0, lane, pitch_bytes, mask);
    return;
  }
  pair_tile_minima<NC>(prowT + (size_t)I * kRowBlock, Rp, pcol, S, cj, ncols, lane, 0, 1, acc);
  store_keep_bits(acc, pl, N, I, c, ncols, lane, pitch_bytes, mask);
}

// the same tile for paths shorter than one sample chunk: a plain loop over the drone-major positions
__global__ void __launch_bounds__(kWave)
pairs_mask_short_kernel(const double *__restrict__ pos, int N, int S, PairLimit pl, size_t pitch_bytes,
                        unsigned char *__restrict__ mask) {
#pragma clang fp contract(off)
  constexpr int RPL = kRowsPerLane, NC = kColBlock;
  const int I = blockIdx.y, c = blockIdx.x;
  if (c < I * kColBlocksPerRowBlock) return;
  const int lane = threadIdx.x;
  const int cj = c * NC;
  const int ncols = min(N - cj, NC);
  double acc[RPL][NC];
#pragma unroll
  for (int rr = 0; rr < RPL; ++rr)
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) acc[rr][jj] = INFINITY;
  for (int s = 0; s < S && ncols > 0; ++s) {
    double rx[RPL], ry[RPL], rz[RPL];
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr) {
      const double *pr = pos + ((size_t)min(I * kRowBlock + rr * kWave + lane, N - 1) * S + s) * 3;
      rx[rr] = pr[0];
      ry[rr] = pr[1];
      rz[rr] = pr[2];
    }
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) {
      const double *pcs = pos + ((size_t)(cj + (jj < ncols ? jj : ncols - 1)) * S + s) * 3;
      const double cx = pcs[0], cy = pcs[1], cz = pcs[2];
#pragma unroll
      for (int rr = 0; rr < RPL; ++rr) {
        const double dx = cx - rx[rr], dy = cy - ry[rr], dz = cz - rz[rr];
        acc[rr][jj] = __builtin_fmin(pair_d2(dx, dy, dz), acc[rr][jj]);
      }
    }
  }
  store_keep_bits(acc, pl, N, I, c, ncols > 0 ? ncols : 0, lane, pitch_bytes, mask);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// a wave per row: kept pairs of the row (its words from the diagonal word on; the words before it are never written)
__global__ void __launch_bounds__(kWave * kRowWaves)
pairs_count_kernel(const unsigned long long *__restrict__ mask, int N, int W, int32_t *__restrict__ count) {
  const int row = blockIdx.x * kRowWaves + (int)(threadIdx.x / kWave), lane = threadIdx.x % kWave;
  if (row >= N) return;
  int n = 0;
  uniform_for<int>(lane, W, kWave, [&](int w) { n += __popcll(mask[(size_t)row * W + w]); }, row / 64);
  n = wave_sum_i32(n);
  if (lane == 0) count[row] = n;
}

// one workgroup: offset[r] = kept pairs of the rows before r, *n_found = the total
__global__ void __launch_bounds__(kScanThreads)
pairs_scan_kernel(const int32_t *__restrict__ count, int N, long long *__restrict__ offset,
                  long long *__restrict__ n_found) {
  __shared__ long long s[kScanThreads];
  const int t = threadIdx.x;
  const int per = (N + kScanThreads - 1) / kScanThreads, r0 = t * per;
  long long sum = 0;
  for (int k = 0; k < per; ++k) sum += r0 + k < N ? count[r0 + k] : 0;
  s[t] = sum;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const long long v = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  long long at = s[t] - sum;
  for (int k = 0; k < per; ++k)
    if (r0 + k < N) {
      offset[r0 + k] = at;
      at += count[r0 + k];
    }
  if (t == kScanThreads - 1) *n_found = s[t];
}

// a wave per row: the row's set bits in ascending column order to their list positions
__global__ void __launch_bounds__(kWave * kRowWaves)
pairs_emit_kernel(const unsigned long long *__restrict__ mask, const int32_t *__restrict__ count,
                  const long long *__restrict__ offset, const double *__restrict__ pos, int N, int S, int W,
                  long long max_pairs, int32_t *__restrict__ pairs, double *__restrict__ pair_dist) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * kRowWaves + (int)(threadIdx.x / kWave), lane = threadIdx.x % kWave;
  if (row >= N) return;
  if (count[row] == 0) return;
  long long at = offset[row];
  if (at >= max_pairs) return;      // (the list is ascending: nothing of this row fits)
  for (int w0 = row / 64; w0 < W; w0 += kWave) {
    const int w = w0 + lane;
    unsigned long long word = w < W ? mask[(size_t)row * W + w] : 0ull;
    const int pc = __popcll(word);
    int incl = pc;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int o = __shfl_up(incl, d);
      incl += lane >= d ? o : 0;
    }
    long long p = at + (incl - pc);
    at += __shfl(incl, kWave - 1);
    // every lane runs the body while any lane has a bit left
    while (__ballot(word != 0ull) != 0) {
      const bool has = word != 0ull;
      const int j = has ? w * 64 + __builtin_ctzll(word) : row;
      word &= word - 1ull;
      const bool put = has && p < max_pairs;
      if (pair_dist && __ballot(put) != 0) {
        const double *pa = pos + (size_t)row * S * 3, *pb = pos + (size_t)(put ? j : row) * S * 3;
        double d2 = INFINITY;
        for (int s = 0; s < S; ++s) {
          const double dx = pb[3 * s] - pa[3 * s], dy = pb[3 * s + 1] - pa[3 * s + 1], dz = pb[3 * s + 2] - pa[3 * s + 2];
          d2 = __builtin_fmin(pair_d2(dx, dy, dz), d2);
        }
        if (put) pair_dist[p] = sqrt(d2);
      }
      if (put) {
        pairs[2 * p] = row;
        pairs[2 * p + 1] = j;
      }
      p += has ? 1 : 0;
    }
  }
}

int launch_near_pairs(msnap_ctx *ctx, int N, int S, const double *pos, double base, const double *speed, double gap,
                      double margin, long long max_pairs, int32_t *pairs, double *pair_dist, long long *n_found) {
  const int rc = ensure(ctx, ctx->pairs_work, near_pairs_work_bytes(N, S));
  if (rc) return rc;
  const int W = (int)near_pairs_words(N), Rp = (int)near_pairs_pitch(N), n_rb = Rp / kRowBlock;
  double *rowT = (double *)ctx->pairs_work.p;
  unsigned long long *mask = (unsigned long long *)(rowT + (size_t)Rp * S * 3);
  long long *offset = (long long *)(mask + (size_t)N * W);
  int32_t *count = (int32_t *)(offset + N);
  const PairLimit lim{speed, base, gap, 1.0 + margin};
  const size_t pitch_bytes = (size_t)W * 8;
  const dim3 tiles((unsigned)(W * 8), (unsigned)n_rb);
  if (S < kSampleChunk) {
    MSNAP_LAUNCH(ctx, pairs_mask_short_kernel, tiles, dim3(kWave), 0, pos, N, S, lim, pitch_bytes, (unsigned char *)mask);
  } else {
    if (int rt = launch_collide_transpose(ctx, pos, N, Rp, S * 3, rowT)) return rt;
    MSNAP_LAUNCH(ctx, pairs_mask_kernel, tiles, dim3(kWave), 0, (const double *)rowT, pos, N, S, Rp, lim, pitch_bytes,
                 (unsigned char *)mask);
  }
  const dim3 rows((unsigned)((N + kRowWaves - 1) / kRowWaves));
  MSNAP_LAUNCH(ctx, pairs_count_kernel, rows, dim3(kWave * kRowWaves), 0, (const unsigned long long *)mask, N, W, count);
  MSNAP_LAUNCH(ctx, pairs_scan_kernel, dim3(1), dim3(kScanThreads), 0, (const int32_t *)count, N, offset, n_found);
  if (max_pairs > 0)
    MSNAP_LAUNCH(ctx, pairs_emit_kernel, rows, dim3(kWave * kRowWaves), 0, (const unsigned long long *)mask,
                 (const int32_t *)count, (const long long *)offset, pos, N, S, W, max_pairs, pairs, pair_dist);
  return MSNAP_OK;
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

// the entry points live beside their launcher, as msnap_clearance.hip's do
static int near_pairs_args(const msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, double base, double gap,
                           double margin, long long max_pairs, const int32_t *pairs, const long long *n_found) {
  if (!ctx || !pos || !n_found || n_drones < 0 || n_samples < 1 || max_pairs < 0 || (!pairs && max_pairs > 0))
    return MSNAP_EINVAL;
  if (base != base || gap != gap || margin != margin) return MSNAP_EINVAL;
  if (n_drones > kCullMaxDrones) return MSNAP_EINVAL;
  return MSNAP_OK;
}

int msnap_formation_near_pairs_device(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, double base,
                                      const double *speed, double gap, double margin, long long max_pairs,
                                      int32_t *pairs, double *pair_dist, long long *n_found) {
  MSNAP_ENTER(ctx, near_pairs_args(ctx, n_drones, n_samples, pos, base, gap, margin, max_pairs, pairs, n_found));
  if (n_drones < 2) {
    MSNAP_HIP(ctx, hipMemsetAsync(n_found, 0, sizeof(long long), ctx->stream));
    return MSNAP_OK;
  }
  return launch_near_pairs(ctx, n_drones, n_samples, pos, base, speed, gap, margin, max_pairs, pairs, pair_dist, n_found);
}

int msnap_formation_near_pairs(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, double base,
                               const double *speed, double gap, double margin, long long max_pairs, int32_t *pairs,
                               double *pair_dist, long long *n_found) {
  MSNAP_ENTER(ctx, near_pairs_args(ctx, n_drones, n_samples, pos, base, gap, margin, max_pairs, pairs, n_found));
  if (n_drones < 2) {
    *n_found = 0;
    return MSNAP_OK;
  }
  // the list regions go in and out: what the pass does not write (rows from min(n_found, max_pairs) on) stays the caller's
  const size_t cap = (size_t)max_pairs;
  return staged(ctx, {upload(pos, (size_t)n_drones * n_samples * 3 * 8), upload(speed, speed ? (size_t)n_drones * 8 : 0),
                      Region{pairs, pairs, pairs ? cap * 2 * 4 : 0}, Region{pair_dist, pair_dist, pair_dist ? cap * 8 : 0},
                      download(n_found, sizeof(long long))},
                [&](const DevPtr *d) {
                  return launch_near_pairs(ctx, n_drones, n_samples, d[0], base, speed ? (const double *)d[1] : nullptr,
                                           gap, margin, max_pairs, pairs ? (int32_t *)d[2] : nullptr,
                                           pair_dist ? (double *)d[3] : nullptr, d[4]);
                });
}

}  // extern "C"
