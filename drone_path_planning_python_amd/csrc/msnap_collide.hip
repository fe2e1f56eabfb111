// The pairwise pass (formation collide): the span path, the exact broad phase with both its evaluators, the part and
// finish path of a pass shared between ranks, and their host launch planning.  gfx950, wave64.
#include <math.h>

#include "msnap_internal.h"
#include "msnap_collide.h"
#include "msnap_pair_tile.h"
#include "msnap_wave.h"

namespace msnap {

// ------------------------------------------------------------------------------------
// Formation pass: for every owned drone i the minimum over all other drones j and all common
// samples s of |p_i(s) - p_j(s)|.  Semantics are this repo's: no reference
// implementation exists.
//
// Arithmetic.  One lane per TWO row drones (row blocks of 128: rows lane and lane + 64); the column
// drone is wave-uniform, its samples arrive through scalar loads and are SGPR operands of the 7
// operations per pair and sample: 3 differences, d2 = pair_d2 (msnap_pair_tile.h) -- the definition
// of include/msnap.h, restated bit for bit by both oracles, which is what decides ties between
// equidistant formation neighbours -- and the minimum.
// The running minima of a block of 8 columns stay in registers over all samples.  A scalar load has
// only an all-or-nothing wait, so a wave has ONE column fetch (6 samples, 2 x 42 operations) in
// flight while it computes the previous one; the other waves of the SIMD (4 fit) cover the rest of
// the latency.  The rows are read from a transposed image [sample][xyz][row] written once per call
// (coalesced 512-byte loads; drone-major row loads would saturate the texture addresser).
//
// Work.  Columns that are also rows of this call (a single GPU: all of them; a shard: its own
// 1/G) are evaluated ONCE per unordered pair: row block I meets the own-range columns from its
// own first column on -- one-sidedly inside its diagonal block, two-sidedly behind it: d2 is
// bitwise symmetric, so after such a block the per-column minima over the 128 rows (through a
// per-wave LDS image) are stored as partial results of the COLUMN drones.  The (row block,
// column) units of the whole launch form one line -- row block after row block, the columns each
// still has to meet -- and every wave takes an equal contiguous share of it: the waves finish
// together, no SIMD idles while another still has tiles queued (a triangular grid of whole tiles
// leaves 2.03 tiles per wave: a third of the chip waits for the rest).  A merge kernel takes the
// minimum over a drone's row-side shares and column-side row blocks (lowest partner index wins
// ties on both sides).
// ------------------------------------------------------------------------------------

struct CollideGeom {
  int R, ro, Cn, S;         // rows, global index of row 0, columns, samples
  int Rp;                   // rows of the transposed row image (R rounded up to whole row blocks)
  int os, oe;               // own range: the columns [os, oe) that are this call's rows (os == oe: none)
  int sym;                  // own-range pairs evaluated once
  int n_rb;                 // row blocks
  int upw;                  // (row block, column) units per share
  int upw_tail;             // units per share behind `split` (smaller shares even out the end of the launch)
  long long split;          // first unit of the tail shares (a multiple of upw)
  int sparts;               // sample parts: a share of the line is taken by `sparts` waves, each a range of chunks
  long long total;          // units of the whole line
  // The launch walks the units [u_lo, u_lo + u_n) of the line, cut into its own shares (`split` is relative to
  // u_lo); they touch the row blocks I_lo .. I_hi.  A whole pass: 0, total, 0, n_rb - 1.  One rank's part of a
  // pass over the whole swarm (msnap_formation_collide_part, `part` = 1): a contiguous 1/P of the line; the
  // transposed row image and the partial buffers are indexed relative to I_lo, and the merge writes the squared
  // minimum of EVERY drone (+inf / -1 where this part met none of its pairs) instead of distances.
  long long u_lo, u_n;
  int I_lo, I_hi;
  int part;
};

// units of the row blocks before I: without the own-range shortcut every row block meets all Cn columns;
// with it row block I skips the own-range columns before its own first one
__device__ __host__ __forceinline__ long long collide_ustart(const CollideGeom &g, int I) {
  return g.sym ? (long long)I * g.Cn - (long long)kRowBlock * I * (I - 1) / 2 : (long long)I * g.Cn;
}

// share w covers the units [collide_share_begin(w), collide_share_begin(w + 1)) of the line
__device__ __host__ __forceinline__ long long collide_share_begin(const CollideGeom &g, long long w) {
  const long long w1 = g.split / g.upw;                  // shares of the head
  const long long u = w <= w1 ? w * g.upw : g.split + (w - w1) * g.upw_tail;
  return g.u_lo + (u < g.u_n ? u : g.u_n);
}
__device__ __host__ __forceinline__ long long collide_share_of(const CollideGeom &g, long long u) {   // u: a unit of the launch
  const long long ul = u - g.u_lo;
  return ul < g.split ? ul / g.upw : g.split / g.upw + (ul - g.split) / g.upw_tail;
}

// What a lane carries through a share: its kRowsPerLane rows (lane, lane + 64, ...)
struct RowSet {
  bool live[kRowsPerLane];       // row exists (rows past the batch end replay row R - 1 and must not win)
  int grow[kRowsPerLane];        // global index (to exclude the drone itself)
  double best[kRowsPerLane];     // row-side minimum over the share's columns
  int bestj[kRowsPerLane];
};
// the rows of row block I of a call with R rows, the first of them global drone ro.  (The callers value-initialise the
// set where they declare it, `RowSet rs = {}`: where its first stores arrive only through this inlined helper the
// compiler carries every row's `best` twice through the column loop, one copy for the compare and one for the value
// stored -- collide_span_kernel 127 -> 128 VGPRs and 28 bytes of scratch.)
__device__ __forceinline__ void row_set_init(RowSet &rs, int I, int lane, int R, int ro) {
#pragma unroll
  for (int rr = 0; rr < kRowsPerLane; ++rr) {
    const int raw = I * kRowBlock + rr * kWave + lane;
    rs.live[rr] = raw < R;
    rs.grow[rr] = ro + (rs.live[rr] ? raw : R - 1);
    rs.best[rr] = INFINITY;
    rs.bestj[rr] = -1;
  }
}

// The exact broad phase of a whole-swarm pass (launch_formation_collide, "cull" path).  Rows and columns are walked in
// a spatially sorted order (Morton order of the drones' path boxes); every aligned group of 8 drones of that order has
// the bounding box of its drones' finite samples and the largest of its drones' BOUNDS -- a squared distance each drone
// is known to attain to some other drone (its sorted neighbours, collide_bound_kernel).  A two-sided share (128 rows x
// 8 columns) is evaluated unless, for every one of the row block's 16 groups, the box distance to the column group
// exceeds both groups' largest bounds: then no pair of the share can lower any of its rows' or columns' minima -- nor tie
// them: the test is strict, and the box distance is formed with the pass's own fma formula, so it never exceeds the
// squared distance of any pair of the two boxes.  Minima, partners (compared by ORIGINAL index, `oid`) and hits are
// those of the full pass, whatever the order and whatever is skipped.
struct CollideCull {
  const double *colbox;    // [ceil(N / 8)][6] lo x,y,z / hi x,y,z per aligned group of 8 sorted drones
};

// (clamped gaps, not differences, through pair_d2's own formula: the value must never exceed pair_d2 of any pair of
// points of the two boxes)
__device__ __forceinline__ double box_box_lb2(const double *__restrict__ a, const double *__restrict__ b) {
#pragma clang fp contract(off)
  double gp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double g1 = a[k] - b[3 + k], g2 = b[k] - a[3 + k];     // lo_a - hi_b, lo_b - hi_a
    gp[k] = fmax(0.0, fmax(g1, g2));
  }
  return __builtin_fma(gp[2], gp[2], __builtin_fma(gp[1], gp[1], gp[0] * gp[0]));
}

// One block of NC (even, <= kColBlock) consecutive columns [cj, cj + ncols) against the wave's
// kRowBlock rows: the minima of the register tile (pair_tile_minima, msnap_pair_tile.h: straight-line
// code over the columns, so a short block takes the next instance up), folded into the row side and,
// for a two-sided block, the column side.
template <int NC, bool CULL = false>
__device__ __forceinline__ void collide_block(const CollideGeom &g, const double *__restrict__ prowT,
                                              const double *__restrict__ pcol, int cj, int ncols, bool two_sided,
                                              RowSet &rs, int I, int h, int crow, int lane, double *sFold, int *sFoldI,
                                              double *__restrict__ cpart_d2, int32_t *__restrict__ cpart_i,
                                              const int32_t *__restrict__ oid = nullptr) {
  constexpr int RPL = kRowsPerLane;
  double acc[RPL][NC];
  pair_tile_minima<NC>(prowT, g.Rp, pcol, g.S, cj, ncols, lane, h, g.sparts, acc);
  // row side: columns ascend, so the lowest index wins a tie (cull path: sorted order, ties by the ORIGINAL index)
#pragma unroll
  for (int jj = 0; jj < NC; ++jj) {
    const int j = cj + jj;
    const int oj = CULL ? oid[jj < ncols ? j : cj] : j;
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr) {
      acc[rr][jj] = (j == rs.grow[rr] || jj >= ncols) ? INFINITY : acc[rr][jj];
      const bool take = CULL ? (acc[rr][jj] < rs.best[rr]) | ((acc[rr][jj] == rs.best[rr]) & (oj < rs.bestj[rr]))
                             : (acc[rr][jj] < rs.best[rr]);
      if (take) {
        rs.best[rr] = acc[rr][jj];
        rs.bestj[rr] = oj;
      }
    }
  }
  if (two_sided) {
    // column side: min over the kRowBlock rows of every column of the block, with the lowest row.  Each
    // lane first folds its own rows (the lower row wins a tie); the 64 candidates of a column go through the
    // LDS image [column][lane]; lane = kColBlock * part + column then scans its part of the column and the
    // parts are folded with cross-lane exchanges.  Rows past the batch end replay row R-1 and must not win.
    // (The lane index is taken from an opaque copy: left visible, the fold's lane-derived addresses are hoisted
    // out of the share's loops and kept -- in scratch -- across the column loop, whose 128 registers are spoken for.)
    asm volatile("" : "+v"(lane));
    int orow[RPL];       // cull path: the rows' ORIGINAL indices, fetched here rather than held through the column loop
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr) orow[rr] = CULL ? oid[rs.live[rr] ? I * kRowBlock + rr * kWave + lane : g.R - 1] : 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      double v = rs.live[0] ? acc[0][c] : INFINITY;
      int vi = CULL ? orow[0] : lane;
#pragma unroll
      for (int rr = 1; rr < RPL; ++rr) {
        const double o = rs.live[rr] ? acc[rr][c] : INFINITY;
        const int oi = CULL ? orow[rr] : lane + rr * kWave;
        if (o < v || (CULL && o == v && oi < vi)) {
          v = o;
          vi = oi;
        }
      }
      sFold[c * kWave + lane] = v;
      sFoldI[c * kWave + lane] = vi;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    constexpr int PER = kColBlock;                 // candidates a lane scans: 64 lanes / (64 / kColBlock) parts
    const int c = lane & (kColBlock - 1), part = lane / kColBlock;
    double cm = INFINITY;
    int ci = 0;
    if (c < NC) {
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const double v = sFold[c * kWave + part * PER + k];
        const int vi = sFoldI[c * kWave + part * PER + k];
        if (v < cm || (v == cm && vi < ci)) {
          cm = v;
          ci = vi;
        }
      }
    }
#pragma unroll
    for (int mask = kColBlock; mask <= 32; mask <<= 1) {
      const double other = shfl_xor_f64(cm, mask);
      const int oi = __shfl_xor(ci, mask);
      const bool take = (other < cm) | ((other == cm) & (oi < ci));
      cm = take ? other : cm;
      ci = take ? oi : ci;
    }
    if (part == 0 && c < ncols) {
      const size_t slot = (size_t)crow * g.R + (size_t)(cj + c - g.os);      // crow: the (row block, sample part) slot row
      cpart_d2[slot] = cm;
      cpart_i[slot] = (cm == INFINITY) ? -1 : (CULL ? ci : g.ro + I * kRowBlock + ci);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
  }
}

// the narrowest instance (2, kColBlock / 2 or kColBlock columns) that holds the block's ncols columns
template <bool CULL>
__device__ __forceinline__ void collide_block_by_width(int ncols, const CollideGeom &g, const double *__restrict__ prowT,
                                                       const double *__restrict__ pcol, int cj, bool two_sided,
                                                       RowSet &rs, int I, int h, int crow, int lane, double *sFold,
                                                       int *sFoldI, double *__restrict__ cpart_d2,
                                                       int32_t *__restrict__ cpart_i, const int32_t *__restrict__ oid) {
  if (ncols <= 2)
    collide_block<2, CULL>(g, prowT, pcol, cj, ncols, two_sided, rs, I, h, crow, lane, sFold, sFoldI, cpart_d2, cpart_i, oid);
  else if (ncols <= kColBlock / 2)
    collide_block<kColBlock / 2, CULL>(g, prowT, pcol, cj, ncols, two_sided, rs, I, h, crow, lane, sFold, sFoldI, cpart_d2,
                                       cpart_i, oid);
  else
    collide_block<kColBlock, CULL>(g, prowT, pcol, cj, ncols, two_sided, rs, I, h, crow, lane, sFold, sFoldI, cpart_d2,
                                   cpart_i, oid);
}

// The rows of a call as [sample][xyz][row] (row pitch Rp; the rows behind R replay row R - 1): 64 x 64
// tiles through LDS, read along a drone's samples and written along the rows.
// Rows of workgroups behind the `ny` of the transposition mark the column-side partner slots of a part launch
// as empty (-1): a part covers its first and last row block only partly, and the merge skips empty slots.
// `perm` (cull path): row r of the image is drone perm[r] of prow, and `psorted` receives the same rows drone-major
// (the column array of the sorted pass), both from one read of the tile.
__global__ void __launch_bounds__(256)
collide_transpose_kernel(const double *__restrict__ prow, int R, int Rp, int E, double *__restrict__ prow_t, int ny,
                         int32_t *__restrict__ fill, size_t fill_n, const int32_t *__restrict__ perm,
                         double *__restrict__ psorted) {
  constexpr int TE = 32;      // elements of a drone per tile (x 64 rows): 2.4 workgroups per CU at 4096 x 91
  __shared__ double tile[64][TE + 1];
  if ((int)blockIdx.y >= ny) {
    const size_t stride = (size_t)(gridDim.y - ny) * gridDim.x * 256;
    uniform_for<size_t>(threadIdx.x, fill_n, stride, [&](size_t i) { fill[i] = -1; },
                        ((size_t)(blockIdx.y - ny) * gridDim.x + blockIdx.x) * 256);
    return;
  }
  const int r0 = blockIdx.x * 64, e0 = blockIdx.y * TE;
  {
    const int tx = threadIdx.x & (TE - 1), ty = threadIdx.x / TE;
#pragma unroll      // (compile-time bounds, the same trips for every lane: not a loop in the code)
    for (int i = ty; i < 64; i += 256 / TE) {
      const int r = min(r0 + i, R - 1), e = e0 + tx;
      const double v = e < E ? prow[(size_t)(perm ? perm[r] : r) * E + e] : 0.0;
      tile[i][tx] = v;
      if (psorted && e < E && r0 + i < R) psorted[(size_t)r * E + e] = v;
    }
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll      // (as above)
  for (int i = ty; i < TE; i += 4) {
    const int e = e0 + i;
    if (e < E) prow_t[(size_t)e * Rp + r0 + tx] = tile[tx][i];
  }
}

__device__ __forceinline__ void collide_span_body(const double *__restrict__ prow_t, const double *__restrict__ pcol,
                                                  const CollideGeom &g, double *__restrict__ part_d2,
                                                  int32_t *__restrict__ part_j, double *__restrict__ cpart_d2,
                                                  int32_t *__restrict__ cpart_i) {
  constexpr int CB = kColBlock;
  __shared__ double sFold[CB * kWave];
  __shared__ int sFoldI[CB * kWave];
  const int lane = threadIdx.x;
  const int w = blockIdx.x / g.sparts, h = blockIdx.x - w * g.sparts;
  long long u = collide_share_begin(g, w);
  const long long u_end = collide_share_begin(g, (long long)w + 1);
  if (u >= u_end) return;
  // the row block the share starts in
  int I = 0;
  while (I + 1 < g.n_rb && collide_ustart(g, I + 1) <= u) ++I;
  for (; u < u_end; ++I) {
    const long long ub = collide_ustart(g, I), un = collide_ustart(g, I + 1);
    const int ua = (int)(u - ub);                                         // first unit inside row block I
    const int ue = (int)((u_end < un ? u_end : un) - ub);                 // one past the last
    u = ub + ue;
    // unit -> column: the columns left of the own range, then from the row block's own first column on
    const int diag0 = g.os + I * kRowBlock;                               // only meaningful with g.sym
    const int skip = g.sym ? I * kRowBlock : 0;                           // own-range columns not met
    RowSet rs = {};
    row_set_init(rs, I, lane, g.R, g.ro);
    const double *prowT = prow_t + (size_t)(I - g.I_lo) * kRowBlock;
    const int crow = (I - g.I_lo) * g.sparts + h;
    for (int ux = ua; ux < ue;) {
      // a block: up to CB consecutive columns that do not straddle a boundary of the line
      const int cj = (g.sym && ux >= g.os) ? ux + skip : ux;
      int lim = ue - ux;                                                  // columns left in the share
      bool two_sided = false;
      if (g.sym) {
        if (cj < g.os) lim = lim < g.os - cj ? lim : g.os - cj;                               // left of the own range
        else if (cj < diag0 + kRowBlock) lim = lim < diag0 + kRowBlock - cj ? lim : diag0 + kRowBlock - cj;   // diagonal block
        else if (cj < g.oe) {                                                                // behind it, still own
          lim = lim < g.oe - cj ? lim : g.oe - cj;
          two_sided = true;
        }
      }
      const int ncols = lim < CB ? lim : CB;
      ux += ncols;
      collide_block_by_width<false>(ncols, g, prowT, pcol, cj, two_sided, rs, I, h, crow, lane, sFold, sFoldI, cpart_d2,
                                    cpart_i, nullptr);
    }
    // one partial entry per (wave, row block): w + I is unique (a later wave starts in a later or the same
    // row block) and the entries of row block I are the contiguous ids of the waves that meet it
    const size_t id = ((size_t)w + (I - g.I_lo)) * g.sparts + h;
#pragma unroll
    for (int rr = 0; rr < kRowsPerLane; ++rr) {
      part_d2[id * kRowBlock + rr * kWave + lane] = rs.best[rr];
      part_j[id * kRowBlock + rr * kWave + lane] = (rs.best[rr] == INFINITY) ? -1 : rs.bestj[rr];
    }
  }
}

__global__ void __launch_bounds__(kWave, 4)
collide_span_kernel(const double *__restrict__ prow_t, const double *__restrict__ pcol, CollideGeom g,
                    double *__restrict__ part_d2, int32_t *__restrict__ part_j, double *__restrict__ cpart_d2,
                    int32_t *__restrict__ cpart_i) {
  collide_span_body(prow_t, pcol, g, part_d2, part_j, cpart_d2, cpart_i);
}

// ---- the whole-swarm pass with the exact broad phase (CollideCull) ----
// Sorted order; row block I (rows 128 I ..) meets the columns from its own first one on, in aligned groups of 8:
// share k of row block I is the columns 128 I + 8 k .. (+ 8); its first 16 shares are the diagonal block (one-sided
// among the block's own rows, never culled), the others are two-sided and culled by the box test.

// Sample parts per surviving share.  A share is kSampleChunk-sample chunks of VALU work (1.7 us of SIMD time each
// at 8 columns x 128 rows) plus some 1.5 us of its own per item -- list entry, first row loads, the fold; the items are
// spread over the SIMDs, which run their waves one instruction at a time: the estimate is the number of items a SIMD
// works off times the length of one, and the part count with the smallest estimate wins (a part keeps two chunks).
// The fixture's 1393 survivors take 95-96 us per pass with 2, 3 or 4 parts alike (1: 106); cutting some shares into one
// part more than the others so that the items are exactly the wave slots changed nothing there and cost a sparse
// swarm 10 us (its uncut shares become the long poles) -- CullSplit keeps that form, x = 0.
constexpr int kCullMaxParts = 8;
struct CullSplit {
  int lo, hi, x;      // x shares in `hi` parts, the others in `lo`
  __device__ __host__ __forceinline__ int items(int tot) const { return x * hi + (tot - x) * lo; }
  // first item of list position f
  __device__ __host__ __forceinline__ int item_of(int f) const { return f <= x ? f * hi : x * hi + (f - x) * lo; }
};
// `force`: bits 0..7 a part count to use whatever the estimate says (0: none), bits 8.. the largest part count the
// column-side slots of this launch were laid out for (0: kCullMaxParts)
__device__ __host__ __forceinline__ CullSplit cull_split(int tot, int slots, int nch, int force) {
  CullSplit c;
  c.x = 0;
  int maxp = (force >> 8) > 0 && (force >> 8) < kCullMaxParts ? (force >> 8) : kCullMaxParts;
  force &= 0xff;
  if (force > 0) {
    c.lo = c.hi = force < maxp ? force : maxp;
    return c;
  }
  // the row-side entries of a launch are laid out for max(shares, 2 x slots) items (launch_formation_collide): a share
  // is cut only while the items stay below twice the wave slots
  const int fit = tot > 0 ? 2 * slots / tot : maxp;
  maxp = fit < maxp ? (fit > 1 ? fit : 1) : maxp;
  const int simds = slots / 4 > 0 ? slots / 4 : 1;
  int best = 1;
  long long best_cost = -1;
  for (int sp = 1; sp <= maxp && (sp == 1 || nch / sp >= 2); ++sp) {
    const long long serial = ((long long)tot * sp + simds - 1) / simds;
    const long long cost = serial * (17 * ((nch + sp - 1) / sp) + 15);      // 0.1 us
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      best = sp;
    }
  }
  c.lo = c.hi = best;
  return c;
}

// The second granularity of the broad phase: pairs of GROUPS (8 x 8 drones of the sorted order).  Of a surviving share
// (128 rows x 8 columns) usually one or two of its 16 row groups are what kept it; the group pairs that pass the same
// test are a few per cent of all (fixture: 3919 of 131 328, 0.25 M pairs against the surviving shares' 1.43 M).  They
// are evaluated by collide_eval_groups_kernel with the samples across the lanes, every item leaving 16 candidates -- one
// per row drone and one per column drone.  The selection leaves, besides the list itself, what lets
// collide_finish_groups_kernel fold a group's candidates without searching: the items of group g as the row side are the
// contiguous list range [astart[g], + acnt[g]) (the diagonal item (g, g) included), the items (a, g) with g as the column
// side are the non-zero entries of blist[g][a < g] = list position + 1.
struct CullGroups {
  int32_t *glist;                 // [cap] (a << 16 | b), a <= b: surviving group pairs, a-major, ascending b per a
  int32_t *astart, *acnt;         // [nG] list range of the items (g, b >= g)
  int32_t *blist;                 // [nG][nG]: list position + 1 of the item (a, g) at [g][a] (0: none; zeroed per pass)
  double *cand_d2;                // [cap][16] what item `it` found for its 8 row drones and its 8 column drones
  int32_t *cand_j;
  int cap;                        // list capacity (all group pairs when this path is taken: it cannot overflow)
  int nG;
};
// Same arithmetic per pair and sample on both paths; the group kernel spends about 2.2 x as many vector instructions per
// pair-sample (91 samples on 128 lanes, the cross-lane folds), the share kernel runs a single short round at 0.7 of its
// pace: groups when 64 x 2.2 x (group pairs) < 1024 x 1.45 x (shares).
__device__ __host__ __forceinline__ bool cull_groups_cheaper(long long shares, long long groups) {
  return groups * 141 < shares * 1485;
}
// what a pass leaves for the next one's choice of evaluator (one 64-bit word in page-locked host memory, written by
// the evaluator's first wave: the host reads it without synchronising): swarm size, surviving shares, surviving
// group pairs
__device__ __host__ __forceinline__ unsigned long long cull_hint_pack(int N, int shares, long long groups) {
  return ((unsigned long long)(N & 0x7fff) << 48) | ((unsigned long long)(shares & 0xffffff) << 24) |
         (unsigned long long)(groups < 0xffffff ? groups : 0xffffff);
}

// One workgroup per row block: its threads test the shares (at most 1024 of them: kCullMaxDrones / 8); the survivors are
// written, in ascending order, to a range of the list that the workgroup reserves with one atomic add -- the row
// blocks' ranges come in any order, each is contiguous: list[start[I] .. + cnt[I]) = (I << 16 | k).
// (1024 threads: with 256 a wavefront sat alone on its SIMD and walked 32 dependent box tests -- 12 us of an 8-launch
// pass's shortest chain; sixteen wavefronts per workgroup hide each other's latencies)
constexpr int kSelThreads = 1024;
constexpr int kSelGroups = 8;      // group-pair selection: a's per workgroup
// kSelTrips (template parameter): trips of a workgroup over a row block's shares / a group's partners: 1 up to 8192
// drones, 2 up to kCullMaxDrones (16 384 / 8 = 2 x kSelThreads)
template <int kSelTrips>
__global__ void __launch_bounds__(kSelThreads)
collide_select_kernel(int N, int n_rb, CollideCull cu, const double *__restrict__ bound, int32_t *__restrict__ list,
                      int32_t *__restrict__ cnt, int32_t *__restrict__ meta, CullGroups cg) {
  // Every workgroup first stages what all its tests read: the largest bound of every group of 8 sorted drones (the
  // bounds were finished by the previous launch: atomic minima of the gather tiles over the sorted neighbours; 0 for a
  // drone without a finite sample) and -- swarms up to 8192 drones, 56 KB -- the groups' boxes: one memory round trip,
  // then the box tests run out of LDS.
  constexpr bool kStage = kSelTrips == 1;
  constexpr int kStageGroups = kStage ? kCullGroupMaxDrones / kColBlock : 1;
  __shared__ double sCmax[kCullMaxDrones / kColBlock];
  __shared__ double sBox[kStageGroups * 6];
  {
    const int nG = (N + kColBlock - 1) / kColBlock;
    uniform_for<int>(threadIdx.x, nG, kSelThreads, [&](int gq) {
      double m = 0.0;
#pragma unroll
      for (int d = 0; d < kColBlock; ++d) {
        const int r = gq * kColBlock + d;
        m = fmax(m, bound[r < N ? r : N - 1]);
      }
      sCmax[gq] = m;
    });
    if constexpr (kStage) {      // (one flight: six loads per thread at most)
      double bv[kStageGroups * 6 / kSelThreads];
#pragma unroll
      for (int u = 0; u < kStageGroups * 6 / kSelThreads; ++u) {
        const int e = threadIdx.x + u * kSelThreads;
        bv[u] = e < nG * 6 ? cu.colbox[e] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kStageGroups * 6 / kSelThreads; ++u) {
        const int e = threadIdx.x + u * kSelThreads;
        if (e < nG * 6) sBox[e] = bv[u];
      }
    }
    __syncthreads();
  }
  auto load_box = [&](int gq, double(&B)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if constexpr (kStage) B[k] = sBox[gq * 6 + k];
      else B[k] = cu.colbox[(size_t)gq * 6 + k];
    }
  };
  if ((int)blockIdx.x >= n_rb) {
    // group pairs (a, b), a <= b: a workgroup takes kSelGroups a's and tests each against every b (the same strict test
    // on the two groups' boxes and bounds); its survivors are appended with ONE atomic reservation -- a reservation per
    // a was 512 atomics on one word, 20 ns apiece -- the workgroups in no particular order
    constexpr int NW = kSelThreads / kWave, NS = kSelGroups * kSelTrips;
    __shared__ int gsum[NS * NW + 1];
    __shared__ int gbase, gtot;
    const int a0 = (blockIdx.x - n_rb) * kSelGroups, nG = (N + kColBlock - 1) / kColBlock;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    unsigned long long kept = 0;      // bit (ai * kSelTrips + t): pair (a0 + ai, a + t * kSelThreads + thread) survives
#pragma unroll
    for (int ai = 0; ai < kSelGroups; ++ai) {
      const int a = a0 + ai;
      double A[7], A6[6];
      load_box(a < nG ? a : nG - 1, A6);
#pragma unroll
      for (int k = 0; k < 6; ++k) A[k] = A6[k];
      A[6] = sCmax[a < nG ? a : nG - 1];
#pragma unroll
      for (int t = 0; t < kSelTrips; ++t) {      // (at most kCullMaxDrones / 8 groups)
        bool keep = false;
        if (a + t * kSelThreads < nG) {      // (wave-uniform)
          const int b = a + t * kSelThreads + threadIdx.x, bc = b < nG ? b : nG - 1;
          double B6[6];
          load_box(bc, B6);
          const double lb2 = box_box_lb2(A, B6);
          keep = b < nG && (b == a || !((lb2 > A[6]) & (lb2 > sCmax[bc])));
        }
        const unsigned long long m = __ballot(keep);
        kept |= keep ? 1ull << (ai * kSelTrips + t) : 0ull;
        if (lane == 0) gsum[(ai * kSelTrips + t) * NW + w] = __popcll(m);
      }
    }
    __syncthreads();
    // exclusive scan of the NS x NW wave counts (two wavefronts' worth)
    if (threadIdx.x < kWave) {
      int run = 0;
      for (int i0 = 0; i0 < NS * NW; i0 += kWave) {
        const int v = i0 + lane < NS * NW ? gsum[i0 + lane] : 0;
        int inc = v;
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) {
          const int o = __shfl_up(inc, m);
          inc += lane >= m ? o : 0;
        }
        if (i0 + lane < NS * NW) gsum[i0 + lane] = run + inc - v;
        run += __shfl(inc, kWave - 1);
      }
      if (lane == 0) {
        gbase = atomicAdd(&meta[kMetaGroups], run);
        gtot = run;
      }
    }
    __syncthreads();
    // the survivors of one a are contiguous (a-major order): its row-side range for the evaluator's finish
    if (threadIdx.x < kSelGroups && a0 + (int)threadIdx.x < nG) {
      const int ai = threadIdx.x;
      const int s0 = gsum[ai * kSelTrips * NW], s1 = ai + 1 < kSelGroups ? gsum[(ai + 1) * kSelTrips * NW] : gtot;
      cg.astart[a0 + ai] = gbase + s0;
      cg.acnt[a0 + ai] = s1 - s0;
    }
#pragma unroll
    for (int ai = 0; ai < kSelGroups; ++ai)
#pragma unroll
      for (int t = 0; t < kSelTrips; ++t) {
        const bool keep = (kept >> (ai * kSelTrips + t)) & 1ull;
        const unsigned long long m = __ballot(keep);
        const int pos = gbase + gsum[(ai * kSelTrips + t) * NW + w] + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < cg.cap) {
          const int a = a0 + ai, b = a + t * kSelThreads + threadIdx.x;
          cg.glist[pos] = (a << 16) | b;
          if (b != a) cg.blist[(size_t)b * cg.nG + a] = pos + 1;      // the column side's reverse list (0: none)
        }
      }
    return;
  }
  constexpr int GPB = kRowBlock / kColBlock;      // groups of 8 per row block
  constexpr int NW = kSelThreads / kWave;
  __shared__ int wsum[kSelTrips][NW];
  __shared__ int sStart;
  __shared__ double sRow[GPB][8];      // the row block's own groups: box, largest bound
  __shared__ double sAll[8];           // their union, the largest of their bounds
  const int I = blockIdx.x, lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int nsh = (N - I * kRowBlock + kColBlock - 1) / kColBlock;      // <= kSelTrips * kSelThreads (kCullMaxDrones)
  const int ng = nsh < GPB ? nsh : GPB;
  if (threadIdx.x < 7 * GPB) {
    const int q = threadIdx.x / 7, k = threadIdx.x % 7;
    if (q < ng) sRow[q][k] = k < 6 ? (kStage ? sBox[(I * GPB + q) * 6 + k] : cu.colbox[(size_t)(I * GPB + q) * 6 + k]) : sCmax[I * GPB + q];
  }
  __syncthreads();
  // the union of the row block's groups: a share that fails against it fails against every group (most do, and whole
  // wavefronts of them: the group-by-group test below is 16 box distances per share)
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    double v = sRow[0][k];
    for (int q = 1; q < ng; ++q) v = k < 3 ? fmin(v, sRow[q][k]) : fmax(v, sRow[q][k]);
    sAll[k] = v;
  }
  __syncthreads();
  unsigned long long mk[kSelTrips];
  bool keep[kSelTrips];
  // (the column groups' boxes of all trips are fetched before the first test: one memory round trip, not four)
  double cbx[kSelTrips][6], cmx[kSelTrips];
#pragma unroll
  for (int t = 0; t < kSelTrips; ++t) {
    if (t * kSelThreads >= nsh) continue;      // (workgroup-uniform)
    const int k = t * kSelThreads + threadIdx.x, J = I * GPB + (k < nsh ? k : nsh - 1);
    load_box(J, cbx[t]);
    cmx[t] = sCmax[J];
  }
#pragma unroll
  for (int t = 0; t < kSelTrips; ++t) {
    const int k = t * kSelThreads + threadIdx.x;
    keep[t] = false;
    if (k < nsh) {
      keep[t] = true;
      if (k >= GPB) {
        // Skip the share unless some pair of it could reach (or tie) a minimum of its row or its column: the rows are
        // taken group by group -- a block of 128 consecutive drones of the sorted order can straddle a jump of the
        // curve, its groups of 8 hardly ever do.
        const double cm = cmx[t];
        bool any = false;
        const double lb0 = box_box_lb2(sAll, cbx[t]);
        if (!((lb0 > sAll[6]) & (lb0 > cm))) {
          for (int q = 0; q < ng; ++q) {
            const double lb2 = box_box_lb2(sRow[q], cbx[t]);
            any |= !((lb2 > sRow[q][6]) & (lb2 > cm));
          }
        }
        keep[t] = any;
      }
    }
    mk[t] = __ballot(keep[t]);
    if (lane == 0) wsum[t][w] = __popcll(mk[t]);
  }
  __syncthreads();
  int all = 0, off[kSelTrips];
#pragma unroll
  for (int t = 0; t < kSelTrips; ++t) {
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      if (q == w) off[t] = all;      // (all: the survivors with a lower share number so far)
      all += wsum[t][q];
    }
  }
  if (threadIdx.x == 0) {
    const int start = atomicAdd(&meta[kMetaTotal], all);
    sStart = start;
    meta[kMetaStart + I] = start;
    cnt[I] = all;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kSelTrips; ++t)
    if (keep[t]) list[sStart + off[t] + __popcll(mk[t] & ((1ull << lane) - 1ull))] = (I << 16) | (t * kSelThreads + threadIdx.x);
}

// The surviving shares, walked by a fixed grid of waves: item it = (survivor it / sp, sample part it % sp) of the
// list; its row-side partial entry is entry `it` of part_d2 / part_j, the column side goes to the (row block,
// sample part) slots as in the plain pass.  The next item's list entry is fetched before the current item runs.
__device__ __forceinline__ void
collide_span_list_body(const double *__restrict__ prow_t, const double *__restrict__ pcol, CollideGeom g,
                       double *__restrict__ part_d2, int32_t *__restrict__ part_j, double *__restrict__ cpart_d2,
                       int32_t *__restrict__ cpart_i, const int32_t *__restrict__ oid, const int32_t *__restrict__ list,
                       int sp_force, int slots, int32_t *__restrict__ meta) {
  constexpr int CB = kColBlock;
  __shared__ double sFold[CB * kWave];
  __shared__ int sFoldI[CB * kWave];
  const int lane = threadIdx.x;
  const int tot = meta[kMetaTotal];
  const CullSplit sp = cull_split(tot, slots, pair_tile_chunks(g.S), sp_force);
  if (blockIdx.x == 0 && lane == 0) {
    meta[kMetaParts] = sp.lo;
    meta[kMetaParts + 1] = sp.hi;
    meta[kMetaParts + 2] = sp.x;
  }
  const int items = sp.items(tot);      // (at most 33280 shares x kCullMaxParts)
  const int xi = sp.x * sp.hi;          // items of the shares cut into `hi` parts
  auto share_of = [&](int it) { return it < xi ? it / sp.hi : sp.x + (it - xi) / sp.lo; };
  int it = blockIdx.x;
  int entry = it < items ? list[share_of(it)] : 0;
  while (it < items) {
    const int f = share_of(it);
    g.sparts = it < xi ? sp.hi : sp.lo;
    const int h = it - sp.item_of(f);
    const int I = entry >> 16, k = entry & 0xffff;
    const int nxt = it + gridDim.x;
    entry = nxt < items ? list[share_of(nxt)] : 0;
    const int crow = I * sp.hi + h;      // column-side slot row: `hi` rows per row block
    const int cj = I * kRowBlock + k * CB;
    const int ncols = g.Cn - cj < CB ? g.Cn - cj : CB;
    const bool two_sided = k >= kRowBlock / CB;
    RowSet rs = {};
    row_set_init(rs, I, lane, g.R, 0);      // (sorted order: rows are numbered from 0)
    const double *prowT = prow_t + (size_t)I * kRowBlock;
    collide_block_by_width<true>(ncols, g, prowT, pcol, cj, two_sided, rs, I, h, crow, lane, sFold, sFoldI, cpart_d2,
                                 cpart_i, oid);
#pragma unroll
    for (int rr = 0; rr < kRowsPerLane; ++rr) {
      part_d2[(size_t)it * kRowBlock + rr * kWave + lane] = rs.best[rr];
      part_j[(size_t)it * kRowBlock + rr * kWave + lane] = (rs.best[rr] == INFINITY) ? -1 : rs.bestj[rr];
    }
    it = nxt;
  }
}

// One wavefront per surviving group pair (a, b): 32 SAMPLES x the two halves of the column group across the lanes
// (lane = 32 half + sample; three trips for 65..96 samples), the 8 rows x 4 columns of the half in registers -- both
// drones' positions come as coalesced loads of the sorted drone-major copy, no scalar or LDS operand traffic.  After the
// samples a reduce-scatter butterfly inside each half (32 -> 16 -> ... -> 1 value per lane, halving the lane span each
// time) leaves pair (r, c) = ((lane >> 2) & 7, lane & 3) of the half in its lane; row-side (over c, then over the halves)
// and column-side (over r) candidates follow with lexicographic (distance, ORIGINAL index) folds and go to the item's
// 16 candidate slots.
constexpr int kGroupHalf = kColBlock / 2;
constexpr int kGroupLanes = kWave / 2;  // samples per trip

// The pass's last launch on the group path: one wavefront per group of 8 sorted drones folds the candidates of all the
// group's items -- row-side slots of the items (g, b) (a contiguous list range), column-side slots of the items (a, g)
// (the non-zero entries of the group's reverse-list row, fetched in one flight and compacted through LDS) -- a lane per
// item, then across the lanes drone by drone: the minimum, and the lowest ORIGINAL partner index among the lanes that hold
// it (as in the all-pairs pass); distance, partner and hit leave through the sort permutation.
// (Built first as the tail of the evaluator -- the wave completing a group's last item, found by an arrival counter,
// finished the group: 36 us where evaluator + this launch take 27.  Inside one launch the candidates cross XCDs through
// device-coherent stores the writer has to wait for, a returning atomic and coherent loads: five memory-side round trips
// of ~2 us behind every item, against one kernel boundary.)
constexpr int kFinishWaves = 4;      // groups (wavefronts) per workgroup
// kChunks (template parameter): 64-entry chunks of a reverse-list row: 8 up to 4096 drones, 16 up to 8192, 32 up to 16 384
template <int kChunks>
__global__ void __launch_bounds__(kWave * kFinishWaves)
collide_finish_groups_kernel(int N, const int32_t *__restrict__ oid, const int32_t *__restrict__ meta, CullGroups cg,
                             double radius, double *__restrict__ min_dist, int32_t *__restrict__ partner,
                             int32_t *__restrict__ hit) {
  __shared__ int sItAll[kFinishWaves][kChunks * kWave];
  const int lane = threadIdx.x & (kWave - 1), w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  int *sIt = sItAll[w];
  const int gq = blockIdx.x * kFinishWaves + w;
  if (gq >= cg.nG) return;
  int pl[kChunks];
#pragma unroll
  for (int c = 0; c < kChunks; ++c)
    pl[c] = (c * kWave < gq && c * kWave + lane < gq) ? cg.blist[(size_t)gq * cg.nG + c * kWave + lane] : 0;
  if (meta[kMetaGroups] > cg.cap) {
    // more survivors than list slots: the share evaluator runs.  The selection still filled the reverse lists of the
    // first cap items -- cleared here as below, the next pass trusts them to be all-zero (blist_clean)
#pragma unroll
    for (int c = 0; c < kChunks; ++c)
      if (pl[c] > 0) cg.blist[(size_t)gq * cg.nG + c * kWave + lane] = 0;
    return;
  }
  const int nA = cg.acnt[gq], sA = cg.astart[gq];
  // lane = 8 e + k: entry slot e, drone k of the group
  const int k = lane & (kColBlock - 1), e = lane >> 3;
  const int r = gq * kColBlock + k;
  const int out = r < N ? oid[r] : 0;      // (fetched under the candidates)
  int nB = 0;
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const unsigned long long m = __ballot(pl[c] > 0);      // (0 behind the group's own row)
    if (pl[c] > 0) sIt[nB + __popcll(m & ((1ull << lane) - 1ull))] = pl[c] - 1;
    nB += __popcll(m);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
  double best = INFINITY;
  int bj = -1;
  constexpr int U = 8;      // entries of a lane in flight: 64 items of the group per round (a round is a dependent round
                            // trip: configs[3] fixture 12.5 -> 11.2 us against U = 4; 16 gives no more)
  for (int q0 = 0; q0 < nA + nB; q0 += U * (kWave / kColBlock)) {
    double d[U];
    int j[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * (kWave / kColBlock) + e;
      d[u] = INFINITY;
      j[u] = -1;
      if (q < nA + nB) {
        const size_t slot = (q < nA ? (size_t)(sA + q) * 16 : (size_t)sIt[q - nA] * 16 + kColBlock) + k;
        d[u] = cg.cand_d2[slot];
        j[u] = cg.cand_j[slot];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (j[u] >= 0 && (bj < 0 || d[u] < best || (d[u] == best && j[u] < bj))) {
        best = d[u];
        bj = j[u];
      }
  }
  // the eight entry lanes of a drone folded: lowest distance, then lowest ORIGINAL partner index
#pragma unroll
  for (int m = kColBlock; m < kWave; m <<= 1) {
    const double o = shfl_xor_f64(best, m);
    const int oj = __shfl_xor(bj, m);
    if (oj >= 0 && (bj < 0 || o < best || (o == best && oj < bj))) {
      best = o;
      bj = oj;
    }
  }
  if (e == 0 && r < N) {
    const double dist = sqrt(bj >= 0 ? best : INFINITY);
    min_dist[out] = dist;
    partner[out] = bj;
    hit[out] = (dist < 2.0 * radius) ? 1 : 0;
  }
  // the row is left clean for the next pass (here, not where it is read: the counter the candidate loads wait on
  // counts stores too, and they would wait for these)
#pragma unroll
  for (int c = 0; c < kChunks; ++c)
    if (pl[c] > 0) cg.blist[(size_t)gq * cg.nG + c * kWave + lane] = 0;
}

// The evaluator of the surviving group pairs: a fixed grid of waves walks the list, one item per wave slot at the
// fixture's 3919 survivors; collide_finish_groups_kernel follows.
constexpr int kGroupWaves = 4;      // waves per SIMD the group evaluator is built for (128 registers)
__global__ void __launch_bounds__(kWave, kGroupWaves)
collide_eval_groups_kernel(const double *__restrict__ pcol, int N, int S, const int32_t *__restrict__ oid,
                           const int32_t *__restrict__ meta, CullGroups cg, unsigned long long *__restrict__ hint) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  int tot = meta[kMetaGroups];
  if (blockIdx.x == 0 && lane == 0 && hint != nullptr)
    __hip_atomic_store(hint, cull_hint_pack(N, meta[kMetaTotal], tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (tot > cg.cap) tot = 0;      // (more survivors than list slots: the share evaluator behind this launch runs instead)
  const unsigned stride = (unsigned)S * 3u;
  // XCD-aware item order.  Blocks are dealt round-robin over the 8 XCDs (observed; a speed matter only), so the blocks
  // b, b + 8, ... share an XCD and its L2: they walk one contiguous eighth of the list.  The list is a-major -- the ~8
  // items of a group sit side by side and each reads the group's 8 drone rows (17 KB), their column groups are
  // neighbours in the sorted order -- so most of an item's 35 KB are then hits in its XCD's 4 MB L2; in list order the
  // eight items of a group went to eight XCDs and every one of them fetched the rows from beyond L2.
  const int per = (tot + 7) >> 3;
  auto item_of = [&](int v) { return (v >> 3) < per ? (v & 7) * per + (v >> 3) : tot; };      // (>= tot: none)
  // (the first list entry is fetched beside the survivor count, the next one under the current item)
  int v = blockIdx.x, it = item_of(v);
  int entry = (it < tot && it < cg.cap) ? cg.glist[it] : 0;
  for (; (v >> 3) < per; v += gridDim.x, it = item_of(v)) {
    const int it_next = item_of(v + (int)gridDim.x);
    const int ent_raw = entry;
    entry = it_next < tot ? cg.glist[it_next] : 0;
    if (it >= tot) continue;
    // (the entry is wave-uniform: as a scalar the drones' row bases are scalar too, and every load is base + one lane offset)
    const int ent = __builtin_amdgcn_readfirstlane(ent_raw);
    const int a = ent >> 16, b = ent & 0xffff;
    const bool diag = a == b;

    // (everything derived from the lane index is rebuilt per phase from an opaque copy: left visible, the values the
    // candidate folds need are computed up front and held through the sample loop, whose 128 registers are spoken for)
    int lane_s = threadIdx.x;
    asm volatile("" : "+v"(lane_s));
    const int half = lane_s >> 5, ls = lane_s & (kGroupLanes - 1);
    double acc[kColBlock * kGroupHalf];
#pragma unroll
    for (int p = 0; p < kColBlock * kGroupHalf; ++p) acc[p] = INFINITY;
#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += kGroupLanes) {
      const int sq = s0 + ls < S ? s0 + ls : S - 1;      // (a sample seen twice does not change a minimum)
      // one 32-bit lane offset for all loads of the trip: scalar drone base + zero-extended lane offset + immediate
      const unsigned voff = (unsigned)sq * 24u;
      double cx[kGroupHalf], cy[kGroupHalf], cz[kGroupHalf];
#pragma unroll
      for (int c = 0; c < kGroupHalf; ++c) {
        const int d = b * kColBlock + half * kGroupHalf + c;      // (a last group may be short: clamped, masked below)
        const double *p = reinterpret_cast<const double *>(
            reinterpret_cast<const char *>(pcol + (size_t)(d < N ? d : N - 1) * stride) + (size_t)voff);
        cx[c] = p[0];
        cy[c] = p[1];
        cz[c] = p[2];
      }
      // The row drones' samples are fetched two rows ahead of the arithmetic, through a ring of three register sets.
      // Left to the compiler every row was load, wait, 28 operations -- 24 dependent L2 round trips per item, the whole
      // of the kernel's 21 us; the compiler barrier pins each fetch in front of the arithmetic two rows earlier.
      double rw[3][3];
      auto fetch = [&](int r, double(&dst)[3]) {
        const int d = a * kColBlock + r;
        const double *p = reinterpret_cast<const double *>(
            reinterpret_cast<const char *>(pcol + (size_t)(d < N ? d : N - 1) * stride) + (size_t)voff);
        dst[0] = p[0];
        dst[1] = p[1];
        dst[2] = p[2];
      };
      fetch(0, rw[0]);
      fetch(1, rw[1]);
#pragma unroll
      for (int r = 0; r < kColBlock; ++r) {
        if (r + 2 < kColBlock) fetch(r + 2, rw[(r + 2) % 3]);
        asm volatile("" ::: "memory");
        const double x = rw[r % 3][0], y = rw[r % 3][1], z = rw[r % 3][2];
#pragma unroll
        for (int c = 0; c < kGroupHalf; ++c) {
          const double dx = cx[c] - x, dy = cy[c] - y, dz = cz[c] - z;
          min_quiet(acc[r * kGroupHalf + c], pair_d2(dx, dy, dz));      // (behind the opaque lane copy: by hand)
        }
      }
    }
    // reduce-scatter over the 32 lanes of the half: 32 values per lane -> 1, pair p = lane & 31
#pragma unroll
    for (int n = 16, m = 16; n >= 1; n >>= 1, m >>= 1) {
      const bool up = (lane_s & m) != 0;
#pragma unroll
      for (int i = 0; i < n; ++i) {
        const double keep = up ? acc[i + n] : acc[i], send = up ? acc[i] : acc[i + n];
        acc[i] = __builtin_fmin(keep, __shfl_xor(send, m));
      }
    }
    double v = acc[0];
    // this lane's pair after the butterfly
    int lane_c = threadIdx.x;
    asm volatile("" : "+v"(lane_c));
    const int pr = (lane_c & (kGroupLanes - 1)) >> 2, pc = lane_c & (kGroupHalf - 1), half_c = lane_c >> 5;
    const int ra = a * kColBlock + pr, cb = b * kColBlock + half_c * kGroupHalf + pc;
    const int oi = oid[ra < N ? ra : N - 1], oj = oid[cb < N ? cb : N - 1];
    if (ra >= N || cb >= N || (diag && ra == cb)) v = INFINITY;
    // row side: over the 4 columns of the half (lane bits 0, 1), then over the halves (bit 5)
    {
      double w = v;
      int wj = oj;
#pragma unroll
      for (int m = 1; m <= 32; m = (m == 2 ? 32 : m << 1)) {
        const double o = __shfl_xor(w, m);
        const int ojx = __shfl_xor(wj, m);
        const bool take = (o < w) | ((o == w) & (ojx < wj));
        w = take ? o : w;
        wj = take ? ojx : wj;
      }
      if ((lane & 35) == 0) {      // half 0, pc == 0: lane = 4 pr
        cg.cand_d2[(size_t)it * 16 + pr] = w;
        cg.cand_j[(size_t)it * 16 + pr] = w < INFINITY ? wj : -1;
      }
    }
    // column side: over the 8 rows (lane bits 2..4); the diagonal group's columns are its rows
    {
      double w = v;
      int wi = oi;
#pragma unroll
      for (int m = 4; m <= 16; m <<= 1) {
        const double o = __shfl_xor(w, m);
        const int oix = __shfl_xor(wi, m);
        const bool take = (o < w) | ((o == w) & (oix < wi));
        w = take ? o : w;
        wi = take ? oix : wi;
      }
      if ((lane_c & (kGroupLanes - 1)) < kGroupHalf) {      // pr == 0: lane = 32 half + pc
        const int k = kColBlock + half_c * kGroupHalf + pc;
        cg.cand_d2[(size_t)it * 16 + k] = w;
        cg.cand_j[(size_t)it * 16 + k] = (!diag && w < INFINITY) ? wi : -1;
      }
    }
  }
}

// The evaluator of the surviving shares (collide_span_list_body above); collide_merge_kernel follows it.
__global__ void __launch_bounds__(kWave, 4)
collide_eval_shares_kernel(const double *__restrict__ prow_t, const double *__restrict__ pcol, CollideGeom g,
                           double *__restrict__ part_d2, int32_t *__restrict__ part_j, double *__restrict__ cpart_d2,
                           int32_t *__restrict__ cpart_i, const int32_t *__restrict__ oid, const int32_t *__restrict__ list,
                           int sp_force, int slots, int32_t *__restrict__ meta, unsigned long long *__restrict__ hint,
                           int groups_cap) {
  // (launched behind the group evaluator of a large swarm: only if the survivors did not fit its list)
  if (groups_cap > 0 && meta[kMetaGroups] <= groups_cap) return;
  if (blockIdx.x == 0 && threadIdx.x == 0 && hint != nullptr)
    __hip_atomic_store(hint, cull_hint_pack(g.R, meta[kMetaTotal], meta[kMetaGroups]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  collide_span_list_body(prow_t, pcol, g, part_d2, part_j, cpart_d2, cpart_i, oid, list, sp_force, slots, meta);
}

// paths shorter than one sample chunk: plain loops, one-sided
__global__ void __launch_bounds__(kWave)
collide_short_kernel(const double *__restrict__ prow, const double *__restrict__ pcol, int R, int ro, int Cn, int S,
                     double radius, double *__restrict__ min_dist, int32_t *__restrict__ partner,
                     int32_t *__restrict__ hit, int raw) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * kWave + threadIdx.x;
  if (r >= R) return;
  const int grow = ro + r;
  const double *pr = prow + (size_t)r * S * 3;
  double best = INFINITY;
  int bestj = -1;
  for (int j = 0; j < Cn; ++j) {
    const double *pc = pcol + (size_t)j * S * 3;
    double m = INFINITY;
    for (int sq = 0; sq < S; ++sq) {
      const double dx = pc[(size_t)sq * 3 + 0] - pr[(size_t)sq * 3 + 0];
      const double dy = pc[(size_t)sq * 3 + 1] - pr[(size_t)sq * 3 + 1];
      const double dz = pc[(size_t)sq * 3 + 2] - pr[(size_t)sq * 3 + 2];
      m = __builtin_fmin(pair_d2(dx, dy, dz), m);
    }
    if (j == grow) m = INFINITY;
    if (m < best) {
      best = m;
      bestj = j;
    }
  }
  if (raw) {      // a part of a pass (msnap_formation_collide_part): squared minimum, no hit flag
    min_dist[r] = best;
    partner[r] = (best == INFINITY) ? -1 : bestj;
    return;
  }
  const double dist = sqrt(best);
  min_dist[r] = dist;
  partner[r] = (best == INFINITY) ? -1 : bestj;
  hit[r] = (dist < 2.0 * radius) ? 1 : 0;
}

// One workgroup per kMergeRows rows, kMergeParts sub-groups: sub-group q sweeps every kMergeParts-th partial
// entry of its rows (a drone has a few hundred of them: swept by one thread the kernel is 28 us of dependent
// loads at 4096 drones; with 64 rows per workgroup only 64 of the 256 CUs had work), the sub-groups'
// candidates are folded through LDS.  16 consecutive rows are 128 contiguous bytes of a partial entry.
// (64 sub-groups with 8 loads per round: 12 us instead of 9 -- the sequential fold and the big workgroups cost
// more than the shorter sweeps save.)
constexpr int kMergeRows = 16;
constexpr int kMergeParts = 16;
__global__ void __launch_bounds__(kMergeRows * kMergeParts)
collide_merge_kernel(const double *__restrict__ part_d2, const int32_t *__restrict__ part_j, CollideGeom g,
                     const double *__restrict__ cpart_d2, const int32_t *__restrict__ cpart_i, double radius,
                     double *__restrict__ min_dist, int32_t *__restrict__ partner, int32_t *__restrict__ hit,
                     const int32_t *__restrict__ oid, const int32_t *__restrict__ cnt, const int32_t *__restrict__ meta,
                     int groups_cap = 0) {
  if (groups_cap > 0 && meta[kMetaGroups] <= groups_cap) return;      // (the group evaluator's fold wrote the results)
  __shared__ double sD[kMergeParts][kMergeRows];
  __shared__ int sJ[kMergeParts][kMergeRows];
  const int lr = threadIdx.x & (kMergeRows - 1), q = threadIdx.x / kMergeRows;
  const int r_raw = blockIdx.x * kMergeRows + lr;
  const int r = r_raw < g.R ? r_raw : g.R - 1;
  const int out = oid ? oid[r] : r;      // cull path: row r of the sorted pass is drone oid[r] (fetched under the sweeps)
  double best = INFINITY;
  int bj = -1;
  constexpr int U = 8;      // entries fetched per round: the loads of a round are independent
  auto sweep = [&](const double *pd, const int32_t *pj, size_t pitch, int n) {
    for (int s0 = q; s0 < n; s0 += U * kMergeParts) {
      double v[U];
      int j[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int sidx = s0 + k * kMergeParts;
        const int sc = sidx < n ? sidx : n - 1;
        v[k] = pd[(size_t)sc * pitch];
        j[k] = sidx < n ? pj[(size_t)sc * pitch] : -1;
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        if (j[k] >= 0 && (v[k] < best || (v[k] == best && j[k] < bj))) {
          best = v[k];
          bj = j[k];
        }
      }
    }
  };
  if (cnt) {
    // broad-phase pass through the surviving shares (collide_span_list_body): they are consecutive entries per row block
    const int I = __builtin_amdgcn_readfirstlane(r / kRowBlock);      // (kMergeRows divides kRowBlock)
    CullSplit sp;
    sp.lo = meta[kMetaParts];
    sp.hi = meta[kMetaParts + 1];
    sp.x = meta[kMetaParts + 2];
    const int f0 = meta[kMetaStart + I], first_item = sp.item_of(f0), n_items = sp.item_of(f0 + cnt[I]) - first_item;
    const size_t first = (size_t)first_item * kRowBlock + (r - I * kRowBlock);
    sweep(part_d2 + first, part_j + first, kRowBlock, n_items);
    if (I > 0) sweep(cpart_d2 + r, cpart_i + r, (size_t)g.R, I * sp.hi);
  } else if (g.total > 0) {
    // row side: the shares of this launch that met this drone's row block
    const int I = r / kRowBlock;
    long long ua = collide_ustart(g, I), ub = collide_ustart(g, I + 1) - 1;      // the row block's units ...
    ua = ua < g.u_lo ? g.u_lo : ua;                                                // ... that this launch walks
    ub = ub >= g.u_lo + g.u_n ? g.u_lo + g.u_n - 1 : ub;
    if (ub >= ua) {
      const long long wf = collide_share_of(g, ua), wl = collide_share_of(g, ub);
      const size_t first = ((size_t)wf + (I - g.I_lo)) * g.sparts * kRowBlock + (r - I * kRowBlock);
      sweep(part_d2 + first, part_j + first, kRowBlock, (int)(wl - wf + 1) * g.sparts);
    }
    // column side: the row blocks of this launch before this drone's own (each left `sparts` entries per
    // column; a part launch leaves the slots it did not reach marked empty)
    const int Ib = I < g.I_hi + 1 ? I : g.I_hi + 1;
    if (g.sym && Ib > g.I_lo) sweep(cpart_d2 + r, cpart_i + r, (size_t)g.R, (Ib - g.I_lo) * g.sparts);
  }
  sD[q][lr] = best;
  sJ[q][lr] = bj;
  __syncthreads();
  if (q == 0 && r_raw < g.R) {
#pragma unroll
    for (int k = 1; k < kMergeParts; ++k) {
      const double v = sD[k][lr];
      const int j = sJ[k][lr];
      if (j >= 0 && (v < best || (v == best && j < bj))) {
        best = v;
        bj = j;
      }
    }
    if (g.part) {     // one part of a pass: squared minima, folded over the parts by collide_finish_kernel
      min_dist[r] = best;
      partner[r] = bj;
    } else {
      const double dist = sqrt(best);
      min_dist[out] = dist;
      partner[out] = bj;
      hit[out] = (dist < 2.0 * radius) ? 1 : 0;
    }
  }
}

// The parts of a pass folded: minimum over the parts' squared minima (lowest partner wins a tie), distance, hit.
__global__ void __launch_bounds__(256)
collide_finish_kernel(const unsigned char *__restrict__ parts, size_t part_stride, int n_parts, int N, int row_offset,
                      int n_rows, double radius, double *__restrict__ min_dist, int32_t *__restrict__ partner,
                      int32_t *__restrict__ hit) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  const int r = row_offset + i;
  double best = INFINITY;
  int bj = -1;
  for (int p = 0; p < n_parts; ++p) {
    const unsigned char *base = parts + (size_t)p * part_stride;
    const double v = reinterpret_cast<const double *>(base)[r];
    const int j = reinterpret_cast<const int32_t *>(base + (size_t)N * sizeof(double))[r];
    if (j >= 0 && (v < best || (v == best && j < bj))) {
      best = v;
      bj = j;
    }
  }
  const double dist = sqrt(best);
  min_dist[i] = dist;
  partner[i] = bj;
  hit[i] = (dist < 2.0 * radius) ? 1 : 0;
}

// rows [r0, r1) of a part's output marked empty (paths shorter than one sample chunk: the plain kernel fills its rows)
__global__ void __launch_bounds__(256) collide_part_clear_kernel(double *__restrict__ d2, int32_t *__restrict__ pj, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) {
    d2[i] = INFINITY;
    pj[i] = -1;
  }
}

// ------------------------------------------------------------------------------------
// The exact broad phase of a whole-swarm pass (CollideCull above): sort keys, sort, bounds and boxes.
// ------------------------------------------------------------------------------------

// per drone (one wavefront each, four to a workgroup: the drone's S x 3 doubles are one coalesced sweep): the box of its
// finite samples (lo = +inf, hi = -inf when it has none) and the sort key (drone_sort_key).  Only for callers whose
// positions do not come from this library's sampler -- msnap_sample_collide_device computes both while the samples sit
// in its LDS image.
__global__ void __launch_bounds__(kWave * kKeyDrones)
collide_key_kernel(const double *__restrict__ pos, int N, int S, double *__restrict__ box, unsigned *__restrict__ key) {
  const int lane = threadIdx.x & (kWave - 1);
  const int d = blockIdx.x * kKeyDrones + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (d >= N) return;
  const double *p = pos + (size_t)d * S * 3;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int E = S * 3;
  for (int e0 = 0; e0 < E; e0 += 3 * kWave) {
    // three elements per lane and trip, 64 apart: element e is coordinate e % 3, and 64 % 3 == 1
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int e = e0 + q * kWave + lane;
      const double v = e < E ? p[e] : __builtin_nan("");
      const int k = (lane + q) % 3;           // (e0 is a multiple of 3)
      if (__builtin_isfinite(v)) {
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
          if (k == kk) {
            lo[kk] = v < lo[kk] ? v : lo[kk];
            hi[kk] = v > hi[kk] ? v : hi[kk];
          }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = uniform_f64(wave_minmax_f64<false>(lo[k]));
    hi[k] = uniform_f64(wave_minmax_f64<true>(hi[k]));
  }
  if (lane < 3) {
    box[(size_t)d * 6 + lane] = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lo[2];
    box[(size_t)d * 6 + 3 + lane] = lane == 0 ? hi[0] : lane == 1 ? hi[1] : hi[2];
  }
  if (lane == 0) key[d] = drone_sort_key(lo, hi);
}

// The sort, as a rank count spread over the chip: drones are ordered by (key, index) -- all distinct -- so the sorted
// position of drone i is the number of drones below it.  One workgroup of 16 wavefronts per 16 drones: the lanes hold
// the (key << 32 | index) words of ALL drones in registers (wavefront w the w-th sixteenth, up to 8 per lane), the 16
// drones of the tile are wave-uniform: one 64-bit compare per 64 pairs, the count is the population of its lane mask
// (scalar unit), the sixteen wavefronts' counts are added through LDS.  N^2 / 64 vector compares -- 260 k at 4096
// drones -- over 256 workgroups; counting in the lanes (a compare and an add-with-carry per pair, 64 drones per
// workgroup) took 8-10 us, a 78-stage bitonic network in one workgroup 36 us.
// perm[sorted position] = original index.  The kernel is also the pass's first launch: it zeroes the counters the later
// launches add to (survivor totals, per-group item counts and arrivals) and starts every drone's BOUND -- a squared
// distance the drone is known to attain, lowered by the gather tiles with atomic minima -- at +inf, or at 0 for a drone
// without a finite sample (its own result is +inf / -1 whatever is evaluated, it is invisible to the others, and it
// must not keep its group from being culled).
constexpr int kRankWaves = 16;
constexpr int kRankTile = 16;
// kRankKeys (template parameter): words per lane, N / 1024 rounded up to 4, 8 or 16 (kCullMaxDrones)
template <int kRankKeys>
__global__ void __launch_bounds__(kWave * kRankWaves)
collide_rank_kernel(const unsigned *__restrict__ key, int N, int32_t *__restrict__ perm, const double *__restrict__ box,
                    unsigned long long *__restrict__ bound, int32_t *__restrict__ zero, int n_zero,
                    int32_t *__restrict__ meta) {
  __shared__ int cnt[kRankWaves][kRankTile];
  {
    const int gid = blockIdx.x * (kWave * kRankWaves) + threadIdx.x;
    uniform_for<int>(threadIdx.x, n_zero, gridDim.x * (kWave * kRankWaves), [&](int z) { zero[z] = 0; },
                     blockIdx.x * (kWave * kRankWaves));
    if (gid == 0) {      // (the selection adds its survivors)
      meta[kMetaTotal] = 0;
      meta[kMetaGroups] = 0;
    }
  }
  const int lane = threadIdx.x & (kWave - 1), w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int nq = (N + kRankWaves * kWave - 1) / (kRankWaves * kWave);      // words per lane
  // All of a lane's words and the tile's 16 keys are ONE flight of loads (unconditional, clamped addresses; masked
  // afterwards): written with the bounds tests around the loads, every word and every tile key was its own load-and-
  // wait -- 20 dependent round trips, two thirds of the kernel's 7.5 us.  The tile keys travel as one vector load and
  // are handed out with readlane.
  const int i0 = blockIdx.x * kRankTile;
  unsigned kraw[kRankKeys];
#pragma unroll
  for (int q = 0; q < kRankKeys; ++q) {
    const int j = (w * nq + q) * kWave + lane;
    kraw[q] = key[(q < nq && j < N) ? j : 0];
  }
  const unsigned ktile = key[i0 + (lane & (kRankTile - 1)) < N ? i0 + (lane & (kRankTile - 1)) : N - 1];
  // (a tile drone's box travels in the same flight: it only decides where the drone's bound starts)
  double bx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (threadIdx.x < kRankTile && i0 + (int)threadIdx.x < N) {
#pragma unroll
    for (int k = 0; k < 6; ++k) bx[k] = box[(size_t)(i0 + threadIdx.x) * 6 + k];
  }
  unsigned long long mine[kRankKeys];
#pragma unroll
  for (int q = 0; q < kRankKeys; ++q) {
    const int j = (w * nq + q) * kWave + lane;
    mine[q] = (q < nq && j < N) ? ((unsigned long long)kraw[q] << 32) | (unsigned)j : ~0ull;      // (~0: below nothing)
  }
#pragma unroll
  for (int t = 0; t < kRankTile; ++t) {
    const int i = i0 + t < N ? i0 + t : N - 1;      // wave-uniform
    const unsigned long long ki = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)ktile, t) << 32) | (unsigned)i;
    int c = 0;
#pragma unroll
    for (int q = 0; q < kRankKeys; ++q)
      if (q < nq) c += __popcll(__ballot(mine[q] < ki));
    if (lane == 0) cnt[w][t] = c;
  }
  lds_barrier();      // (the zeroing stores above need not have landed)
  if (threadIdx.x < kRankTile && i0 + (int)threadIdx.x < N) {
    int r = 0;
#pragma unroll
    for (int q = 0; q < kRankWaves; ++q) r += cnt[q][threadIdx.x];
    const int i = i0 + threadIdx.x;
    perm[r] = i;
    const bool has = (bx[0] <= bx[3]) & (bx[1] <= bx[4]) & (bx[2] <= bx[5]);
    bound[r] = has ? 0x7ff0000000000000ull : 0ull;
  }
}

// The pass's second launch, three kinds of workgroups behind the sort:
//  * TILES (64 sorted rows x 5 samples, through LDS, as collide_transpose_kernel): the sorted row image
//    [sample][xyz][row] and the sorted drone-major copy from one read of pos through the permutation -- and, while the
//    tile (with the 4 rows behind it) sits in LDS, the drones' BOUNDS: for sorted drone r the minimum over its sorted
//    neighbours r +- 1..4 and the tile's samples of the pass's own squared distance (pair_d2;
//    non-finite samples never win), folded into bound[r] with an atomic minimum on the bit pattern (squared distances
//    are non-negative doubles: ordered like their patterns).  ANY subset of a drone's pair-samples bounds its final
//    minimum from above; with every tile contributing, all samples and the pairs across tile boundaries count.
//  * BOXES: per aligned group of 8 sorted drones the union of their path boxes (the group's bound is the maximum of
//    its drones' bounds, formed by the selection once the atomics are complete).
//  * FILL: the column-side partner slots of the share evaluator marked empty (share path only).
#ifndef MSNAP_TILE_E
#define MSNAP_TILE_E 15      // (tools: A/B builds; 4096 x 91: 33 -> 55.5 us per pass, 24 -> 54.1, 18 -> 53.1, 15 -> 52.7, 12 -> 52.4, 9 -> 52.6)
#endif
constexpr int kTileE = MSNAP_TILE_E, kTileRows = 64, kTileHalo = 4;
constexpr int kTilePitch = kTileE + 1 + (kTileE & 1);      // an odd number of doubles: conflict-free columns (33 -> 35)
static_assert(kTileE % 3 == 0, "whole samples per tile");
constexpr int kBoxGroups = 32;      // groups per BOXES workgroup: 8 lanes each
__global__ void __launch_bounds__(256)
collide_gather_kernel(const double *__restrict__ pos, int N, int Rp, int E, double *__restrict__ prow_t,
                      double *__restrict__ psorted, const int32_t *__restrict__ perm, unsigned long long *__restrict__ bound,
                      const double *__restrict__ box, double *__restrict__ colbox, int nx, int ny, int n_box,
                      int32_t *__restrict__ fill, size_t fill_n) {
#pragma clang fp contract(off)
  __shared__ double tile[(kTileRows + kTileHalo) * kTilePitch];
  __shared__ double sF[kTileHalo][kTileRows];
  const int tid = threadIdx.x;
  const int nb = (int)blockIdx.x - nx * ny;
  if (nb >= n_box) {
    const size_t stride = (size_t)(gridDim.x - nx * ny - n_box) * 256;
    uniform_for<size_t>(tid, fill_n, stride, [&](size_t i) { fill[i] = -1; }, (size_t)(nb - n_box) * 256);
    return;
  }
  if (nb >= 0) {
    const int gq = nb * kBoxGroups + (tid >> 3), r = gq * kColBlock + (tid & 7);
    double g6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) g6[k] = k < 3 ? INFINITY : -INFINITY;
    if (r < N) {
      const double *bx = box + (size_t)perm[r] * 6;
#pragma unroll
      for (int k = 0; k < 6; ++k) g6[k] = bx[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      auto fold = [k](double a, double c) { return k < 3 ? fmin(a, c) : fmax(a, c); };
      g6[k] = fold(g6[k], dpp_f64<0xB1>(g6[k]));      // lane xor 1
      g6[k] = fold(g6[k], dpp_f64<0x4E>(g6[k]));      // lane xor 2
      g6[k] = fold(g6[k], dpp_f64<0x141>(g6[k]));     // mirror inside the half-row of 8
    }
    if ((tid & 7) == 0 && gq * kColBlock < N) {
#pragma unroll
      for (int k = 0; k < 6; ++k) colbox[(size_t)gq * 6 + k] = g6[k];
    }
    return;
  }
  const int bx = blockIdx.x % nx, by = blockIdx.x / nx;
  const int r0 = bx * kTileRows, e0 = by * kTileE;
  const int ne = E - e0 < kTileE ? E - e0 : kTileE;      // whole samples: E and kTileE are multiples of 3
  // the tile's rows of the permutation first (one round trip), then every thread's elements in ONE flight: written as
  // a plain loop each element was permutation load, wait, position load, wait -- eight dependent round trips per thread
  __shared__ int sPerm[kTileRows + kTileHalo];
  if (tid < kTileRows + kTileHalo) sPerm[tid] = perm[r0 + tid < N ? r0 + tid : N - 1];
  __syncthreads();
  constexpr int kElems = (kTileRows + kTileHalo) * kTileE, kPer = (kElems + 255) / 256;
  double val[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int idx = tid + u * 256, i = idx / kTileE, tx = idx - i * kTileE;
    val[u] = (idx < kElems && tx < ne) ? pos[(size_t)sPerm[i] * E + e0 + tx] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int idx = tid + u * 256, i = idx / kTileE, tx = idx - i * kTileE;
    if (idx < kElems) {
      tile[i * kTilePitch + tx] = val[u];
      if (i < kTileRows && tx < ne && r0 + i < N) psorted[(size_t)(r0 + i) * E + e0 + tx] = val[u];
    }
  }
  lds_barrier();      // (not __syncthreads(): that would sit out the round trip of the stores above)
  {
    const int tx = tid & 63, ty = tid >> 6;
    uniform_for<int>(ty, ne, 4, [&](int i) { prow_t[(size_t)(e0 + i) * Rp + r0 + tx] = tile[tx * kTilePitch + i]; });
  }
  {
    // pair (row, row + k) over the tile's samples, one thread each
    const int row = tid & 63, k = (tid >> 6) + 1;
    const double *pa = tile + row * kTilePitch, *pb = tile + (row + k) * kTilePitch;
    double f = INFINITY;
    for (int q = 0; q < ne; q += 3) {
      const double dx = pb[q] - pa[q], dy = pb[q + 1] - pa[q + 1], dz = pb[q + 2] - pa[q + 2];
      f = __builtin_fmin(pair_d2(dx, dy, dz), f);
    }
    sF[k - 1][row] = r0 + row + k < N ? f : INFINITY;      // (rows past the end replay row N - 1)
  }
  lds_barrier();
  if (tid < kTileRows + kTileHalo) {
    // row t of the tile (the halo rows too): its pairs with the rows after it and before it
    double b = INFINITY;
#pragma unroll
    for (int k = 1; k <= kTileHalo; ++k) {
      if (tid < kTileRows) b = __builtin_fmin(b, sF[k - 1][tid]);
      if (tid >= k && tid - k < kTileRows) b = __builtin_fmin(b, sF[k - 1][tid - k]);
    }
    if (b < INFINITY && r0 + tid < N) atomicMin(&bound[r0 + tid], (unsigned long long)__double_as_longlong(b));
  }
}

// what the cost model makes of a pass's survivor counts (the choice the NEXT pass of this swarm takes from the hint)
bool collide_counts_by_groups(const msnap_ctx *ctx, int n_drones, int shares_surviving, int group_pairs_surviving) {
  if (ctx->collide_cull_mode == 1) return false;
  if (n_drones > kCullGroupMaxDrones && 2LL * group_pairs_surviving > kGroupCapLarge) return false;
  if (ctx->collide_cull_mode == 2) return true;
  return cull_groups_cheaper(shares_surviving, group_pairs_surviving);
}

// whether a pass with these arguments runs behind the exact broad phase (which builds its own, spatially sorted, row
// image: a caller-provided one is then not read -- msnap_formation_collide_reads_rows_t)
bool formation_collide_takes_broad_phase(const msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                                         bool no_sym) {
  if (n_samples < kSampleChunk || n_rows != n_cols || row_offset != 0 || ctx->collide_no_cull || no_sym) return false;
  const int cull_min = ctx->collide_cull_min_drones > 0 ? ctx->collide_cull_min_drones : kCullMinDrones;
  return n_rows >= cull_min && n_rows >= 2 * kRowBlock && n_rows <= kCullMaxDrones;
}

// ---- host side: every launcher reads plan -> carve -> launch ----

int launch_collide_transpose(msnap_ctx *ctx, const double *pos, int n_rows, int Rp, int E, double *out, int32_t *fill,
                             size_t fill_n) {
  const int ny = (E + 31) / 32;
  MSNAP_LAUNCH(ctx, collide_transpose_kernel, dim3(Rp / 64, ny + (fill ? 4 : 0)), dim3(256), 0, pos, n_rows, Rp, E, out,
               ny, fill, fill_n, (const int32_t *)nullptr, (double *)nullptr);
  return MSNAP_OK;
}

int launch_collide_keys(msnap_ctx *ctx, const double *pos, int N, int S, double *box, unsigned *key) {
  MSNAP_LAUNCH(ctx, collide_key_kernel, dim3((N + kKeyDrones - 1) / kKeyDrones), dim3(kWave * kKeyDrones), 0, pos, N, S,
               box, key);
  return MSNAP_OK;
}

// A bump carver over ctx->collide_work: take() hands out the next n elements.  With a null base it only counts, so a
// layout written once gives both the size ensure() is asked for and the pointers.
struct Carver {
  char *base;
  size_t off;
  template <class T>
  T *take(size_t n) {
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// the layout run twice: with a null base for the size (and 64 bytes of slack), then over the block
template <class Bufs, class Dims>
static int carve_collide_work(msnap_ctx *ctx, Bufs (*layout)(Carver &, const Dims &), const Dims &d, Bufs &b) {
  Carver sizing{nullptr, 0};
  layout(sizing, d);
  int rc = ensure(ctx, ctx->collide_work, sizing.off + 64);
  if (rc) return rc;
  Carver c{(char *)ctx->collide_work.p, 0};
  b = layout(c, d);
  return MSNAP_OK;
}

// The span path's buffers (doubles, then ints): row image [E][Rp] (none when the sampler handed one over) | row-side
// entries | column-side slots || entries (j) | slots (j)
struct SpanDims {
  size_t t_entries, part_entries, centries;
};
struct SpanBufs {
  double *rows_t, *pd, *cd;
  int32_t *pj, *ci;
};
static SpanBufs span_layout(Carver &c, const SpanDims &d) {      // (a braced list is evaluated left to right)
  return SpanBufs{c.take<double>(d.t_entries),       c.take<double>(d.part_entries), c.take<double>(d.centries),
                  c.take<int32_t>(d.part_entries), c.take<int32_t>(d.centries)};
}

// The broad phase's buffers (doubles, then ints): sorted row image [E][Rp] | sorted columns [N][E] | box [N][6] |
// colbox [nJ][6] | bound [N] | row-side entries | column-side slots | candidates [gcap][16] || entries (j) | slots (j,
// pre-filled -1) | keys [N] | perm [N] | survivor list [shares] | cnt [n_rb] | meta | acnt, astart [nJ] | blist [nJ][nJ]
// (zeroed per pass; the group evaluator's only: blist_n is 0 without it) | glist [gcap] | cand_j [gcap][16]
struct BroadDims {
  size_t Rp, E, N, nJ, entries, centries, gcap, shares, n_rb, blist_n;
};
struct BroadBufs {
  double *rows_t, *psorted, *box_own, *colbox;
  unsigned long long *bound;
  double *pd, *cd, *cand_d2;
  int32_t *pj, *ci;
  unsigned *key_own;
  int32_t *perm, *surv, *cnt, *meta, *acnt, *astart, *blist, *glist, *cand_j;
};
static BroadBufs broad_layout(Carver &c, const BroadDims &d) {
  return BroadBufs{c.take<double>(d.Rp * d.E), c.take<double>(d.N * d.E),  c.take<double>(d.N * 6),
                   c.take<double>(d.nJ * 6),   c.take<unsigned long long>(d.N),
                   c.take<double>(d.entries),  c.take<double>(d.centries), c.take<double>(d.gcap * 16),
                   c.take<int32_t>(d.entries), c.take<int32_t>(d.centries),
                   c.take<unsigned>(d.N),
                   c.take<int32_t>(d.N),       c.take<int32_t>(d.shares),  c.take<int32_t>(d.n_rb),
                   c.take<int32_t>(kMetaWords), c.take<int32_t>(d.nJ),     c.take<int32_t>(d.nJ),
                   c.take<int32_t>(d.blist_n), c.take<int32_t>(d.gcap),    c.take<int32_t>(d.gcap * 16)};
}

// The sequence both span passes end in: the row image of the n_img_rows drone-major rows `rows` (unless the sampler
// handed one over: rows_t_in) -> collide_span_kernel, `waves` shares x sparts -> collide_merge_kernel.  fill_n > 0: the
// transposition also marks the column-side partner slots empty (a part pass).  waves == 0 is the merge of nothing:
// inf / -1 / 0 everywhere.
static int launch_span_merge(msnap_ctx *ctx, const CollideGeom &g, long long waves, const double *rows, int n_img_rows,
                             const double *rows_t_in, const double *pos_cols, const SpanBufs &b, size_t fill_n,
                             double radius, double *min_dist, int32_t *partner, int32_t *hit) {
  if (waves > 0) {
    if (!rows_t_in) {
      int rc = launch_collide_transpose(ctx, rows, n_img_rows, g.Rp, g.S * 3, b.rows_t, fill_n ? b.ci : nullptr, fill_n);
      if (rc) return rc;
    }
    MSNAP_LAUNCH(ctx, collide_span_kernel, dim3((unsigned)(waves * g.sparts)), dim3(kWave), 0,
                 rows_t_in ? rows_t_in : (const double *)b.rows_t, pos_cols, g, b.pd, b.pj, b.cd, b.ci);
  }
  MSNAP_LAUNCH(ctx, collide_merge_kernel, dim3((g.R + kMergeRows - 1) / kMergeRows), dim3(kMergeRows * kMergeParts), 0,
               (const double *)b.pd, (const int32_t *)b.pj, g, (const double *)b.cd, (const int32_t *)b.ci, radius,
               min_dist, partner, hit, (const int32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr);
  return MSNAP_OK;
}

// what a whole pass's planning leaves besides the geometry
struct WholePlan {
  long long upw;          // units per share before the narrowing to CollideGeom's int
  long long slots;        // resident waves: 4 per SIMD
  long long waves;        // shares of the line
  size_t cpart_entries;   // column-side partial entries per sample part
  bool cull;              // the pass runs behind the exact broad phase
};

// The geometry and the share plan of a whole pass (n_cols == 0: nobody to collide with, the plan of nothing).
static WholePlan plan_whole_pass(const msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                                 bool no_sym, CollideGeom &g) {
  WholePlan p{1, (long long)ctx->n_cu * 4 * 4, 0, 0, false};
  g.R = n_rows;
  g.ro = row_offset;
  g.Cn = n_cols;
  g.S = n_samples;
  g.n_rb = (n_rows + kRowBlock - 1) / kRowBlock;
  g.Rp = g.n_rb * kRowBlock;
  g.sparts = 1;
  g.u_lo = 0;
  g.u_n = 0;
  g.I_lo = 0;
  g.I_hi = g.n_rb - 1;
  g.part = 0;
  if (n_cols == 0) {
    g.os = g.oe = 0;
    g.sym = 0;
    g.upw = g.upw_tail = 1;
    g.split = 0;
    g.total = 0;
    return p;
  }
  // the rows are the columns [row_offset, row_offset + n_rows) when that range exists: pairs inside it
  // are evaluated once (unless the column-side partial buffer would be unreasonable)
  const bool rows_in_cols = (long long)row_offset + n_rows <= n_cols;
  g.os = rows_in_cols ? row_offset : n_cols;
  g.oe = rows_in_cols ? row_offset + n_rows : n_cols;
  p.cpart_entries = (size_t)g.n_rb * n_rows;
  // (the column-side partial buffer is bounded at 2 GB: 170 k rows on one GPU; beyond that, and for callers whose
  // rows are not the slice of the columns -- no_sym: "collide_no_sym", or msnap_formation_collide's comparison of its
  // host arrays -- every pair of the range is evaluated from both
  // sides; msnap_get_option("collide_last_sym") reports which way the last pass went)
  g.sym = (rows_in_cols && n_rows > kRowBlock && !no_sym && p.cpart_entries * 12 <= ((size_t)2 << 30)) ? 1 : 0;
  g.upw = 1;
  g.total = collide_ustart(g, g.n_rb);
  g.u_n = g.total;
  // Equal contiguous shares of the line, one 8-column block (x 128 rows) each.  Many small shares beat one
  // share per resident wave: the dispatcher hands the next share to whichever SIMD frees a slot, which
  // evens out the speed differences between SIMDs; shares of 4 columns everywhere lose more to the
  // per-block prologue and fold than they gain (4096 x 91: 288 -> 340 us); a share that ends inside a
  // block pays for the whole block.  "collide_waves_per_cu" (tuning tools) asks for fewer, longer shares.
  long long upw = kColBlock;
  const long long slots = p.slots;
  if (ctx->collide_waves_per_cu > 0) {
    upw = g.total / ((long long)ctx->n_cu * ctx->collide_waves_per_cu) / kColBlock * kColBlock;
    if (upw < kColBlock) upw = kColBlock;
  }
  // the row-side partial buffer holds one 128-row entry per (wave, row block) pair: bound it
  while (((g.total + upw - 1) / upw + g.n_rb) * kRowBlock * 12 > ((long long)512 << 20)) upw *= 2;
  g.upw = (int)upw;
  // A launch that does not even fill the wave slots once (4 per SIMD: <= 2730 drones on one GPU) sends the
  // last quarter of the line out in half-size shares, so that the SIMDs finish within half a share of each
  // other (2048 x 91: 90-95 -> 81-89 us; a shard's rows against all columns -- equal one-sided blocks -- lose by
  // it: 1024 of 4096 rows 109-117 -> 120-133 us, so whole swarms only).  With more shares than slots the dispatcher evens things out by
  // itself and the 4-column blocks only cost (3072: 144 -> 136 us, 4096: 230-250 -> 222-229, 6144: 477-505 -> 448).
  g.upw_tail = (int)upw;
  g.split = (g.total + upw - 1) / upw * upw;
  const long long shares = (g.total + upw - 1) / upw;
  if (upw == kColBlock && ctx->collide_waves_per_cu == 0 && shares <= slots && n_rows == n_cols) {
    g.upw_tail = kColBlock / 2;
    g.split = shares * 3 / 4 * upw;
  } else if (upw == kColBlock && ctx->collide_waves_per_cu == 0 && shares % slots != 0 && shares % slots <= slots / 8) {
    // a few shares more than whole rounds of the slots (4096 drones: 8448 on 4096): left whole they would run
    // as a last round of their own; as 2-column shares they are one short round spread over all SIMDs
    // (4096 x 91: 217 -> 207 us; with 704 of 4800 shares beyond the round at 3072 drones the 2-column blocks
    // cost more than they even out: 136 -> 153 us, hence the limit of an eighth of the slots)
    g.upw_tail = 2;
    g.split = (shares - shares % slots) * upw;
  }
  p.upw = upw;
  p.waves = g.split / upw + (g.total - g.split + g.upw_tail - 1) / g.upw_tail;
  // the exact broad phase (CollideCull): a whole swarm, sorted on the GPU
  // (below some 3000 drones the six small launches in front of the pass cost more than a sparse swarm saves:
  // 2048 x 91 dense 91 -> 121 us, sparse 92 -> 84; 4096 x 91 dense 243 -> 282, sparse 243 -> 122, the formation
  // fixture 243 -> 105)
  p.cull = g.sym && formation_collide_takes_broad_phase(ctx, n_rows, row_offset, n_cols, n_samples, no_sym);
  if (p.cull) return p;
  // A small launch (a small swarm, or one of many shards) is as long as ONE share takes -- 16 sample chunks x 8
  // columns are one dependent chain of scalar fetches, 43 us at 512 drones whatever the arithmetic.  While the
  // shares do not fill a quarter of the wave slots (half-full launches lose: 512 of 4096 rows 71 -> 84 us), each
  // is taken by 2, 4 or 8 waves with a range of the sample chunks each (narrower column blocks instead would repeat the row loads per block: 1024 drones 46 -> 59 us).
  if (ctx->collide_sample_parts > 0) {
    g.sparts = ctx->collide_sample_parts < 8 ? ctx->collide_sample_parts : 8;
  } else if (ctx->collide_waves_per_cu == 0) {
    const int nch = (n_samples + kSampleChunk - 1) / kSampleChunk;      // (the unrounded count, on purpose: not pair_tile_chunks)
    while (g.sparts < 8 && p.waves * g.sparts < slots / 4 && nch / (g.sparts * 2) >= 2) g.sparts *= 2;
  }
  return p;
}

// A whole pass behind the exact broad phase.
// Launches: [key, unless the sampler left boxes and keys] -> rank -> gather -> select -> evaluator -> fold, the last
// two either
//   * the surviving GROUP PAIRS (8 x 8 drones) and the per-group fold of their candidates, or
//   * the surviving SHARES (128 x 8) and the merge of their entries.
// Which one is a HOST decision (the launch sequences differ): "collide_cull_mode" 1 / 2 force it; otherwise the
// survivor counts the previous pass of this context left in page-locked memory (cull_hint_pack; read without
// synchronising, so possibly a few passes old) are put through the cost model, and a pass without such a hint
// for its swarm size takes the shares.  Both evaluators are exact; the choice only moves time.
static int launch_broad_phase(msnap_ctx *ctx, const CollideGeom &g, long long slots, const double *pos_cols,
                              const double *rows_t_in, double radius, double *min_dist, int32_t *partner,
                              int32_t *hit) {
  const int N = g.R, n_samples = g.S, E = n_samples * 3;
  const size_t nJ = ((size_t)N + kColBlock - 1) / kColBlock;
  long long shares = 0;
  for (int I = 0; I < g.n_rb; ++I) shares += (N - I * kRowBlock + kColBlock - 1) / kColBlock;
  const long long all_groups = (long long)nJ * (nJ + 1) / 2;
  // Up to kCullGroupMaxDrones every group pair has a list slot; larger swarms get kGroupCapLarge slots and BOTH
  // evaluators are launched -- the share evaluator and its merge return at once unless the survivors overflowed the
  // list (then the group evaluator did nothing and the group fold only cleared the reverse-list entries the selection
  // wrote for the first kGroupCapLarge items): two empty launches on a pass of a quarter millisecond.
  const bool all_fit = N <= kCullGroupMaxDrones;
  bool by_groups = false;
  if (ctx->collide_cull_mode == 2) {
    by_groups = true;
  } else if (ctx->collide_cull_mode != 1 && ctx->cull_hint) {
    const unsigned long long h = *(volatile unsigned long long *)ctx->cull_hint;
    const int hN = (int)(h >> 48) & 0x7fff;
    const long long hs = (long long)((h >> 24) & 0xffffff), hg = (long long)(h & 0xffffff);
    by_groups = h != 0 && hN == (N & 0x7fff) && hg != 0xffffff && cull_groups_cheaper(hs, hg) &&
                (all_fit || 2 * hg <= kGroupCapLarge);
  }
  const bool both = by_groups && !all_fit;
  // sample parts a share may be cut into: the column-side slots are n_rb x spmax x N entries, pre-filled per call
  const int spmax = N > 8192 ? 2 : kCullMaxParts;
  ctx->collide_last_shares = (int)shares;
  const int sp_force = (ctx->collide_sample_parts > 0 ? (ctx->collide_sample_parts < spmax ? ctx->collide_sample_parts : spmax) : 0) |
                       (spmax << 8);
  // share evaluator: row-side entries, one per item (cull_split cuts shares only while the items stay below twice the
  // wave slots), column-side slots.  Group evaluator: list, 16 candidate slots per item, reverse lists
  const long long items_max = (sp_force & 0xff) ? shares * (sp_force & 0xff) : (shares > 2 * slots ? shares : 2 * slots);
  const size_t entries = (by_groups && !both) ? 0 : (size_t)items_max * kRowBlock;
  const size_t centries = (by_groups && !both) ? 0 : (size_t)g.n_rb * spmax * N;
  const size_t gcap = !by_groups ? 0 : all_fit ? (size_t)all_groups : (size_t)kGroupCapLarge;
  // the sampler's hand-over (msnap_sample_collide_device: boxes [N][6], then keys [N]) saves the key launch -- when
  // the sampler wrote it beside these positions
  const bool have_keys = handover_form(ctx, rows_t_in, pos_cols, N, n_samples) == 2;
  BroadBufs b;
  int rc = carve_collide_work(ctx, broad_layout,
                              BroadDims{(size_t)g.Rp, (size_t)E, (size_t)N, nJ, entries, centries, gcap, (size_t)shares,
                                        (size_t)g.n_rb, by_groups ? nJ * nJ : 0},
                              b);
  if (rc) return rc;
  const double *box = have_keys ? rows_t_in : b.box_own;
  const unsigned *key = have_keys ? reinterpret_cast<const unsigned *>(rows_t_in + (size_t)N * 6) : b.key_own;
  CullGroups cg{b.glist, b.astart, b.acnt, b.blist, b.cand_d2, b.cand_j, (int)gcap, (int)nJ};
  // the reverse lists are all-zero between passes (the fold zeroes what it read, also when the list overflowed and
  // the share evaluator ran behind it -- the `both` launch of a larger swarm): they are cleared only when this
  // block has held something else since -- another layout, another evaluator, any other pass of the context -- and,
  // so that a graph replays whatever ran between its replays, always under stream capture
  // (nor is a block trusted that a graph may replay on between two eager passes)
  const bool trust = by_groups && !stream_is_capturing(ctx) && !ctx->collide_work.in_graph;
  const bool blist_clean = trust && ctx->blist_clean == (const void *)b.blist && ctx->blist_clean_n == (int)nJ;
  ctx->blist_clean = trust ? (const void *)b.blist : nullptr;
  ctx->blist_clean_n = (int)nJ;
  // (what the last pass did: the broad-phase fields are set together, once its buffer exists)
  ctx->collide_meta = b.meta;
  ctx->collide_last_cull = 1;
  ctx->collide_last_by_groups = by_groups ? (all_fit ? 1 : 2) : 0;      // (2: while the survivors fit kGroupCapLarge)
  ctx->collide_last_n = N;
  ctx->collide_last_handover = have_keys ? 2 : 0;
  if (!have_keys) {
    rc = launch_collide_keys(ctx, pos_cols, N, n_samples, b.box_own, b.key_own);
    if (rc) return rc;
  }
  MSNAP_LAUNCH(ctx, (N <= 4096 ? collide_rank_kernel<4> : N <= 8192 ? collide_rank_kernel<8> : collide_rank_kernel<16>),
               dim3((N + kRankTile - 1) / kRankTile), dim3(kWave * kRankWaves), 0, key, N, b.perm, box, b.bound, b.blist,
               (int)(by_groups && !blist_clean ? nJ * nJ : 0), b.meta);
  const int nx = g.Rp / kTileRows, ny = (E + kTileE - 1) / kTileE;
  const int n_box = (int)((nJ + kBoxGroups - 1) / kBoxGroups), n_fill = centries ? 4 * nx : 0;
  MSNAP_LAUNCH(ctx, collide_gather_kernel, dim3((unsigned)(nx * ny + n_box + n_fill)), dim3(256), 0, pos_cols, N, g.Rp, E,
               b.rows_t, b.psorted, (const int32_t *)b.perm, b.bound, box, b.colbox, nx, ny, n_box, b.ci, centries);
  CollideCull cu{b.colbox};
  MSNAP_LAUNCH(ctx, (N <= kCullGroupMaxDrones ? collide_select_kernel<1> : collide_select_kernel<2>),
               dim3(g.n_rb + (unsigned)((nJ + kSelGroups - 1) / kSelGroups)), dim3(kSelThreads), 0, N, g.n_rb, cu,
               (const double *)b.bound, b.surv, b.cnt, b.meta, cg);
  if (by_groups) {
    MSNAP_LAUNCH(ctx, collide_eval_groups_kernel, dim3((unsigned)(ctx->n_cu * 4 * kGroupWaves)), dim3(kWave), 0,
                 (const double *)b.psorted, N, n_samples, (const int32_t *)b.perm, (const int32_t *)b.meta, cg,
                 ctx->cull_hint);
    MSNAP_LAUNCH(ctx, (N <= 4096 ? collide_finish_groups_kernel<8> : N <= 8192 ? collide_finish_groups_kernel<16> : collide_finish_groups_kernel<32>),
                 dim3((unsigned)((nJ + kFinishWaves - 1) / kFinishWaves)), dim3(kWave * kFinishWaves), 0, N,
                 (const int32_t *)b.perm, (const int32_t *)b.meta, cg, radius, min_dist, partner, hit);
    if (!both) return MSNAP_OK;
  }
  MSNAP_LAUNCH(ctx, collide_eval_shares_kernel, dim3((unsigned)slots), dim3(kWave), 0, (const double *)b.rows_t,
               (const double *)b.psorted, g, b.pd, b.pj, b.cd, b.ci, (const int32_t *)b.perm, (const int32_t *)b.surv,
               sp_force, (int)slots, b.meta, ctx->cull_hint, both ? (int)gcap : 0);
  MSNAP_LAUNCH(ctx, collide_merge_kernel, dim3((N + kMergeRows - 1) / kMergeRows), dim3(kMergeRows * kMergeParts), 0, b.pd,
               b.pj, g, b.cd, b.ci, radius, min_dist, partner, hit, (const int32_t *)b.perm, (const int32_t *)b.cnt,
               (const int32_t *)b.meta, both ? (int)gcap : 0);
  return MSNAP_OK;
}

// `rows_t`: the rows' transposed image [n_samples][3][row pitch] when the caller already has it (the sampler's
// second output, msnap_sample_collide); nullptr: built here from pos_rows
int launch_formation_collide(msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                             const double *pos_rows, const double *pos_cols, double radius, double *min_dist,
                             int32_t *partner, int32_t *hit, const double *rows_t_in, bool no_sym) {
  ctx->collide_last_handover = 0;
  if (n_cols > 0 && n_samples < kSampleChunk) {
    MSNAP_LAUNCH(ctx, collide_short_kernel, dim3((n_rows + kWave - 1) / kWave), dim3(kWave), 0, pos_rows, pos_cols,
                 n_rows, row_offset, n_cols, n_samples, radius, min_dist, partner, hit, 0);
    return MSNAP_OK;
  }
  CollideGeom g;
  const WholePlan p = plan_whole_pass(ctx, n_rows, row_offset, n_cols, n_samples, no_sym, g);
  // nobody to collide with: the merge of nothing writes inf / -1 / 0
  if (n_cols == 0)
    return launch_span_merge(ctx, g, 0, nullptr, 0, nullptr, nullptr, SpanBufs{}, 0, radius, min_dist, partner, hit);
  ctx->collide_last_sym = g.sym;
  // (what the last pass did: launch_broad_phase sets its fields once its buffer exists)
  ctx->collide_last_cull = 0;
  ctx->collide_meta = nullptr;
  ctx->collide_last_shares = (int)(p.waves < 0x7fffffff ? p.waves : 0x7fffffff);
  if (p.cull) return launch_broad_phase(ctx, g, p.slots, pos_cols, rows_t_in, radius, min_dist, partner, hit);
  // (a row image is only what the sampler's record says it is: a hand-over in the keys form -- written for a whole-
  // swarm pass that, by the options now in force, is not taken --, for other rows or other positions, or not on
  // record is not one)
  if (handover_form(ctx, rows_t_in, pos_rows, n_rows, n_samples) != 1) rows_t_in = nullptr;
  ctx->collide_last_handover = rows_t_in ? 1 : 0;
  if (p.upw > 0x3fffffff || p.waves * g.sparts > 0x7fffffff) return MSNAP_EINVAL;
  const size_t part_entries = ((size_t)p.waves + g.n_rb) * g.sparts * kRowBlock;
  const size_t centries = g.sym ? p.cpart_entries * g.sparts : 0;
  const size_t t_entries = rows_t_in ? 0 : (size_t)g.Rp * n_samples * 3;
  ctx->blist_clean = nullptr;      // (the block is about to hold this pass's buffers)
  SpanBufs b;
  int rc = carve_collide_work(ctx, span_layout, SpanDims{t_entries, part_entries, centries}, b);
  if (rc) return rc;
  return launch_span_merge(ctx, g, p.waves, pos_rows, n_rows, rows_t_in, pos_cols, b, 0, radius, min_dist, partner, hit);
}

// The geometry and the share plan of part `part` of `n_parts` (n_samples >= kSampleChunk): it walks the units
// [total * p / P, total * (p + 1) / P) of the whole swarm's line, the cuts rounded to whole 8-column blocks.  Returns
// the part's shares (0: an empty part, the plan of nothing) and leaves the row blocks it touches in `nrb`.
static long long plan_part_pass(const msnap_ctx *ctx, int N, int n_samples, int part, int n_parts, CollideGeom &g,
                                int &nrb) {
  g.R = N;
  g.ro = 0;
  g.Cn = N;
  g.S = n_samples;
  g.n_rb = (N + kRowBlock - 1) / kRowBlock;
  g.os = 0;
  g.oe = N;
  g.sym = 1;
  g.total = collide_ustart(g, g.n_rb);
  auto cut = [&](int p) {
    const long long u = g.total * p / n_parts / kColBlock * kColBlock;
    return p >= n_parts ? g.total : u;
  };
  g.u_lo = cut(part);
  g.u_n = cut(part + 1) - g.u_lo;
  g.part = 1;
  g.sparts = 1;
  g.upw = g.upw_tail = kColBlock;
  g.I_lo = 0;
  g.I_hi = -1;
  const long long shares = (g.u_n + kColBlock - 1) / kColBlock;
  g.split = shares * kColBlock;
  long long waves = shares;
  if (shares > 0) {
    const long long u0 = g.u_lo, u1 = g.u_lo + g.u_n - 1;
    while (g.I_lo + 1 < g.n_rb && collide_ustart(g, g.I_lo + 1) <= u0) ++g.I_lo;
    g.I_hi = g.I_lo;
    while (g.I_hi + 1 < g.n_rb && collide_ustart(g, g.I_hi + 1) <= u1) ++g.I_hi;
    // Filling the wave slots (4 per SIMD) ONCE is what a part launch is tuned for -- nothing refills a slot that
    // frees early, and a launch that exceeds the slots by a few shares runs those as a round of their own
    // (4096 x 91 in two parts: 4224 shares on 4096 slots took 133 us against 112 for half of the single launch).
    //  * fewer shares than slots: every share is taken by floor(slots / shares) waves, each a range of the sample
    //    chunks (a share alone is one chain of 16 x 8 dependent fetches; an eighth of the 4096-drone line,
    //    1056 shares, span kernel alone / merge under rocprofv3: 54 / 8 us whole, 43 / 11 in halves, 40 / 17 in
    //    quarters -- 4224 waves, 128 of them queued -- 46 / 31 in eighths; every split multiplies the partial
    //    entries the merge sweeps)
    //  * a few shares more than whole rounds of the slots: the excess goes out as 2-column shares (the whole-pass
    //    rule above)
    const long long slots = (long long)ctx->n_cu * 4 * 4;
    const int nch = (n_samples + kSampleChunk - 1) / kSampleChunk;      // (the unrounded count, on purpose: not pair_tile_chunks)
    if (ctx->collide_sample_parts > 0) {
      g.sparts = ctx->collide_sample_parts < 8 ? ctx->collide_sample_parts : 8;
    } else if (shares * 2 <= slots) {
      long long sp = slots / shares;
      sp = sp > 8 ? 8 : sp;
      while (sp > 1 && nch / sp < 2) --sp;
      g.sparts = (int)sp;
    } else if (shares % slots != 0 && shares % slots <= slots / 8 && shares > slots) {
      g.upw_tail = 2;
      g.split = (shares - shares % slots) * kColBlock;
    }
    waves = g.split / kColBlock + (g.u_n - g.split + g.upw_tail - 1) / g.upw_tail;
  }
  nrb = g.I_hi - g.I_lo + 1;                 // row blocks this part touches (0: an empty part)
  g.Rp = (nrb > 0 ? nrb : 1) * kRowBlock;
  if (waves == 0) g.total = 0;   // the merge of nothing: +inf / -1 everywhere
  return waves;
}

// One rank's part of the pass over the WHOLE swarm: every unordered pair of the swarm is a (row block, column)
// unit of one triangular line -- the line a single-GPU launch walks -- and part p of P takes the p-th of P equal
// contiguous ranges of its 8-column shares.  It evaluates each of its pairs once, credits both drones, and leaves
// the squared minimum and partner of EVERY drone (+inf / -1 where it met none of the drone's pairs) in
// out_d2 [N] / out_j [N]; collide_finish_kernel folds the P parts.
int launch_formation_collide_part(msnap_ctx *ctx, int N, int n_samples, const double *pos_all, int part, int n_parts,
                                  double *out_d2, int32_t *out_j) {
  if (n_samples < kSampleChunk) {
    // short paths: the plain kernel on the part's block of rows, one-sidedly against all columns
    const int r0 = (int)((long long)N * part / n_parts), r1 = (int)((long long)N * (part + 1) / n_parts);
    MSNAP_LAUNCH(ctx, collide_part_clear_kernel, dim3((N + 255) / 256), dim3(256), 0, out_d2, out_j, N);
    if (r1 > r0)
      MSNAP_LAUNCH(ctx, collide_short_kernel, dim3((r1 - r0 + kWave - 1) / kWave), dim3(kWave), 0,
                   pos_all + (size_t)r0 * n_samples * 3, pos_all, r1 - r0, r0, N, n_samples, 0.0, out_d2 + r0, out_j + r0,
                   (int32_t *)nullptr, 1);
    return MSNAP_OK;
  }
  CollideGeom g;
  int nrb;
  const long long waves = plan_part_pass(ctx, N, n_samples, part, n_parts, g, nrb);
  if (waves * g.sparts > 0x7fffffff) return MSNAP_EINVAL;
  const size_t part_entries = ((size_t)waves + (size_t)(nrb > 0 ? nrb : 0)) * g.sparts * kRowBlock;
  const size_t centries = (size_t)(nrb > 0 ? nrb : 0) * g.sparts * (size_t)N;
  const int E = n_samples * 3;
  const size_t t_entries = (size_t)g.Rp * E;
  if ((part_entries + centries) * 12 > ((size_t)16 << 30)) return MSNAP_ENOMEM;
  ctx->collide_last_cull = 0;      // (the buffer the last broad-phase pass left its counts in is reused)
  ctx->collide_last_handover = 0;
  ctx->collide_meta = nullptr;
  ctx->blist_clean = nullptr;      // (the block is about to hold this pass's buffers)
  SpanBufs b;
  int rc = carve_collide_work(ctx, span_layout, SpanDims{t_entries, part_entries, centries}, b);
  if (rc) return rc;
  const int r_first = g.I_lo * kRowBlock;
  const int r_cnt = (N - r_first) < g.Rp ? (N - r_first) : g.Rp;
  return launch_span_merge(ctx, g, waves, pos_all + (size_t)r_first * E, r_cnt, nullptr, pos_all, b, centries, 0.0,
                           out_d2, out_j, nullptr);
}

int launch_formation_collide_finish(msnap_ctx *ctx, int N, int n_parts, const void *parts, size_t part_stride,
                                    int row_offset, int n_rows, double radius, double *min_dist, int32_t *partner,
                                    int32_t *hit) {
  MSNAP_LAUNCH(ctx, collide_finish_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (const unsigned char *)parts,
               part_stride, n_parts, N, row_offset, n_rows, radius, min_dist, partner, hit);
  return MSNAP_OK;
}

}  // namespace msnap
