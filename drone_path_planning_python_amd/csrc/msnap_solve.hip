// K1 -- batched minimum-snap solve, one lane per (drone, axis), gfx950.
//
// Replaces calculate_trajectory1D / calculate_trajectory4D
// (reference src/optimizations/calculatingTrajectories.py:37-213) for a batch.
//
// Algorithm (DESIGN.md "K1"): the reference's square 8M x 8M collocation system
// has the unique solution of the minimum-snap QP.  Writing every segment in
// Hermite form (endpoint position + k-1 derivatives, k = 4 for order 7)
// satisfies the waypoint, endpoint and C^1..C^(k-1) rows identically; the
// remaining rows (continuity of d^k..d^(2k-2), calculatingTrajectories.py:115-119)
// are, up to sign, the stationarity conditions dJ/d(d_i[n]) = 0 of the snap
// cost J = sum_seg T^-(2k-1) e^T H e.  That reduced KKT system is symmetric
// positive definite and block tridiagonal with (k-1) x (k-1) blocks:
//     O_{i-1}^T u_{i-1} + D_i u_i + O_i u_{i+1} = r_i ,   i = 1..M-1
//     D_i = T_{i-1}^(n+m-K) HEE + T_i^(n+m-K) HSS ,  O_i = T_i^(n+m-K) HSE
// It is solved by a block LDL^T sweep (forward: S_i, G_i = S_i^-1 O_i,
// z_i = S_i^-1 y_i; backward: u_i = z_i - G_i u_{i+1}) and each segment's
// monomial coefficients are recovered from its two endpoint states with the
// constant matrices CS / CE.
//
// Mapping: lane = 4*dl + axis; a wavefront carries 16 drones.  The matrix part
// (S_i, G_i) depends on the time grid only and is recomputed by the 4 axis
// lanes of a drone (no cross-lane traffic, no divergence: every lane runs the
// same M-step recurrence).  The tile's inputs are staged in LDS by one
// coalesced sweep.  The variants share the arithmetic (Sweep<K>::knot_geom / chain, recover_segment)
// and are chosen per launch by plan_solve (msnap_solve_plan.h), which launch_solve_k carries out:
//   solve_kernel_twist<K,H,M>  2 <= n_seg <= 24 (order 7) / 12 (order 9), batch up to one 8-drone
//                              wavefront per SIMD: two-sided sweep (halves the dependent chain)
//                              meeting at a shared knot, one straight-line instance per
//                              (order, n_seg)                                (latency path)
//   solve_kernel_reg<K,10|20>  n_seg <= 20: knot loops unrolled, path data and z_i in
//                              registers, G_i in LDS, persistent waves with cross-tile
//                              input prefetch                               (throughput path)
//   solve_kernel<K, false>     any n_seg whose stash fits 160 KiB: rolled loops, LDS stash
//   solve_kernel<K, true>      longer paths: stash on a global scratch slab
#include "msnap_consts.h"
#include <cstdlib>

#include "msnap_internal.h"
#include "msnap_dispatch.h"
#include "msnap_sweep.h"
#include "msnap_rolled.h"

namespace msnap {


// ------------------------------------------------------------------------------------
// generic variant: rolled loops, G_i / z_i stashed in LDS (GS = false) or on a global slab (GS = true).  The solve
// of a tile is rolled_solve_tile (msnap_rolled.h), shared with the boundary-state solve of msnap_states.hip; here
// are the layout and the tile loop.
// ------------------------------------------------------------------------------------
template <int K, bool GS>
__global__ void __launch_bounds__(kWave)
solve_kernel(const double *__restrict__ wp, const double *__restrict__ tt, int shared_times,
             int N, int M, double *__restrict__ coef, double *__restrict__ dur,
             int32_t *__restrict__ status, double *__restrict__ gscratch, int ntiles) {
  constexpr int NU = K - 1, NC = 2 * K;

  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int lane = threadIdx.x;
  const int knots = M - 1;
  const int wpitch = (M + 1) * 4;
  const int tpitch = M + 1;

  // LDS: output transpose image Tr[NC/2][68] (16-B slots) | then, LDS variant only,
  //      inputs Wraw[16][(M+1)*4] | Traw[16][M+1]
  // stash (LDS or global slab): X[M][16] | G[knots][NU*NU][16] | Z[knots][NU][64]
  RolledTile p;
  p.sWraw = lds + (NC / 2) * kTrPitch * 2;
  p.sTraw = p.sWraw + 16 * wpitch;
  if constexpr (GS) {
    p.sX = gscratch + (size_t)blockIdx.x * (size_t)(16 * M + 16 * NU * NU * knots + 64 * NU * knots);
  } else {
    p.sX = p.sTraw + 16 * tpitch;
  }
  p.sG = p.sX + 16 * M;
  p.sZ = p.sG + 16 * NU * NU * knots;
  p.sS0 = p.sS1 = nullptr;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int left = N - tile * kDronesPerWave;
    const int nvalid = left < kDronesPerWave ? left : kDronesPerWave;
    if constexpr (!GS) {
      if (tile != (int)blockIdx.x) __syncthreads();  // LDS is reused by this block's next tile
      stage_inputs(wp, tt, shared_times, tile, nvalid, wpitch, tpitch, p.sWraw, p.sTraw, lane);
      __syncthreads();
      store_durations(p.sTraw, shared_times, tpitch, M, nvalid, lane, dur + (size_t)tile * kDronesPerWave * M);
    }
    rolled_solve_tile<K, GS, false>(p, wp, tt, shared_times, false, false, M, tile, nvalid, lane, coef, dur, status);
  }
}

// ------------------------------------------------------------------------------------
// fast variant for n_seg <= MAXM: knot loops unrolled, z_i in registers, G_i in LDS.
// LDS per wave = inputs + 1/T + G  (18.7 KB at n_seg = 10, order 7) -> 8 waves / CU.
// ------------------------------------------------------------------------------------
template <int K, int MAXM>
__global__ void __launch_bounds__(kWave, ((K <= 4 && MAXM <= 10) ? 2 : 1))   // order 9 / 20 segments need > 256 VGPRs
solve_kernel_reg(const double *__restrict__ wp, const double *__restrict__ tt, int shared_times,
                 int N, int M, double *__restrict__ coef, double *__restrict__ dur,
                 int32_t *__restrict__ status, int ntiles) {
  using SW = Sweep<K>;
  constexpr int NU = SW::NU, NC = SW::NC;

  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int lane = threadIdx.x;
  const int dl = lane >> 2;
  const int a = lane & 3;
  const int wpitch = (M + 1) * 4;
  const int tpitch = M + 1;
  // LDS: [ inputs Wraw | Traw ] -- dead after the forward sweep, then reused as the output
  //      transpose image -- followed by G[M-2][NU*NU][16] (G of the last knot is never read)
  double *sWraw = lds;
  double *sTraw = sWraw + 16 * wpitch;
  double2 *sTr = reinterpret_cast<double2 *>(lds);
  const int in_words = 16 * wpitch + 16 * tpitch;
  const int tr_words = (NC / 2) * kTrPitch * 2;
  double *sG = lds + (in_words > tr_words ? in_words : tr_words);

  auto tile_valid = [&](int tl) {
    const int left = N - tl * kDronesPerWave;
    return left < kDronesPerWave ? left : kDronesPerWave;
  };
  StageRegsAsm<MAXM> pre;
  if ((int)blockIdx.x < ntiles)
    stage_load_asm(wp, tt, shared_times, blockIdx.x, tile_valid(blockIdx.x), wpitch, tpitch, lane, pre);
  wait_vmcnt<0>();   // the first tile's inputs (nothing to overlap them with)
  // Prefetch distance: the next tile's inputs are requested two segments before the end of the
  // backward sweep, when most of this tile's registers are dead.  (Requesting them right after the
  // forward sweep hides more latency on paper but measured 4 % slower at saturation)
  // The wait at the top of a tile leaves the 2 x kStoresPerSeg stores of the two segments issued after the
  // loads in flight (this kernel is launched for n_seg >= 2 only, so both always run and the immediate is a
  // constant; waiting for the first of the two segments' stores as well costs 6 % at 65 536 x 10, order 9).
  // tools/check_prefetch_isa.py counts the stores on every path of the code object; the multi-tile tests
  // of tests/test_solve_gpu.py compare a persistent wave's tiles with the same tiles solved alone.
  constexpr int kStoresPerSeg = (NC == 8 ? 4 : NC / 2);

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int d_raw = tile * kDronesPerWave + dl;
    const bool live = d_raw < N;
    const int d = live ? d_raw : N - 1;
    const int nvalid = tile_valid(tile);
    const int next = tile + gridDim.x;

    // tile top: a marker instruction for tools/check_prefetch_isa.py (priority 0 is the default: no effect)
    asm volatile("s_setprio 0" ::: "memory");
    wave_lds_fence();   // the previous tile's LDS reads are done (in-order LDS, one wave)
    stage_wait_asm<MAXM, 2 * kStoresPerSeg>(pre);
    stage_store_asm(shared_times, nvalid, wpitch, tpitch, sWraw, sTraw, lane, pre);
    wave_lds_fence();
    store_durations(sTraw, shared_times, tpitch, M, nvalid, lane, dur + (size_t)tile * kDronesPerWave * M);
    const int dloc = live ? dl : (N - 1 - tile * kDronesPerWave);
    const double *lw = sWraw + dloc * wpitch + a;
    const double *lt = sTraw + (shared_times ? 0 : dloc * tpitch);

    // per-lane copies of the path: waypoints, segment lengths and their reciprocals stay in
    // registers for the backward sweep (knot loops are unrolled, so the indices are static)
    double wreg[MAXM + 1], xreg[MAXM], zreg[MAXM > 1 ? MAXM - 1 : 1][NU];

    const double t0 = lt[0];
    double tcur = lt[1];
    wreg[0] = lw[0];
    wreg[1] = lw[4];
    bool nonfinite = !(finite64(t0) & finite64(tcur) & finite64(wreg[0]) & finite64(wreg[1]));
    const double T0 = tcur - t0;
    const double T0q = T0 - t0;   // Appendix-A quirk: segment 0 has length T_0 - t0 in s - t0
    bool badtime = !(T0 > 0.0) | !(T0q > 0.0) | (t0 < 0.0);
    xreg[0] = rcp64(T0q);
    SW sw;
    sw.init(xreg[0], wreg[1] - wreg[0]);

    double tpre = lt[M >= 2 ? 2 : M];
    double wpre = lw[(M >= 2 ? 2 : M) * 4];
#pragma unroll
    for (int i = 1; i < MAXM; ++i) {
      if (i < M) {
        const double tnext = tpre;
        wreg[i + 1] = wpre;
        {
          const int ip = (i + 2 <= M) ? i + 2 : M;
          tpre = lt[ip];
          wpre = lw[ip * 4];
        }
        nonfinite |= !finite64(tnext) | !finite64(wreg[i + 1]);
        const double Ti = tnext - tcur;
        badtime |= !(Ti > 0.0);
        xreg[i] = rcp64(Ti);
        double G[NU][NU], z[NU];
        sw.step(xreg[i], wreg[i + 1] - wreg[i], G, z);
        {   // the checks of this knot settled here, in one register: left as booleans the compares are sunk behind the
            // sweep and every |w|, T and pivot waits for them in registers (see solve_kernel_twin)
          int f = (nonfinite ? 4 : 0) | (badtime ? 2 : 0) | (sw.singular ? 1 : 0);
          asm volatile("" : "+v"(f));
          nonfinite = (f & 4) != 0;
          badtime = (f & 2) != 0;
          sw.singular = (f & 1) != 0;
        }
        if (i < M - 1) {
          double *g = sG + (i - 1) * (NU * NU * 16) + dl;
#pragma unroll
          for (int r = 0; r < NU; ++r)
#pragma unroll
            for (int c = 0; c < NU; ++c) g[(r * NU + c) * 16] = G[r][c];
        }
#pragma unroll
        for (int r = 0; r < NU; ++r) zreg[i - 1][r] = z[r];
        tcur = tnext;
      }
    }

    const int st = drone_status(nonfinite, badtime, sw.singular);
    if (live && a == 0) status[d] = st;
    const bool bad = st != 0;

    // ---------------- backward sweep + recovery: registers + one G block per knot ----------------
    double un[NU], gq[NU][NU];
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      un[r] = 0.0;
#pragma unroll
      for (int c = 0; c < NU; ++c) gq[r][c] = 0.0;
    }
#pragma unroll
    for (int i = MAXM - 1; i >= 0; --i) {
      if (i == (MAXM >= 2 ? 1 : 0)) {
        // software pipelining across tiles: with two segments left most of this tile's registers
        // are dead, so the next tile's inputs start their trip from HBM now.  Unconditional
        // (clamped to the last tile) and at a static point of the unrolled loop: a conditional
        // definition would keep `pre` live -- and spilled -- across the whole tile.
        __builtin_amdgcn_sched_barrier(0);
        const int nx = next < ntiles ? next : ntiles - 1;
        stage_load_asm(wp, tt, shared_times, nx, tile_valid(nx), wpitch, tpitch, lane, pre);
      }
      if (i <= 1 || i < M) {   // n_seg >= 2 (launch_solve_k): segments 0 and 1 always exist
        double u[NU];
#pragma unroll
        for (int r = 0; r < NU; ++r) {
          double v = (i >= 1) ? zreg[i >= 1 ? i - 1 : 0][r] : 0.0;
          if (i >= 1) {
            // at the last knot (i == M - 1, the first iteration that runs) gq and un are still zero and
            // the products add -0.0: bitwise z itself, without a select on the runtime segment count
#pragma unroll
            for (int c = 0; c < NU; ++c) v = __builtin_fma(-gq[r][c], un[c], v);
          }
          u[r] = v;
        }
        if (i >= 2) {   // G of knot i-1 (slot i-2), used by the next iteration (i-1 < M-1 always)
          const double *g = sG + (i - 2) * (NU * NU * 16) + dl;
#pragma unroll
          for (int r = 0; r < NU; ++r)
#pragma unroll
            for (int c = 0; c < NU; ++c) gq[r][c] = g[(r * NU + c) * 16];
        }
        double c[NC];
        recover_segment<K>(wreg[i], wreg[i + 1] - wreg[i], xreg[i], u, un, c);
        if (i == 0 && t0 != 0.0) taylor_shift<NC>(c, -t0);
        if constexpr (NC == 8)
          store_segment_quad8(MSNAP_SEG_BASE(coef, tile, M, i, NC), MSNAP_SEG_STRIDE(M, NC), nvalid, lane, c, bad);
        else
          store_segment_coalesced<NC>(sTr, MSNAP_SEG_BASE(coef, tile, M, i, NC), MSNAP_SEG_STRIDE(M, NC), nvalid,
                                      lane, c, bad);
#pragma unroll
        for (int r = 0; r < NU; ++r) un[r] = u[r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// order-9 throughput variant, two-sided AND column-split ("twin"): lane = 8*drone + 4*side + axis,
// 8 drones per wavefront.
//  * Two sides.  The per-lane state a solve keeps between its two sweeps (z_i, the waypoints, 1/T) is what
//    pushes the one-sided order-9 kernel to 307 registers = one wave per SIMD; with the knots of a path
//    shared between two sides (the merge at the meeting knot and the reversed-time bookkeeping of side 1 are
//    those of solve_kernel_twist below) every lane keeps half of it and the dependent chain is half as long.
//  * Column split.  Order 9 has NU = 4 unknown derivatives per knot = the 4 axis lanes of a drone: lane a
//    solves column a of G_i = S_i^-1 O_i and forms column a of the Schur term O_i^T G_i (plus its own axis'
//    z_i and O_i^T z_i) instead of all four lanes carrying all 16 entries; the symmetric Schur block of the
//    next knot is gathered with quad-broadcast DPP moves, and the G columns go to LDS as they are made.
//    What a lane carries of the previous segment is its 8 powers of 1/T (the end-side block E = HEE * powers
//    is folded into the FMAs that build S) and 4 right-hand terms.
//  * All inputs of the tile go to registers at the tile top (the reciprocals run side by side, off the
//    recurrence), so the input stage is dead before the first G column is stashed and aliases the rest.
// 256 registers without scratch and 13.6 KB of LDS -> two waves per SIMD.  One instance per even segment
// count 4..10 (both sides own (M-2)/2 >= 1 knots and M/2 segments); odd counts keep solve_kernel_reg<5,10>.
// (A one-sided column-split kernel was tried first: 16 drones per wave need 33 doubles of scratch at 256
// registers and ran at 83 us against solve_kernel_reg's 75 and this kernel's 57-60 at 65 536 x 10.)
// ------------------------------------------------------------------------------------

// (the output transposition image, kTwinTrPitch / kTwinTrWords, and kTwinDrones: msnap_solve_plan.h)

// Output stores of the twin kernel.  The 4 axis lanes of a (drone, side) block hold the block's 320 bytes as
// 4 x 5 pieces of 16 bytes (lane = axis, piece = coefficient pair).  Through the LDS image the pieces are
// redistributed so that store q of lane j carries piece 4q + j of the lane's OWN block: every quad writes one
// whole 64-byte segment per instruction (the pattern of store_quad8_at), the address is the block base plus an
// immediate, and the only per-lane plan is where in the image the five pieces sit (set up once per tile).
struct TwinStorePlan {
  int ridx[5];   // double2 index into the image of the piece this lane stores with instruction q
};

__device__ __forceinline__ void twin_store_plan(int lane, TwinStorePlan &pl) {
  const int j = lane & 3, blk4 = lane & ~3;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int within = q * 4 + j;            // 16-byte piece of the block: (axis a2, pair j2)
    const int a2 = within / 5;
    const int j2 = within - a2 * 5;
    pl.ridx[q] = j2 * kTwinTrPitch + blk4 + a2;
  }
}

// `blkp`: this lane's block of the segment + (lane & 3) * 2 doubles
__device__ __forceinline__ void store_twin_coalesced(double2 *sTr, double *__restrict__ blkp, int lane,
                                                     const TwinStorePlan &pl, const double (&c)[10]) {
  constexpr int NJ = 5;
#pragma unroll
  for (int j = 0; j < NJ; ++j) sTr[j * kTwinTrPitch + lane] = make_double2(c[2 * j], c[2 * j + 1]);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
#pragma unroll
  for (int q = 0; q < NJ; ++q) *reinterpret_cast<double2 *>(blkp + q * 8) = sTr[pl.ridx[q]];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
}

// waves per SIMD an instance is built for (registers: 512 / waves per lane)
// (registers as built: order 7: 81 / 96 / 124 / 148 / 175 / 202 / 233 / 256 at 4 / 6 / ... / 18 segments; order 9:
//  92 / 123 / 164 / 201 / 242 at 4 / 6 / 8 / 10 / 12)
// knots per side whose z lives in LDS (1.5 KB per knot at order 7): the 17- to 20-segment instances -- 19 and 20
// segments would otherwise keep 23 / 8 dwords in scratch at the 256 registers of two waves per SIMD, 17 and 18 sit
// exactly at 256 (no kernel of the library uses scratch: tests/test_abi.py)
template <int K, int M>
constexpr int kTwinZInLds = (K == 4 && M >= 17) ? 4 : 0;
template <int K, int M>
constexpr int kTwinWaves = (K == 5 && M >= 13) ? 1 : 2;   // (order 9, 13..20 segments: 512 registers per lane, see kTwinMaxSeg)

// cross-tile input prefetch of the twin kernel: the hand-issued loads and exact wait of solve_kernel_reg
// (stage_load_asm / stage_wait_asm), for 8 drones per tile and a compile-time segment count
template <int M>
struct TwinStage {
  static constexpr int UW = (kTwinDrones * (M + 1) * 4 / 2 + kWave - 1) / kWave;   // 16-byte loads per lane
  static constexpr int UT = (kTwinDrones * (M + 1) + kWave - 1) / kWave;           // 8-byte loads per lane
  u32x4 vw[UW];
  double vt[UT];
};

template <int M>
__device__ __forceinline__ void twin_stage_load(const double *__restrict__ wp, const double *__restrict__ tt,
                                                int shared_times, int tile, int nvalid, int lane, TwinStage<M> &r) {
  constexpr int wpitch = (M + 1) * 4, tpitch = M + 1;
  const double2 *wsrc = reinterpret_cast<const double2 *>(wp + (size_t)tile * kTwinDrones * wpitch);
  const int wcnt = nvalid * wpitch / 2;
  const double *tsrc = shared_times ? tt : tt + (size_t)tile * kTwinDrones * tpitch;
  const int tcnt = shared_times ? tpitch : nvalid * tpitch;
#pragma unroll
  for (int u = 0; u < TwinStage<M>::UW; ++u) {
    const int e = u * kWave + lane;
    const double2 *p = wsrc + (e < wcnt ? e : wcnt - 1);
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r.vw[u]) : "v"(p) : "memory");
  }
#pragma unroll
  for (int u = 0; u < TwinStage<M>::UT; ++u) {
    const int f = u * kWave + lane;
    const double *p = tsrc + (f < tcnt ? f : tcnt - 1);
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(r.vt[u]) : "v"(p) : "memory");
  }
}

template <int M, int YOUNGER>
__device__ __forceinline__ void twin_stage_wait(TwinStage<M> &r) {
  wait_vmcnt<YOUNGER>();
#pragma unroll
  for (int u = 0; u < TwinStage<M>::UW; ++u) asm volatile("" : "+v"(r.vw[u]));
#pragma unroll
  for (int u = 0; u < TwinStage<M>::UT; ++u) asm volatile("" : "+v"(r.vt[u]));
}

template <int M>
__device__ __forceinline__ void twin_stage_store(int shared_times, int nvalid, double *sWraw, double *sTraw, int lane,
                                                 TwinStage<M> &r) {
  constexpr int wpitch = (M + 1) * 4, tpitch = M + 1;
  u32x4 *wdst = reinterpret_cast<u32x4 *>(sWraw);
  const int wcnt = nvalid * wpitch / 2;
  const int tcnt = shared_times ? tpitch : nvalid * tpitch;
#pragma unroll
  for (int u = 0; u < TwinStage<M>::UW; ++u) {
    const int e = u * kWave + lane;
    if (e < wcnt) wdst[e] = r.vw[u];
  }
#pragma unroll
  for (int u = 0; u < TwinStage<M>::UT; ++u) {
    const int f = u * kWave + lane;
    if (f < tcnt) sTraw[f] = r.vt[u];
  }
}

// gather the symmetric Schur block from the lanes' columns: entry (n, m), m <= n, is element n of lane m's column
template <int NU, int NS, int MCOL = 0>
__device__ __forceinline__ void twin_gather(const double (&col)[NU], double (&OtG)[NS]) {
  if constexpr (MCOL < NU) {
#pragma unroll
    for (int n = MCOL; n < NU; ++n) OtG[sidx(n, MCOL)] = quad_bcast<MCOL>(col[n]);
    twin_gather<NU, NS, MCOL + 1>(col, OtG);
  }
}

template <int K, int M>
__global__ void __launch_bounds__(kWave, (kTwinWaves<K, M>))
solve_kernel_twin(const double *__restrict__ wp, const double *__restrict__ tt, int shared_times,
                  int N, double *__restrict__ coef, double *__restrict__ dur,
                  int32_t *__restrict__ status, int ntiles) {
  using SW = Sweep<K>;
  using C = HermiteConsts<K>;
  constexpr int NU = SW::NU, NC = SW::NC, NS = SW::NS, KK = SW::KK, PM = SW::PM;
  static_assert(NU <= kAxes && NU >= 3, "one column of the knot blocks per axis lane (order 7: the fourth lane idles through the column work)");
  static_assert(M >= 4, "both sides own at least one knot");
  constexpr int kSlotWords = NU * kWave;      // one knot's G: [row][16 (drone, side) blocks][4 column slots]
  // M - 1 interior knots = nL (side 0) + the meeting knot + nR (side 1), nL <= nR <= nL + 1.  With an odd segment
  // count side 1 owns one knot and one segment more: all lanes run H = nR knot steps -- side 0's last one works on
  // valid data of the other side's territory and its effect on the carried state is undone (solve_kernel_twist) --
  // and side 0 sits out the first segment of the backward sweep.
  constexpr int nL = (M - 2) / 2, nR = (M - 2) - nL;
  constexpr int H = nR;
  constexpr bool kAsym = nL != nR;
  constexpr int HA = H > 0 ? H : 1;

  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int lane0 = threadIdx.x;
  constexpr int wpitch = (M + 1) * 4;
  constexpr int tpitch = M + 1;
  // LDS: [ transposition image (order 9 only) | G: [knot][row][16 blocks][column] ]; the input stage aliases both
  // (dead before the first use)
  double *sWraw = lds;
  double *sTraw = sWraw + kTwinDrones * wpitch;
  double2 *sTr = reinterpret_cast<double2 *>(lds);
  double *sG = lds + (NC == 10 ? kTwinTrWords : 0);
  // the longest instances keep z of their first ZL knots (the ones that wait longest for the backward sweep) in LDS
  // behind the G slots instead of in registers: [knot][row][64 lanes]
  constexpr int ZL = kTwinZInLds<K, M>;
  double *sZ = sG + H * kSlotWords;
  double dsg[NU];
#pragma unroll
  for (int r = 0; r < NU; ++r) dsg[r] = (r & 1) ? 1.0 : -1.0;

  auto tile_valid = [&](int tl) {
    const int left = N - tl * kTwinDrones;
    return left < kTwinDrones ? left : kTwinDrones;
  };
  // cross-tile prefetch as in solve_kernel_reg: the next tile's inputs are requested before the last two
  // segments of the backward sweep and retired at the tile top by an exact vmcnt that leaves those two
  // segments' 2 x kStoresPerSeg stores in flight (every instance has H >= 1, so both always run)
  static_assert(nL >= 1, "the prefetch sits in front of segments 1 and 0 of the backward sweep, which both sides own");
  constexpr int kStoresPerSeg = (NC == 8 ? 4 : NC / 2);
  TwinStage<M> pre;
  if ((int)blockIdx.x < ntiles)
    twin_stage_load<M>(wp, tt, shared_times, blockIdx.x, tile_valid(blockIdx.x), lane0, pre);
  wait_vmcnt<0>();

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // Everything derived from the lane index is rebuilt per tile from an opaque copy: left to the compiler,
    // two dozen loop-invariant addresses are hoisted out of the tile loop and live -- spilled -- across the
    // whole tile, which costs more than recomputing them once per ~2 500 instructions.
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int a = lane & 3;
    const int side = (lane >> 2) & 1;
    const int blk = lane >> 2;                  // (drone, side)
    const int dl = lane >> 3;
    double ca[NU];
#pragma unroll
    for (int n = 0; n < NU; ++n)
      ca[n] = a == 0 ? C::HSE[n + 1][1] : a == 1 ? C::HSE[n + 1][2] : a == 2 ? C::HSE[n + 1][3] : C::HSE[n + 1][NU];
    const int d_raw = tile * kTwinDrones + dl;
    const bool live = d_raw < N;
    const int d = live ? d_raw : N - 1;
    const int nvalid = tile_valid(tile);
    const int next = tile + gridDim.x;

    asm volatile("s_setprio 0" ::: "memory");   // tile-top marker for tools/check_prefetch_isa.py
    wave_lds_fence();   // the previous tile's LDS reads are done (in-order LDS, one wave)
    twin_stage_wait<M, 2 * kStoresPerSeg>(pre);
    twin_stage_store<M>(shared_times, nvalid, sWraw, sTraw, lane, pre);
    wave_lds_fence();
    // (the scalar-loop form: with the rounds unrolled -- store_durations<kTwinDrones * M> -- the compiler put accumulation-register
    //  copies of the 17..20-segment order-9 instances INSIDE a round's `if (e < cnt)`; tools/check_exec_isa.py refused that build)
    store_durations(sTraw, shared_times, tpitch, M, nvalid, lane, dur + (size_t)tile * kTwinDrones * M);

    const int dloc = live ? dl : (N - 1 - tile * kTwinDrones);
    const double *lw = sWraw + dloc * wpitch + a;
    const double *lt = sTraw + (shared_times ? 0 : dloc * tpitch);
    // own-coordinate accessors: side 1 walks the path backwards
    auto Wown = [&](int i) -> double { return lw[(side ? M - i : i) * 4]; };
    auto Town = [&](int i) -> double {
      const int j = side ? M - 1 - i : i;
      return lt[j + 1] - lt[j];
    };

    // ---- this side's half of the path into registers: waypoints 0..H+1, 1/T of segments 0..H ----
    double wreg[HA + 2], xreg[HA + 1], zreg[HA][NU];
    const double t0 = lt[0];
    bool nonfinite = !finite64(t0);
    bool badtime = t0 < 0.0;
#pragma unroll
    for (int i = 0; i <= H + 1; ++i) {
      wreg[i] = Wown(i);
      nonfinite |= !finite64(wreg[i]);
    }
#pragma unroll
    for (int i = 0; i <= H; ++i) {
      double T = Town(i);
      nonfinite |= !finite64(T);
      badtime |= !(T > 0.0);
      if (i == 0) {
        T = side ? T : T - t0;   // Appendix-A quirk lives on the start side only
        badtime |= !(T > 0.0);
      }
      xreg[i] = rcp64(T);
    }
    // The input checks are settled HERE, in one register: left as booleans the compares are sunk to where the status
    // is formed -- behind both sweeps -- and every |w|, |T| and T waits there in registers (32 of them at 10 segments).
    int in_flags = (nonfinite ? 4 : 0) | (badtime ? 2 : 0);
    asm volatile("" : "+v"(in_flags));
    wave_lds_fence();   // the input stage is dead: the image and the G slots alias it

    // ---- forward sweep over this side's knots (column split) ----
    // carried from knot to knot: the powers of the previous own segment's 1/T (xpp[p-1] = x^p; the end-side block
    // E = HEE * powers is folded into the FMAs that build S), rz = that segment's end-side right-hand term +
    // O^T z of the previous knot, and the Schur block O^T G
    double xpp[PM], rz[NU], OtG[NS];
    {
      double xp[PM + 1];
      SW::powers(xreg[0], xp);
      const double dw0 = wreg[1] - wreg[0];
#pragma unroll
      for (int p = 1; p <= PM; ++p) xpp[p - 1] = xp[p];
#pragma unroll
      for (int n = 1; n <= NU; ++n) rz[n - 1] = C::HEE[n][0] * (xp[KK - n] * dw0);
#pragma unroll
      for (int e = 0; e < NS; ++e) OtG[e] = 0.0;
    }
#pragma unroll
    for (int it = 1; it <= H; ++it) {
      double xpp0[PM], rz0[NU], OtG0[NS];     // side 0's carried state in front of its phantom step
      if (kAsym && it == H) {
#pragma unroll
        for (int p = 0; p < PM; ++p) xpp0[p] = xpp[p];
#pragma unroll
        for (int r = 0; r < NU; ++r) rz0[r] = rz[r];
#pragma unroll
        for (int e = 0; e < NS; ++e) OtG0[e] = OtG[e];
      }
      double xp[PM + 1];
      SW::powers(xreg[it], xp);
      const double dw = wreg[it + 1] - wreg[it];
      double S[NS], y[NU];
#pragma unroll
      for (int n = 1; n <= NU; ++n)
#pragma unroll
        for (int m = 1; m <= n; ++m)
          S[sidx(n - 1, m - 1)] =
              __builtin_fma(C::HSS[n][m], xp[KK - n - m],
                            __builtin_fma(C::HEE[n][m], xpp[KK - n - m - 1], -OtG[sidx(n - 1, m - 1)]));
#pragma unroll
      for (int n = 1; n <= NU; ++n) {
        const double tdw = xp[KK - n] * dw;
        y[n - 1] = __builtin_fma(-C::HSE[n][0], tdw, -rz[n - 1]);
        rz[n - 1] = C::HEE[n][0] * tdw;
      }
      double dinv[NU];
      in_flags |= (SW::ldl_factor(S, dinv) && (!kAsym || it <= nL || side)) ? 1 : 0;   // (not side 0's phantom step)
      asm volatile("" : "+v"(in_flags));      // (the pivot checks settled per knot, for the same reason)
      // (order 7: lane 3 has no column; it runs the same instructions on column 3's constants and lands in the
      //  unused fourth column slot of the stash)
      const double pa = a == 0 ? xp[NU] : a == 1 ? xp[NU - 1] : a == 2 ? xp[NU - 2] : xp[NU - 3];
      double g[NU];
#pragma unroll
      for (int n = 0; n < NU; ++n) g[n] = ca[n] * (n == NU - 1 ? pa : pa * xp[NU - 1 - n]);
      SW::ldl_solve(S, dinv, g);
      SW::ldl_solve(S, dinv, y);
      {
        // [knot][row r][block][column a]: the 64 lanes of a store write 64 consecutive doubles
        double *gs = sG + (it - 1) * kSlotWords + lane;
#pragma unroll
        for (int r = 0; r < NU; ++r) gs[r * kWave] = g[r];
      }
      if (it <= ZL) {
#pragma unroll
        for (int r = 0; r < NU; ++r) sZ[((it - 1) * NU + r) * kWave + lane] = y[r];
      } else {
#pragma unroll
        for (int r = 0; r < NU; ++r) zreg[it - 1][r] = y[r];
      }
#pragma unroll
      for (int q = 0; q < NU - 1; ++q) {
        g[q] *= xp[NU - 1 - q];
        y[q] *= xp[NU - 1 - q];
      }
      double col[NU];
#pragma unroll
      for (int n = 0; n < NU; ++n) {
        double sg = C::HSE[1][n + 1] * g[0], sz = C::HSE[1][n + 1] * y[0];
#pragma unroll
        for (int q = 1; q < NU; ++q) {
          sg = __builtin_fma(C::HSE[q + 1][n + 1], g[q], sg);
          sz = __builtin_fma(C::HSE[q + 1][n + 1], y[q], sz);
        }
        col[n] = sg * xp[NU - n];
        rz[n] = __builtin_fma(sz, xp[NU - n], rz[n]);
      }
      twin_gather<NU, NS>(col, OtG);
#pragma unroll
      for (int p = 1; p <= PM; ++p) xpp[p - 1] = xp[p];
      if (kAsym && it == H) {       // side 0 keeps what it carried in front of the phantom step
#pragma unroll
        for (int p = 0; p < PM; ++p) xpp[p] = side ? xpp[p] : xpp0[p];
#pragma unroll
        for (int r = 0; r < NU; ++r) rz[r] = side ? rz[r] : rz0[r];
#pragma unroll
        for (int e = 0; e < NS; ++e) OtG[e] = side ? OtG[e] : OtG0[e];
      }
    }

    // ---- the meeting knot (solve_kernel_twist): S = (E - O^T G)_own + D (E - O^T G)_other D ----
    double Sm[NS], um[NU];
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      const double q = rz[r];
      um[r] = -q - dsg[r] * __shfl_xor(q, 4);
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        const double p = __builtin_fma(C::HEE[r + 1][c + 1], xpp[KK - r - c - 3], -OtG[sidx(r, c)]);
        Sm[sidx(r, c)] = p + (dsg[r] * dsg[c]) * __shfl_xor(p, 4);
      }
    }
    {
      double dinv[NU];
      in_flags |= SW::ldl_factor(Sm, dinv) ? 1 : 0;
      SW::ldl_solve(Sm, dinv, um);
    }

    const int gsh = lane & ~7;
    const bool f_nonfinite = ((__ballot((in_flags & 4) != 0) >> gsh) & 0xFFull) != 0;
    const bool f_time = ((__ballot((in_flags & 2) != 0) >> gsh) & 0xFFull) != 0;
    const bool f_sing = ((__ballot((in_flags & 1) != 0) >> gsh) & 0xFFull) != 0;
    const int st = f_nonfinite ? MSNAP_ST_NONFINITE : f_time ? MSNAP_ST_TIMES : f_sing ? MSNAP_ST_SINGULAR : MSNAP_ST_OK;
    if (live && (lane & 7) == 0) status[d] = st;
    const bool bad = st != 0;

    // ---- outward back-substitution + recovery: every side owns its segments 0 .. H ----
    const double qnan = __builtin_nan("");
    const double zero_or_nan = bad ? qnan : 0.0;
    // drones past the batch end replay the tile's last valid one (bitwise the same values) and store on top of it
    TwinStorePlan plan;
    if constexpr (NC == 10) twin_store_plan(lane, plan);
    double *blkp = coef + ((size_t)d * M + (side ? M - 1 - H : H)) * (4 * NC) + (NC == 10 ? a * 2 : 0);
    const int blkstep = side ? 4 * NC : -(4 * NC);   // side 0 walks its segments down, side 1 up
#pragma unroll
    for (int i = 0; i < H + 2; ++i) wreg[i] = bad ? qnan : wreg[i];
    double un[NU];
#pragma unroll
    for (int r = 0; r < NU; ++r) un[r] = bad ? qnan : um[r];
#pragma unroll
    for (int it = H; it >= 0; --it) {
      // one segment at a time: left free, the scheduler issues the G reads of ALL knots at the top of the sweep and
      // holds them (12 registers per knot: 85 / 128 / 166 / 202 / 242 registers at 4..12 segments, order 7)
      if (it != 1) __builtin_amdgcn_sched_barrier(0);
      if (it == 1) {
        // with two segments left most of this tile's registers are dead: the next tile's inputs start now
        // (unconditional, clamped to the last tile, at a static point of the unrolled loop)
        __builtin_amdgcn_sched_barrier(0);
        const int nx = next < ntiles ? next : ntiles - 1;
        twin_stage_load<M>(wp, tt, shared_times, nx, tile_valid(nx), lane, pre);
      }
      const bool own = !kAsym || it <= nL || side != 0;     // side 0 sits out segment nR of an odd path
      double u[NU];
      if (it >= 1) {
        const double2 *gsl = reinterpret_cast<const double2 *>(sG + (it - 1) * kSlotWords + blk * kAxes);
#pragma unroll
        for (int r = 0; r < NU; ++r) {
          const double2 g01 = gsl[r * (kWave / 2)], g23 = gsl[r * (kWave / 2) + 1];
          double v = (it <= ZL) ? sZ[((it >= 1 ? it - 1 : 0) * NU + r) * kWave + lane] : zreg[it >= 1 ? it - 1 : 0][r];
          v = __builtin_fma(-g01.x, un[0], v);
          v = __builtin_fma(-g01.y, un[1], v);
          v = __builtin_fma(-g23.x, un[2], v);
          if constexpr (NU == 4) v = __builtin_fma(-g23.y, un[3], v);
          u[r] = v;
        }
      } else {
#pragma unroll
        for (int r = 0; r < NU; ++r) u[r] = zero_or_nan;
      }
      double ua[NU], ub[NU];
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        ua[r] = side ? dsg[r] * un[r] : u[r];      // state at the forward start of the piece
        ub[r] = side ? dsg[r] * u[r] : un[r];      // state at its forward end
      }
      const double wa = side ? wreg[it + 1] : wreg[it];
      const double wb = side ? wreg[it] : wreg[it + 1];
      // 1/T through an opaque copy: left visible, the powers of 1/T the recovery needs are recognised as the forward
      // sweep's and kept from there to here -- 6-8 registers per knot and side (85 / 128 / 166 / 202 / 242 registers at
      // 4..12 segments, order 7, before; three or four multiplies per segment instead)
      double xi = xreg[it];
      asm volatile("" : "+v"(xi));
      double c[NC];
      recover_segment<K>(wa, wb - wa, xi, ua, ub, c);
      if (side == 0 && it == 0 && t0 != 0.0) taylor_shift<NC>(c, -t0);
      if (own) {      // (quads are side-uniform: whole quads store or sit out)
        if constexpr (NC == 10) store_twin_coalesced(sTr, blkp, lane, plan, c);
        else store_quad8_at(blkp, a, c, false);      // order 7: the quad transposes its 4 x 4 pieces with DPP, no LDS
      }
      blkp += blkstep;
#pragma unroll
      for (int r = 0; r < NU; ++r) un[r] = own ? u[r] : un[r];
    }
  }
}

// ------------------------------------------------------------------------------------
// small-batch variant (2 <= n_seg <= kTwistMaxSeg): two-sided ("twisted") sweep.
// With few drones a launch is one wavefront's dependent chain, so the chain is halved:
// lane = 8*drone + 4*side + axis.  Side 0 sweeps the knots from the start of the path,
// side 1 runs THE SAME recurrence on the time-reversed path (p'(s) = p(T_total - s):
// waypoints and segment lengths reversed, odd derivatives change sign, D = diag(-1,+1,-1,..)).
// Both stop one knot short of the MEETING knot in the middle.  What each side carries towards
// it -- the end-side block of its last segment and its Schur terms -- adds up (the other
// side's part conjugated by D) to the meeting knot's own symmetric positive definite block, so
// the merge is one cross-lane swap and one more LDL^T step; then both sides back-substitute
// outwards.  Side 1 obtains forward-time coefficients by recovering each piece with its two
// end states swapped and the odd derivatives negated (p(t) = q(T - t)).
// ------------------------------------------------------------------------------------
constexpr int kTwistFenceHalf = 9;   // instances with this many knots per side fence the scheduler per knot

// T > 0 and finite -- !(T > 0) | !finite64(T) exactly -- as one v_cmp_class_f64: positive normal or positive subnormal
__device__ __forceinline__ bool usable_duration(double T) { return __builtin_amdgcn_class(T, 0x180); }

#ifdef MSNAP_TOOLS_TIMELINE
// phase timestamps of the twisted kernel (s_memrealtime, 100 MHz, and s_memtime): tools/twist_timeline.py.
// One row of 32 words per WAVE (row = tile * NW + wave): points 0..4 in words 0..9.
__device__ unsigned long long g_timeline[1024 * 32];
#define MSNAP_TL(k)                                                                       \
  do {                                                                                    \
    const int row__ = (int)blockIdx.x * NW + wave;                                        \
    if (lane == 0 && row__ < 1024) {                                                      \
      g_timeline[row__ * 32 + 2 * (k)] = wall_clock64();                                  \
      g_timeline[row__ * 32 + 2 * (k) + 1] = clock64();                                   \
    }                                                                                     \
  } while (0)
#else
#define MSNAP_TL(k) do { } while (0)
#endif

// One instance per (order, segment count M); MAXH = knots of the longer side.  Every loop bound is
// a constant, so the whole solve is straight-line code that the scheduler interleaves across knots
// (a run-time M costs block boundaries with dozens of register copies each: 6.2 vs 5.3 us at M = 10).
//
// NW waves per tile (1, 2 or 4; option "twist_waves").  The launcher's default takes NW > 1 only while the batch has
// at most one tile per two (NW = 2) or four (NW = 4) CUs, where each wave of a workgroup can have a SIMD, and its
// issue port, to itself; a forced "twist_waves" holds at any tile count, the tiles then share SIMDs (correct, slower:
// the sweeps run NW times on them).  Every wave runs the same sweeps and the same merge (redundantly: no second
// barrier, every wave holds the knot states), then the
// back-substitution and the recovery are split by segment: wave w recovers the pieces it in [lo(w), hi(w)] of
// both sides, and back-substitutes from the meeting knot only as far out as lo(w).  The waves with the longest
// back-substitution recover the fewest pieces.  Every value is computed by the same code from the same
// operands as at NW = 1: the outputs are bitwise those of the one-wave form.
// Contract: grid == tile count (one workgroup per 8-drone tile; the launcher starts exactly that many).
template <int S, int NW>   // S pieces per side (it = 0 .. S-1): the chunk of wave w, larger chunks at the high end
__device__ __forceinline__ constexpr int twist_chunk_lo(int w) {
  return w * (S / NW) + (w > NW - S % NW ? w - (NW - S % NW) : 0);
}
// the Hermite constants of the lean instances (msnap_twist_consts.h).  NOT const: a constant table would be folded back
// into the literals it replaces.
__constant__ TwistConstImage g_twist_consts = twist_const_image();

// N doubles from `src` (wave-uniform) into scalar registers, in the fewest s_load_dwordx16 / x8 / x4 / x2.  Issued from
// inline asm: written as plain loads the compiler sinks them, and their lgkmcnt wait, next to the first use -- onto the
// dependent chain.  The compiler's wait-count pass does not see these loads; the caller retires them with
// sload_wait() before the first use (cdna_hip_programming.md 5.7).  Scalar loads return out of order: only
// lgkmcnt(0) retires them.
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x8 __attribute__((ext_vector_type(8)));
template <int OFF, int N>
__device__ __forceinline__ void sload_f64(const double *src, double (&dst)[N]) {
  if constexpr (N - OFF >= 8) {
    f64x8 v;
    asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(v) : "s"(src), "i"(OFF * 8));
#pragma unroll
    for (int q = 0; q < 8; ++q) dst[OFF + q] = v[q];
    sload_f64<OFF + 8>(src, dst);
  } else if constexpr (N - OFF >= 4) {
    f64x4 v;
    asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(v) : "s"(src), "i"(OFF * 8));
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[OFF + q] = v[q];
    sload_f64<OFF + 4>(src, dst);
  } else if constexpr (N - OFF >= 2) {
    f64x2 v;
    asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(v) : "s"(src), "i"(OFF * 8));
    dst[OFF] = v[0];
    dst[OFF + 1] = v[1];
    sload_f64<OFF + 2>(src, dst);
  } else if constexpr (N - OFF == 1) {
    asm volatile("s_load_dwordx2 %0, %1, %2" : "=s"(dst[OFF]) : "s"(src), "i"(OFF * 8));
  }
}
// one dword of each of the NL 64-byte lines at `src`: brings the lines into the scalar cache for a later sload_f64.
// The registers stay pinned until touch_wait(), behind the wait that retires the loads (a register the compiler
// believed free would be written by the returning load).
template <int OFF, int NL>
__device__ __forceinline__ void sload_touch(const double *src, unsigned (&t)[NL]) {
  if constexpr (OFF < NL) {
    asm volatile("s_load_dword %0, %1, %2" : "=s"(t[OFF]) : "s"(src), "i"(OFF * 64));
    sload_touch<OFF + 1>(src, t);
  }
}
template <int NL>
__device__ __forceinline__ void touch_wait(unsigned (&t)[NL]) {
#pragma unroll
  for (int s = 0; s < NL; ++s) asm volatile("" : "+s"(t[s]));
}
template <int N>
__device__ __forceinline__ void sload_wait(double (&v)[N]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // live in scalar registers from here: no use is scheduled above the wait
#pragma unroll
  for (int s = 0; s < N; ++s) asm volatile("" : "+s"(v[s]));
}

template <int K, int MAXH, int M, int NW>
__global__ void __launch_bounds__(kWave * NW)
solve_kernel_twist(const double *__restrict__ wp, const double *__restrict__ tt, int shared_times,
                   int N, double *__restrict__ coef, double *__restrict__ dur,
                   int32_t *__restrict__ status) {
  static_assert(NW == 1 || NW == 2 || NW == 4, "one, two or four waves per tile");
  using SW = Sweep<K>;
  constexpr int NU = SW::NU, NC = SW::NC, NS = SW::NS;
  // M - 1 interior knots = nL (side 0) + the meeting knot + nR (side 1), nL <= nR <= nL + 1
  constexpr int nL = (M - 2) / 2, nR = (M - 2) - nL;
  static_assert(M >= 2 && MAXH == nR, "MAXH is the knot count of the longer side");
  constexpr int HA = MAXH > 0 ? MAXH : 1;     // array extent (M = 2 has no side knots)

  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int tid = threadIdx.x;
  const int lane = NW > 1 ? tid & (kWave - 1) : tid;
  // the wave index in a scalar register: every branch on it is a scalar branch (exec stays whole)
  const int wave = NW > 1 ? __builtin_amdgcn_readfirstlane(tid / kWave) : 0;
  const int a = lane & 3;
  const int side = (lane >> 2) & 1;
  const int dl = lane >> 3;           // drone inside the tile
  constexpr int wpitch = (M + 1) * 4;
  constexpr int tpitch = M + 1;
  const int mside = side ? nR : nL;
  double *sWraw = lds;
  double *sTraw = sWraw + kTwistDrones * wpitch;
  // D = diag(-1, +1, -1, ...): derivative r+1 of the time-reversed path
  double dsg[NU];
#pragma unroll
  for (int r = 0; r < NU; ++r) dsg[r] = (r & 1) ? 1.0 : -1.0;

  // ONE tile per workgroup, no tile loop: the launcher starts exactly one workgroup per tile (launch_solve_k:
  // grid = nt8).  With a loop around the body the compiler hoisted ~130 loop-invariant instructions (constants,
  // lane-derived indices) into its preheader -- IN FRONT of the tile's input loads, a quarter of a microsecond of a
  // 3.6 us kernel (round 4).  Nor is there a `tile < ntiles` test (and no tile-count argument at all): it made the
  // kernel fetch the count alone, wait, branch, and only then fetch its other arguments -- two dependent
  // scalar-cache round trips in front of the first load.
  const int tile = blockIdx.x;
  // The lean instances (below) take their Hermite constants from g_twist_consts by scalar loads instead of two
  // s_mov_b32 issue slots per constant: the sweep set is requested here, in front of the input loads, and its flight
  // lies under theirs; the recovery set follows behind the last knot (its cache lines are touched here, so that the
  // late request is a scalar-cache hit: the compiler schedules most of the merge in front of the request).
  // (order 9 with 4 segments keeps its literals: with the sweep set resident two scalar registers spill to vector lanes)
  constexpr bool kTab = MAXH * (K - 1) * (K - 1) <= 36 && !(K == 5 && M == 4);
  // (order 9: both sets at once do not fit the 102 scalar registers, 2-9 of them spilled to vector lanes; its
  //  recovery set stays literal)
  constexpr bool kTabRec = kTab && K == 4;
  using HC = std::conditional_t<kTab, TableHermite<K, kTabRec>, LiteralHermite<K>>;
  HC hc;
  constexpr int kRecLines = kTabRec ? (TwistConstLayout<K>::n_rec * 8 + 63) / 64 : 1;
  unsigned rec_touch[kRecLines];
  if constexpr (kTab) {
    sload_f64<0>(g_twist_consts.v + TwistConstLayout<K>::sweep_at, hc.sw);
    if constexpr (kTabRec) sload_touch<0>(g_twist_consts.v + TwistConstLayout<K>::rec_at, rec_touch);   // (the sets start on a line)
  }
  // (pinning the three output pointers in SGPRs at the top -- the compiler re-fetches each right in front of its first
  //  use, a scalar-cache hit on the dependent chain -- was measured and LOST: 4.52 against 4.38 us per step; the kernel
  //  holds ~60 fp64 constants in scalar registers and six more live ones push some of them out)
  {
    MSNAP_TL(0);
    const int d_raw = tile * kTwistDrones + dl;
    const bool live = d_raw < N;
    const int d = live ? d_raw : N - 1;
    const int left = N - tile * kTwistDrones;
    const int nvalid = left < kTwistDrones ? left : kTwistDrones;

    {   // stage the 8 drones' inputs (one flight; at NW > 1 every wave loads its share)
      constexpr int NT = kWave * NW;
      const double2 *wsrc = reinterpret_cast<const double2 *>(wp + (size_t)tile * kTwistDrones * wpitch);
      double2 *wdst = reinterpret_cast<double2 *>(sWraw);
      const int wcnt = nvalid * wpitch / 2;
      const double *tsrc = shared_times ? tt : tt + (size_t)tile * kTwistDrones * tpitch;
      const int tcnt = shared_times ? tpitch : nvalid * tpitch;
      constexpr int UW = (kTwistDrones * wpitch / 2 + NT - 1) / NT;
      constexpr int UT = (kTwistDrones * tpitch + NT - 1) / NT;
      double2 vw[UW];
      double vt[UT];
#pragma unroll
      for (int u = 0; u < UW; ++u) {
        const int e = u * NT + tid;
        vw[u] = wsrc[e < wcnt ? e : wcnt - 1];
      }
#pragma unroll
      for (int u = 0; u < UT; ++u) {
        const int f = u * NT + tid;
        vt[u] = tsrc[f < tcnt ? f : tcnt - 1];
      }
#pragma unroll
      for (int u = 0; u < UW; ++u) asm volatile("" : "+v"(vw[u].x), "+v"(vw[u].y));
#pragma unroll
      for (int u = 0; u < UT; ++u) asm volatile("" : "+v"(vt[u]));
#pragma unroll
      for (int u = 0; u < UW; ++u) {
        const int e = u * NT + tid;
        if (e < wcnt) wdst[e] = vw[u];
      }
#pragma unroll
      for (int u = 0; u < UT; ++u) {
        const int f = u * NT + tid;
        if (f < tcnt) sTraw[f] = vt[u];
      }
    }
    __syncthreads();
    MSNAP_TL(1);
    if constexpr (kTab) {   // (the barrier's own wait has retired them: one slot)
      sload_wait(hc.sw);
      if constexpr (kTabRec) touch_wait(rec_touch);
    }

    const int dloc = live ? dl : (N - 1 - tile * kTwistDrones);
    const double *lw = sWraw + dloc * wpitch + a;
    const double *lt = sTraw + (shared_times ? 0 : dloc * tpitch);
    // own-coordinate accessors: side 1 walks the path backwards
    auto Wown = [&](int i) -> double { return lw[(side ? M - i : i) * 4]; };
    auto Town = [&](int i) -> double {
      const int j = side ? M - 1 - i : i;
      return lt[j + 1] - lt[j];
    };

    // long paths keep z_i in LDS (one slot per lane) so the instance fits the register file
    constexpr bool kZReg = MAXH * NU < 3 * kTwistFenceHalf;
    double wreg[HA + 2], xreg[HA + 1], zreg[kZReg ? HA : 1][NU];
    double *sZ = sTraw + kTwistDrones * tpitch + wave * (HA * NU * kWave) + lane;   // per wave: [knot][r][64 lanes]
    // the G_i blocks stay in registers (overflowing into AGPRs on long paths: the instance is built for one wave per
    // SIMD, whatever NW, and the hardware places no more) -- no LDS round trip on the dependent chain
    double Greg[HA][NU][NU];
    const double t0 = lt[0];
    wreg[0] = Wown(0);
    wreg[1] = Wown(1);
    const double T0 = Town(0);
    const double T0q = side ? T0 : T0 - t0;   // Appendix-A quirk lives on the start side only
    // Input flags.  The instances that fit the architectural register file (kLean) carry ONE per-lane flag through
    // the sweeps, "an input of this lane is not usable" (not finite, or times out of order): which of the two it was
    // is found again from the staged inputs on the rare path behind the merge.  A duration is usable iff it is
    // positive and finite, one class test.  The long instances keep the two flags apart and classify in line, as
    // they always did: a branch behind their merge moves the compiler's accumulation-register copies into the
    // divergent regions of the recovery (tools/check_exec_isa.py).
    constexpr bool kLean = MAXH * NU * NU <= 36;   // order 7: up to 10 segments, order 9: up to 6
    bool inbad = false, nonfinite = false, badtime = false;
    if constexpr (kLean) {
      inbad = !(finite64(t0) & finite64(wreg[0]) & finite64(wreg[1]) & usable_duration(T0)) | !(T0q > 0.0) | (t0 < 0.0);
    } else {
      nonfinite = !(finite64(t0) & finite64(T0) & finite64(wreg[0]) & finite64(wreg[1]));
      badtime = !(T0 > 0.0) | !(T0q > 0.0) | (t0 < 0.0);
    }
    xreg[0] = rcp64(T0q);
    SW sw;
    sw.init(xreg[0], wreg[1] - wreg[0], hc);

    // Per knot, the long dependent prefix that does not involve the recurrence -- inputs from LDS,
    // T, 1/T (reciprocal + Newton), its powers -- is prepared one knot AHEAD, inside the same
    // basic block as the previous knot's recurrence, where it fills that chain's latency bubbles.
    // All lanes run all nR steps; when side 0 owns one knot less its extra step works on valid
    // data and its effect on the carried state is undone.
    double xpc[SW::PM + 1], dwc = 0.0;     // powers of 1/T_it and w_{it+1} - w_it of the current knot
    auto ahead = [&](int it, double (&xp)[SW::PM + 1], double &dw) {
      wreg[it + 1] = Wown(it + 1);
      const double Tit = Town(it);
      if constexpr (kLean) {
        inbad |= !(usable_duration(Tit) & finite64(wreg[it + 1]));
      } else {
        nonfinite |= !finite64(Tit) | !finite64(wreg[it + 1]);
        badtime |= !(Tit > 0.0);
      }
      xreg[it] = rcp64(Tit);
      SW::powers(xreg[it], xp);
      dw = wreg[it + 1] - wreg[it];
    };
    if (MAXH >= 1) ahead(1, xpc, dwc);
    bool singular = false;
    auto knot_step = [&](int it) {
      double G[NU][NU], z[NU];
      typename SW::Knot k;
      SW::knot_geom_xp(xpc, dwc, sw.E, sw.re, k, hc);
      const bool ok = sw.chain(k, G, z);
      singular |= !ok & (it <= mside);
#pragma unroll
      for (int e = 0; e < NS; ++e) sw.E[e] = k.E[e];
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        sw.re[r] = k.re[r];
        if constexpr (kZReg) zreg[it - 1][r] = z[r];
        else sZ[((it - 1) * NU + r) * kWave] = z[r];
#pragma unroll
        for (int c = 0; c < NU; ++c) Greg[it - 1][r][c] = G[r][c];
      }
    };
#pragma unroll
    for (int it = 1; it <= MAXH; ++it) {
      if (it < MAXH) {             // knot it, and the prefix of knot it+1
        double xpn[SW::PM + 1], dwn;
        ahead(it + 1, xpn, dwn);
        knot_step(it);
        dwc = dwn;
#pragma unroll
        for (int q = 0; q <= SW::PM; ++q) xpc[q] = xpn[q];
        // long paths: keep the scheduler from hoisting several knots' inputs at once (register
        // pressure beyond the 512-entry file would spill to scratch)
        if constexpr (MAXH * NU >= 3 * kTwistFenceHalf) __builtin_amdgcn_sched_barrier(0);
      } else if (nL == nR) {       // last knot, owned by both sides
        knot_step(it);
      } else {                     // last knot of side 1 only: side 0 keeps its carried state
        double E0[NS], G0[NS], r0[NU], z0[NU];
#pragma unroll
        for (int e = 0; e < NS; ++e) { E0[e] = sw.E[e]; G0[e] = sw.OtG[e]; }
#pragma unroll
        for (int r = 0; r < NU; ++r) { r0[r] = sw.re[r]; z0[r] = sw.Otz[r]; }
        knot_step(it);
#pragma unroll
        for (int e = 0; e < NS; ++e) { sw.E[e] = side ? sw.E[e] : E0[e]; sw.OtG[e] = side ? sw.OtG[e] : G0[e]; }
#pragma unroll
        for (int r = 0; r < NU; ++r) { sw.re[r] = side ? sw.re[r] : r0[r]; sw.Otz[r] = side ? sw.Otz[r] : z0[r]; }
      }
    }

    MSNAP_TL(2);
    // the recovery set: requested behind the last knot, retired in front of the back-substitution
    if constexpr (kTabRec) sload_f64<0>(g_twist_consts.v + TwistConstLayout<K>::rec_at, hc.rc);
    // ---- the meeting knot: both sides' carried blocks add up to ONE symmetric positive definite
    // system,  S = (E - O^T G)_own + D (E - O^T G)_other D ,  y = -(re + O^T z)_own - D (re + O^T z)_other
    // (each side in its own orientation; D conjugates the other side's blocks).  One cross-lane
    // swap, then the same LDL^T as every other knot.
    double Sm[NS], um[NU];
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      const double q = sw.re[r] + sw.Otz[r];
      um[r] = -q - dsg[r] * row_xor4_f64(q);
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        const double p = sw.E[sidx(r, c)] - sw.OtG[sidx(r, c)];
        Sm[sidx(r, c)] = p + (dsg[r] * dsg[c]) * row_xor4_f64(p);
      }
    }
    {
      double dinv[NU];
      singular |= SW::ldl_factor(Sm, dinv);
      SW::ldl_solve(Sm, dinv, um);
    }

    // Status: per drone over its 8 lanes (2 sides x 4 axes) from wave ballots, no cross-lane round trips
    auto classify = [&]() -> int {
      const int gsh = lane & ~7;
      const bool f_nonfinite = ((__ballot(nonfinite) >> gsh) & 0xFFull) != 0;
      const bool f_time = ((__ballot(badtime) >> gsh) & 0xFFull) != 0;
      const bool f_sing = ((__ballot(singular) >> gsh) & 0xFFull) != 0;
      return f_nonfinite ? MSNAP_ST_NONFINITE : f_time ? MSNAP_ST_TIMES : f_sing ? MSNAP_ST_SINGULAR : MSNAP_ST_OK;
    };
    auto put_status = [&](int st) {
      if (live && (lane & 7) == 0 && wave == NW - 1) status[d] = st;   // (moved to the end with the durations: no gain, 4.30 against 4.28 us)
    };
    // A failed drone's outputs are NaN: poison what every coefficient is computed from once
    // (waypoints -> c0 and the end-side block, knot states -> c1..) instead of selecting per piece.
    double zero_or_nan = 0.0;
    double un[NU];
    auto poison = [&](bool bad) {
      const double qnan = __builtin_nan("");
      zero_or_nan = bad ? qnan : 0.0;
#pragma unroll
      for (int i = 0; i < MAXH + 2; ++i) wreg[i] = bad ? qnan : wreg[i];
#pragma unroll
      for (int r = 0; r < NU; ++r) un[r] = bad ? qnan : um[r];
    };
    if constexpr (kLean) {
      // The common case -- no lane of the wave has anything to report -- is one wave ballot: status 0, and the
      // back-substitution starts from the merge's registers as they are.  Only a wave that holds a failed drone
      // takes the branch (wave-uniform: exec stays whole).
      int st = MSNAP_ST_OK;
#pragma unroll
      for (int r = 0; r < NU; ++r) un[r] = um[r];
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(inbad | singular) != 0, 0)) {
        asm volatile("" ::: "memory");   // keep the block a branch: the compiler would flatten it into selects again
        // which kind of input failure: the sweeps' own tests again, on the inputs still staged in LDS
        const double T0r = Town(0);
        nonfinite = !(finite64(t0) & finite64(T0r) & finite64(wreg[0]) & finite64(wreg[1]));
        badtime = !(T0r > 0.0) | !((side ? T0r : T0r - t0) > 0.0) | (t0 < 0.0);
#pragma unroll
        for (int it = 1; it <= MAXH; ++it) {
          const double Tit = Town(it);
          nonfinite |= !finite64(Tit) | !finite64(wreg[it + 1]);
          badtime |= !(Tit > 0.0);
        }
        st = classify();
        poison(st != 0);
      }
      put_status(st);
    } else {
      const int st = classify();
      put_status(st);
      poison(st != 0);
    }

    MSNAP_TL(3);
    if constexpr (kTabRec) sload_wait(hc.rc);
    // ---- outward back-substitution + recovery: side s owns its segments 0 .. mside; this wave recovers the
    // pieces lo .. hi of each side and back-substitutes out to lo (scalar bounds: wave-uniform branches) ----
    const int lo = twist_chunk_lo<MAXH + 1, NW>(wave), hi = twist_chunk_lo<MAXH + 1, NW>(wave + 1) - 1;
#pragma unroll
    for (int it = MAXH; it >= 0; --it) {
      if (NW > 1 && (it < lo || hi < lo)) break;     // (no piece of this wave further out)
      if (it <= nL || side) {    // only side 1 owns segment nR when nL < nR
        double u[NU];
        if (it >= 1) {
#pragma unroll
          for (int r = 0; r < NU; ++r) {
            double v;
            if constexpr (kZReg) v = zreg[it >= 1 ? it - 1 : 0][r];
            else v = sZ[((it >= 1 ? it - 1 : 0) * NU + r) * kWave];
#pragma unroll
            for (int c = 0; c < NU; ++c) v = __builtin_fma(-Greg[it >= 1 ? it - 1 : 0][r][c], un[c], v);
            u[r] = v;
          }
        } else {
#pragma unroll
          for (int r = 0; r < NU; ++r) u[r] = zero_or_nan;
        }
        if (NW == 1 || it <= hi) {   // (beyond hi: back-substitution only, the piece is another wave's)
        // Side 1 holds the piece in reversed time, q(s) with p(t) = q(T - t).  Its endpoint states in
        // forward time are the reversed ones with the odd derivatives negated, so the forward
        // coefficients come from the same recovery with the two ends swapped -- no Taylor shift.
        double ua[NU], ub[NU];
#pragma unroll
        for (int r = 0; r < NU; ++r) {
          ua[r] = side ? dsg[r] * un[r] : u[r];      // state at the forward start of the piece
          ub[r] = side ? dsg[r] * u[r] : un[r];      // state at its forward end
        }
        const double wa = side ? wreg[it + 1] : wreg[it];
        const double wb = side ? wreg[it] : wreg[it + 1];
        double c[NC];
        // The piece that side 1 alone owns (odd M) keeps the literals: there `side` is known, the compiler folds the
        // reversal's negations into the constants themselves, and the sign bit of a failed drone's NaN coefficients
        // follows that fold (tests/test_twist_bits_gpu.py holds it) -- a constant in a register cannot take it.
        if constexpr (kTabRec) {
          if (it <= nL) recover_segment<K>(wa, wb - wa, xreg[it], ua, ub, c, hc);
          else recover_segment<K>(wa, wb - wa, xreg[it], ua, ub, c);
        } else {
          recover_segment<K>(wa, wb - wa, xreg[it], ua, ub, c);
        }
        if (side == 0 && it == 0 && t0 != 0.0) taylor_shift<NC>(c, -t0);
        const int seg = side ? M - 1 - it : it;
        // a batch this small is latency bound, not store bound: plain per-lane stores.  Lanes past
        // the batch end mirror drone N-1 (same inputs, same values, same addresses), so the stores
        // need no predicate and the sweep stays one basic block.
        {
          // (a lane base formed early and pinned in two vector registers, so that the fetch of `coef` leaves the
          //  dependent chain, was measured: 4.54 against 4.28 us per step -- not shipped)
          double *o = coef + (((size_t)d * M + seg) * 4 + a) * NC;
#pragma unroll
          for (int m = 0; m < NC; m += 2) *reinterpret_cast<double2 *>(o + m) = make_double2(c[m], c[m + 1]);
        }
        }
#pragma unroll
        for (int r = 0; r < NU; ++r) un[r] = u[r];
      }
      if constexpr (MAXH * NU >= 3 * kTwistFenceHalf) __builtin_amdgcn_sched_barrier(0);
    }
    // the durations leave LAST: in front of the sweeps they cost the fetch of their pointer and ~40 instructions on the
    // dependent chain; the staged times are still in LDS (the z stash lives behind them, nothing aliases the inputs;
    // at NW > 1 the whole workgroup shares the rounds)
    __builtin_amdgcn_sched_barrier(0);
    store_durations<kTwistDrones * M, kWave * NW>(sTraw, shared_times, tpitch, M, nvalid, tid,
                                                  dur + (size_t)tile * kTwistDrones * M);
    MSNAP_TL(4);
  }
}

static SolveKnobs solve_knobs(const msnap_ctx *ctx) {
  return {ctx->n_cu, ctx->no_twist, ctx->no_twin, ctx->twist_max_drones, ctx->twin_max_drones, ctx->twist_waves,
          ctx->solve_grid_waves};
}

// plan (msnap_solve_plan.h: family, instance, geometry -- and why) -> slab -> name -> launch
template <int K>
static int launch_solve_k(msnap_ctx *ctx, int N, int M, const double *wp, const double *t, int shared,
                          double *coef, double *dur, int32_t *status) {
  const SolvePlan p = plan_solve(solve_knobs(ctx), K, N, M);
  if (p.slab_bytes > 0) {
    int rc = ensure(ctx, ctx->scratch, p.slab_bytes);
    if (rc) return rc;
  }
  solve_plan_name(p, ctx->last_kernel, sizeof(ctx->last_kernel));   // (note_kernel's one formatting per launch)
  const dim3 grid(p.grid), block(p.block);
  bool found = true;
  switch (p.family) {
    case SolveFamily::twist:
      // grid == tile count, and no tile-count argument: the kernel's seven arguments are exactly the 12 dwords the
      // build preloads into SGPRs
      found = dispatch_range<2, twist_max_seg(K)>(M, [&](auto seg) {
        constexpr int MM = decltype(seg)::value;
        auto launch = [&](auto waves) {
          hipLaunchKernelGGL((solve_kernel_twist<K, twist_half(MM), MM, decltype(waves)::value>), grid, block,
                             p.lds_bytes, ctx->stream, wp, t, shared, N, coef, dur, status);
        };
        if (p.waves == 4) launch(std::integral_constant<int, 4>{});
        else if (p.waves == 2) launch(std::integral_constant<int, 2>{});
        else launch(std::integral_constant<int, 1>{});
      });
      break;
    case SolveFamily::twin:
      found = dispatch_range<kTwinMinSeg, twin_max_seg(K)>(M, [&](auto seg) {
        hipLaunchKernelGGL((solve_kernel_twin<K, decltype(seg)::value>), grid, block, p.lds_bytes, ctx->stream, wp, t,
                           shared, N, coef, dur, status, p.tiles);
      });
      break;
    case SolveFamily::reg:
      if (p.seg == kRegMaxSeg)
        hipLaunchKernelGGL((solve_kernel_reg<K, kRegMaxSeg>), grid, block, p.lds_bytes, ctx->stream, wp, t, shared, N, M,
                           coef, dur, status, p.tiles);
      else
        hipLaunchKernelGGL((solve_kernel_reg<K, kRegMaxSeg2>), grid, block, p.lds_bytes, ctx->stream, wp, t, shared, N, M,
                           coef, dur, status, p.tiles);
      break;
    case SolveFamily::rolled:
      if (p.slab_bytes > 0)
        hipLaunchKernelGGL((solve_kernel<K, true>), grid, block, p.lds_bytes, ctx->stream, wp, t, shared, N, M, coef, dur,
                           status, (double *)ctx->scratch.p, p.tiles);
      else
        hipLaunchKernelGGL((solve_kernel<K, false>), grid, block, p.lds_bytes, ctx->stream, wp, t, shared, N, M, coef,
                           dur, status, (double *)nullptr, p.tiles);
      break;
  }
  if (!found) return MSNAP_EINVAL;   // unreachable: the plan's ranges are the dispatch's bounds
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// one drone's plan: the slab does not depend on the batch size (msnap_solve_plan.h)
bool solve_uses_global_scratch(const msnap_ctx *ctx, int n_seg) {
  return plan_solve(solve_knobs(ctx), ctx->khalf, 1, n_seg).slab_bytes > 0;
}

#ifdef MSNAP_TOOLS_TIMELINE
extern "C" int msnap_debug_read_timeline(unsigned long long *out, int n_words) {
  if (hipDeviceSynchronize() != hipSuccess) return MSNAP_EHIP;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), (size_t)n_words * 8) == hipSuccess ? MSNAP_OK : MSNAP_EHIP;
}
#endif

int solve_kernel_setup(msnap_ctx *ctx) {
  // allow the full 160 KiB of dynamic LDS
  MSNAP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&solve_kernel<4, false>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes));
  MSNAP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&solve_kernel<5, false>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes));
  return MSNAP_OK;
}

int launch_solve(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                 int shared_times, double *coef, double *dur, int32_t *status) {
  if (n_drones == 0) return MSNAP_OK;
  if (ctx->khalf == 4)
    return launch_solve_k<4>(ctx, n_drones, n_seg, wp, t, shared_times, coef, dur, status);
  return launch_solve_k<5>(ctx, n_drones, n_seg, wp, t, shared_times, coef, dur, status);
}

}  // namespace msnap
