// The rolled solve of one 16-drone tile: the body of solve_kernel<K, GS> (msnap_solve.hip, rest to rest), of
// states_solve_kernel<K> (msnap_states.hip, given end states) and of gates_solve_kernel<K> (msnap_gates.hip, prescribed
// derivatives at interior knots as well).  lane = 4 drone + axis; the tile's inputs are staged in
// LDS by the caller (GS: read from global memory here), the knot loops are rolled over Sweep<K>::step, X / G / Z are
// stashed in LDS or on a global slab, and every segment leaves through recover_segment and the full-line stores.
// The callers carve their own layouts -- they differ on purpose -- and pass the pointers.  The elimination itself is
// chain_solve below, the one text of the open chain, which the time allocation's trial (msnap_timeopt_kernel.h) runs
// as well; what the solves do differently is one `if constexpr` each.
#pragma once

#include "msnap_sweep.h"

namespace msnap {

// Where the caller put a tile's images (doubles; sS0 / sS1, the lanes' end states at pitch (K - 1) | 1, for ENDS only).
// The output transpose image (order 9) is not among them: in every layout it is the start of dynamic LDS, and
// rolled_solve_tile names it so where it stores (see there).
struct RolledTile {
  double *sWraw, *sTraw;     // staged waypoints [16][(M+1) 4] and times [16][M+1] (not read with GS)
  double *sX, *sG, *sZ;      // stash: X[M][16] | G[M-1][NU NU][16] | Z[M-1][NU][64]
  double *sS0, *sS1;
};

// one coalesced pass over a tile's state block ([nvalid][4][NU], contiguous) into its LDS image [64][pitch]
// (shared by states_solve_kernel and timeopt_kernel<K, kTimeoptEnds>, which passes its own tile's block and tile = 0)
template <int NU, int PITCH>
__device__ __forceinline__ void load_states(const double *__restrict__ src, int tile, int nvalid, int lane,
                                            double (&v)[NU]) {
  const double *s = src + (size_t)tile * kWave * NU;
  const int cnt = nvalid * 4 * NU;
#pragma unroll
  for (int q = 0; q < NU; ++q) {
    const int e = q * kWave + lane;
    v[q] = s[e < cnt ? e : cnt - 1];
  }
}
template <int NU, int PITCH>
__device__ __forceinline__ void store_states(double *sS, int nvalid, int lane, const double (&v)[NU]) {
  const int cnt = nvalid * 4 * NU;
#pragma unroll
  for (int q = 0; q < NU; ++q) {
    const int e = q * kWave + lane;
    const int l = e / NU;
    if (e < cnt) sS[l * PITCH + (e - l * NU)] = v[q];
  }
}

// One step of iterative refinement of the LAST segment's end conditions.  recover_segment's upper coefficients are
// cancelling sums (constants of 10^2 .. 10^3) computed with 1/T rounded, so the polynomial it returns has the given
// end state only to the accuracy of its coefficients.  Here the end values are evaluated with msnap_eval_state's own
// arithmetic at `tl` -- the local time that evaluator reaches at the sum of the durations -- and their residual
// against (w_M, u_M) is taken out of the upper coefficients through CE (a_hi = CS e_start + CE e_end is linear in the
// end vector; the lower coefficients, and with them the continuity at the knot before, do not move).  The change is
// a few units in the last place; what it buys is that the evaluator returns the given end state to its own rounding.
template <int K>
__device__ __forceinline__ void refine_end(double (&c)[2 * K], double tl, double x, double wend,
                                           const double (&uend)[K - 1]) {
#pragma clang fp contract(off)
  using C = HermiteConsts<K>;
  constexpr int NC = 2 * K;
  double r[K], dd[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) dd[i] = c[i];
  double tp = 1.0;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    if (q > 0) {
#pragma unroll
      for (int i = 0; i < NC - q; ++i) dd[i] = (double)(i + 1) * dd[i + 1];
    }
    double p = 0.0;
#pragma unroll
    for (int i = NC - 1 - q; i >= 0; --i) p = p * tl + dd[i];
    r[q] = (p - (q == 0 ? wend : uend[q > 0 ? q - 1 : 0])) * tp;      // in normalised time: T^q times the q-th derivative
    tp = tp * tl;
  }
  double xq = 1.0;
#pragma unroll
  for (int m = 0; m < K; ++m) xq = xq * x;
#pragma unroll
  for (int m = 0; m < K; ++m) {
    double acc = 0.0;
#pragma unroll
    for (int n = 0; n < K; ++n) acc = acc + C::CE[m][n] * r[n];
    c[K + m] = c[K + m] - acc * xq;
    xq = xq * x;
  }
}

// ------------------------------------------------------------------------------------
// chain_solve: the open-chain elimination of DESIGN.md §3 as one device function, the one text of it.  The rolled
// solves below run it over a stash with the compile-time tile of 16 drones (in LDS, or on solve_kernel<K, true>'s global
// slab: only other pointers), the trial of the time allocation (timeopt_kernel<K, MODE> of msnap_timeopt_kernel.h, the
// rest, end-state and free-total modes) over one whose tile size is a run-time value.  lane = 4 drone + axis.
//   segment 0  x = 1 / T_0 with ENDS; without, the reference takes segment 0's start rows at local time t[0]
//              (Appendix-A quirk, see taylor_shift()): x = 1 / (T_0 - t[0]), and the caller shifts the segment back;
//   knot 1     ENDS: it sees the start state through the coupling block of segment 0, Otz = O_0^T u_0;
//   forward    block LDL^T over the interior knots, Sweep<K>::step, the operands of knot i+1 fetched one knot ahead
//              (their latency off the chain); X = 1/T, G_i = S_i^-1 O_i and z_i go to the stash;
//   backward   u_i = z_i - G_i u_{i+1} from u_M (the stash holds G of every knot, the last one included; with two
//              segments the one knot receives both end terms), the operands of segment i-1 fetched while segment i is
//              recovered; segment 0 starts from u_0;
//   REFINE     the last segment takes one refinement step on its end conditions (refine_end).
// ------------------------------------------------------------------------------------

// One lane's view of its tile's stash, every pointer already at this lane's column (the caller decides whether a lane
// past the batch end writes a column of its own or replays the last drone's).  TD is the tile size in drones: the
// template argument TILE of chain_solve when that is given (16), this struct's field otherwise (K8).
//   lw [(M+1)] at stride 4 (waypoints of this axis) | sT [M+1] (knots) at stride 1 with a compile-time tile (a staged
//   or a global row), at stride TD otherwise (K8's drone-interleaved iterate) |
//   sX [M] at stride TD (1/T, written here) | sG [M-1][NU NU] at stride TD | sZ [M-1][NU] at stride 4 TD
struct ChainLane {
  const double *lw, *sT;
  double *sX, *sG, *sZ;
  int TD;
};

// GATES (msnap_solve_gates): interior knots may carry prescribed derivatives.  frow [M-1]: this
// drone's masks, the one of knot i at [i-1] -- bit q-1: the q-th derivative is prescribed -- and grow [M-1][4 NU] from
// this lane's axis on: its NU values per knot; frow == nullptr (wave-uniform): no gates.  Both are global memory and
// are fetched one knot ahead, as the times and waypoints are.  `invalid` comes back true for a mask outside
// 0 .. 2^NU - 1 or a prescribed value that is not finite.
struct ChainGates {
  const int32_t *frow;
  const double *grow;
  bool invalid;
};

struct ChainUnchecked {      // the default `see`
  __device__ __forceinline__ void operator()(int, double, double, double) const {}
};
struct ChainNoStatus {       // the default `swept`
  __device__ __forceinline__ void operator()() const {}
};

// u0, uM: the end knots' derivative vectors (read with ENDS only for the seed and the last knot's term; rest: zeros).
// seg(i, c, T_i): segment i's coefficients, i = M-1 .. 0.  `singular` is set before the first call of seg.
// swept(): between the sweeps, when every input has been seen and every pivot taken (the rolled solves write their
// status word there, off the recovery loop).
// see(i, t_{i+1}, w_{i+1}, T_i), i = 0 .. M-1: what the forward sweep reads of each segment, as it reads it, for a
// caller that checks its inputs on the way -- t_0 and w_0 are the caller's to look at.  The default sees nothing (K8
// has checked the input times once, and its iterates are its own).
// Nothing here acts on the knots' validity: every loop is bounded by M and wave-uniform, and the caller discards the
// results.
template <int K, bool ENDS, bool REFINE, int TILE = 0, bool GATES = false, class Seg, class See = ChainUnchecked,
          class Swept = ChainNoStatus>
__device__ __forceinline__ void chain_solve(const ChainLane &p, int M, const double (&u0)[K - 1],
                                            const double (&uM)[K - 1], bool &singular, Seg &&seg, See &&see = See{},
                                            ChainGates *gates = nullptr, Swept &&swept = Swept{}) {
  using SW = Sweep<K>;
  using C = HermiteConsts<K>;
  constexpr int NU = SW::NU, NC = SW::NC, KK = SW::KK, PM = SW::PM;
  static_assert(!REFINE || ENDS, "refine_end takes out the residual against a given end state");
  static_assert(!GATES || ENDS, "gates ride on the boundary-state solve");
  const int TD = TILE ? TILE : p.TD, QL = 4 * TD;
  const int TS = TILE ? 1 : TD;      // the knots' stride
  const double *lw = p.lw, *sT = p.sT;
  double *sX = p.sX, *sG = p.sG, *sZ = p.sZ;

  // GATES: the mask and the lane's NU values of the next knot (an unused value may be anything: it is only selected).
  // Knot 1's are asked for here, ahead of everything: they come from global memory, the rest of the set-up from LDS.
  [[maybe_unused]] bool has_gates = false;
  [[maybe_unused]] int mpre = 0;
  [[maybe_unused]] double gpre[NU];
  [[maybe_unused]] bool badgate = false;
  if constexpr (GATES) {
    has_gates = gates->frow != nullptr && M >= 2;
#pragma unroll
    for (int q = 0; q < NU; ++q) gpre[q] = 0.0;
    if (has_gates) {
      mpre = gates->frow[0];
#pragma unroll
      for (int q = 0; q < NU; ++q) gpre[q] = gates->grow[q];
    }
  }

  // ---------------- segment 0 ----------------
  const double t0 = sT[0];
  double tcur = sT[TS];
  const double w0 = lw[0];
  double wcur = lw[4];
  double T = tcur - t0;
  double x;
  if constexpr (ENDS) x = rcp64(T);
  else x = rcp64(T - t0);
  sX[0] = x;
  SW sw;
  sw.init(x, wcur - w0);
  if constexpr (ENDS) {
    double xp[PM + 1];
    SW::powers(x, xp);
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      double w = 0.0;
#pragma unroll
      for (int q = 0; q < NU; ++q) w = __builtin_fma(C::HSE[q + 1][n + 1] * xp[KK - (q + 1) - (n + 1)], u0[q], w);
      sw.Otz[n] = w;
    }
  }

  see(0, tcur, wcur, T);      // (behind the arithmetic, here and below: the checks are off the chain)

  // ---------------- forward block LDL^T sweep over interior knots ----------------
  double tpre = sT[(M >= 2 ? 2 : M) * TS];
  double wpre = lw[(M >= 2 ? 2 : M) * 4];
  double tacc = 0.0;      // REFINE: the durations before the current segment, summed as msnap_eval_flat sums them
  for (int i = 1; i < M; ++i) {
    const double tnext = tpre;
    const double wnext = wpre;
    if constexpr (REFINE) tacc = tacc + T;
    {
      const int ip = (i + 2 <= M) ? i + 2 : M;
      tpre = sT[ip * TS];
      wpre = lw[ip * 4];
    }
    [[maybe_unused]] unsigned mask = 0u;
    [[maybe_unused]] double gv[NU];
    if constexpr (GATES) {
      const int mi = mpre;
#pragma unroll
      for (int q = 0; q < NU; ++q) gv[q] = gpre[q];
      if (has_gates) {
        const int kn = (i + 1 < M) ? i : M - 2;      // knot i+1 sits at [i]; the last knot is read twice
        mpre = gates->frow[kn];
#pragma unroll
        for (int q = 0; q < NU; ++q) gpre[q] = gates->grow[(size_t)kn * (4 * NU) + q];
      }
      badgate |= (mi < 0) | (mi >= (1 << NU));
      mask = (unsigned)mi & ((1u << NU) - 1u);
#pragma unroll
      for (int q = 0; q < NU; ++q) badgate |= (bool)((mask >> q) & 1u) & !finite64(gv[q]);
    }
    T = tnext - tcur;
    x = rcp64(T);
    sX[i * TD] = x;
    double G[NU][NU], z[NU];
    if constexpr (GATES) {
      // one wave-uniform test per knot: a knot no drone of the tile gates takes the plain step (the same bits as the
      // masked one with empty masks, without its selects)
      if (__builtin_amdgcn_ballot_w64(mask != 0u) != 0) sw.template step_masked<true>(x, wnext - wcur, mask, gv, G, z);
      else sw.step(x, wnext - wcur, G, z);
    } else {
      sw.step(x, wnext - wcur, G, z);
    }
    double *g = sG + (size_t)(i - 1) * (NU * NU * TD);
    double *zz = sZ + (size_t)(i - 1) * (NU * QL);
#pragma unroll
    for (int r = 0; r < NU; ++r) {
#pragma unroll
      for (int c = 0; c < NU; ++c) g[(r * NU + c) * TD] = G[r][c];
      zz[r * QL] = z[r];
    }
    see(i, tnext, wnext, T);
    tcur = tnext;
    wcur = wnext;
  }
  singular = sw.singular;
  if constexpr (GATES) gates->invalid = badgate;
  swept();

  // ---------------- backward sweep + coefficient recovery ----------------
  double un[NU], zq[NU], gq[NU][NU];
#pragma unroll
  for (int r = 0; r < NU; ++r) un[r] = uM[r];
  double wn = wcur, tn = tcur;   // w_M, t_M
  // REFINE: the local time msnap_eval_state evaluates the last segment at when asked for the sum of the durations
  const double tl_end = (tacc + T) - tacc;
  double wq = lw[(M - 1) * 4], xq1 = sX[(M - 1) * TD];
  if (M >= 2) {      // stash slot M-2 holds knot M-1
    const double *zz = sZ + (size_t)(M - 2) * (NU * QL);
    const double *g = sG + (size_t)(M - 2) * (NU * NU * TD);
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      zq[r] = zz[r * QL];
#pragma unroll
      for (int c = 0; c < NU; ++c) gq[r][c] = g[(r * NU + c) * TD];
    }
  } else {           // one segment: no knot, no stash
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      zq[r] = 0.0;
#pragma unroll
      for (int c = 0; c < NU; ++c) gq[r][c] = 0.0;
    }
  }
  for (int i = M - 1; i >= 0; --i) {
    double u[NU];
    const double wi = wq;
    const double xi = xq1;
    const double ti = sT[i * TS];
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      double v = zq[r];
      // rest: u_M = 0 and the term is skipped at the last knot -- fma(-g, 0, v) is not v for a zero of the other sign
      // or a non-finite g
      if (ENDS || i < M - 1) {
#pragma unroll
        for (int c = 0; c < NU; ++c) v = __builtin_fma(-gq[r][c], un[c], v);
      }
      u[r] = (i >= 1) ? v : u0[r];      // segment 0 starts from u_0
    }
    if (i >= 1) {
      wq = lw[(i - 1) * 4];
      xq1 = sX[(i - 1) * TD];
      if (i >= 2) {
        const double *zz = sZ + (size_t)(i - 2) * (NU * QL);
        const double *g = sG + (size_t)(i - 2) * (NU * NU * TD);
#pragma unroll
        for (int r = 0; r < NU; ++r) {
          zq[r] = zz[r * QL];
#pragma unroll
          for (int c = 0; c < NU; ++c) gq[r][c] = g[(r * NU + c) * TD];
        }
      }
    }
    double c[NC];
    recover_segment<K>(wi, wn - wi, xi, u, un, c);
    if constexpr (REFINE) {
      if (i == M - 1) refine_end<K>(c, tl_end, xi, wn, un);
    }
    seg(i, c, tn - ti);
#pragma unroll
    for (int r = 0; r < NU; ++r) un[r] = u[r];
    wn = wi;
    tn = ti;
  }
}

// The rolled solves: what stands around chain_solve in solve_kernel<K, GS>, states_solve_kernel<K> and
// gates_solve_kernel<K> -- the end vectors, the input checks, the status word, segment 0's shift, the stores.

// The gates of a batch (GATES; msnap_solve_gates), in global memory as the caller gave them: fix[n_drones][M-1] and
// via[n_drones][M-1][4][K-1] (ChainGates has the meaning).  fix == nullptr (wave-uniform): no gates.
struct RolledGates {
  const int32_t *fix;
  const double *via;
};

// GS: stash on a global slab, operands read from global memory, durations written here (nothing is staged).
// ENDS: the end knots' derivative vectors u_0, u_M are data (has_start / has_end: wave-uniform, a missing one is rest),
// checked like every other input, and the first time must be 0: the start-row quirk has no meaning for a path that
// starts from a moving state.  GATES (with ENDS): interior knots may carry prescribed derivatives.
template <int K, bool GS, bool ENDS, bool GATES = false>
__device__ __forceinline__ void rolled_solve_tile(const RolledTile &p, const double *__restrict__ wp,
                                                  const double *__restrict__ tt, int shared_times, bool has_start,
                                                  bool has_end, int M, int tile, int nvalid, int lane,
                                                  double *__restrict__ coef, double *__restrict__ dur,
                                                  int32_t *__restrict__ status, RolledGates gates = {}) {
  constexpr int NU = K - 1, NC = 2 * K, PITCH = NU | 1;
  static_assert(!(GS && ENDS), "the boundary-state solve has no slab variant");
  // PRECONDITION: `lane` is threadIdx.x and the order-9 transpose image is the start of dynamic LDS, as in every caller
  // (solve_kernel, states_solve_kernel, gates_solve_kernel: one wave per block, Tr first in each layout).  The store
  // below names these two facts of the launch as such instead of capturing them.  Read
  // from a closure they would reach store_segment_coalesced<10> as values out of memory, and the compiler's
  // interprocedural constant and range propagation, which runs before inlining and for all kernels of a translation
  // unit at once, would stop folding them into the helper: solve_kernel_reg<5, 10 | 20>, which never come here, grow by
  // 82 / 120 instructions (profiles/chain_solve_ab.md; profiles/rolled_merge_ab.md met the same with a struct).
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int dl = lane >> 2;
  const int a = lane & 3;
  const int wpitch = (M + 1) * 4;
  const int tpitch = M + 1;

  // lanes past the end of the batch replay the last valid drone's inputs into a stash column of their own (and store
  // on top of its results)
  const bool live = dl < nvalid;
  const int dloc = live ? dl : nvalid - 1;
  const int d = tile * kDronesPerWave + dloc;
  [[maybe_unused]] double *drow = dur + (size_t)d * M;
  ChainLane cl = {nullptr, nullptr, p.sX + dl, p.sG + dl, p.sZ + lane, 0};      // (TD: the tile is a template argument)
  if constexpr (GS) {
    cl.lw = wp + (size_t)d * (size_t)wpitch + a;
    cl.sT = shared_times ? tt : tt + (size_t)d * (size_t)tpitch;
  } else {
    cl.lw = p.sWraw + dloc * wpitch + a;
    cl.sT = p.sTraw + (shared_times ? 0 : dloc * tpitch);
  }
  [[maybe_unused]] ChainGates cg = {nullptr, nullptr, false};
  if constexpr (GATES) {
    if (gates.fix != nullptr && M >= 2) {
      cg.frow = gates.fix + (size_t)d * (size_t)(M - 1);
      cg.grow = gates.via + ((size_t)d * (size_t)(M - 1) * 4 + a) * NU;
    }
  }

  double u0[NU], uM[NU];
  bool nonfinite = false, badtime = false;
#pragma unroll
  for (int q = 0; q < NU; ++q) {
    if constexpr (ENDS) {
      const int sl = (dloc * 4 + a) * PITCH;
      u0[q] = has_start ? p.sS0[sl + q] : 0.0;
      uM[q] = has_end ? p.sS1[sl + q] : 0.0;
      nonfinite |= !finite64(u0[q]) | !finite64(uM[q]);
    } else {
      u0[q] = uM[q] = 0.0;
    }
  }
  const double t0 = cl.sT[0], w0 = cl.lw[0];

  bool singular;
  int st = MSNAP_ST_OK;
  chain_solve<K, ENDS, /*REFINE*/ ENDS, kDronesPerWave, GATES>(
      cl, M, u0, uM, singular,
      [&](int i, double (&c)[NC], double) {
        if constexpr (!ENDS) {
          // segment 0 was solved in s - t0
          if (i == 0 && t0 != 0.0) taylor_shift<NC>(c, -t0);
        }
        if constexpr (NC == 8)
          store_segment_quad8(MSNAP_SEG_BASE(coef, tile, M, i, NC), MSNAP_SEG_STRIDE(M, NC), nvalid, lane, c, st != 0);
        else
          store_segment_coalesced<NC>(reinterpret_cast<double2 *>(lds), MSNAP_SEG_BASE(coef, tile, M, i, NC),
                                      MSNAP_SEG_STRIDE(M, NC), nvalid, (int)threadIdx.x, c, st != 0);
      },
      [&](int i, double t, double w, double T) {
        if (i == 0) {
          nonfinite |= !(finite64(t0) & finite64(t) & finite64(w0) & finite64(w));
          if constexpr (ENDS) badtime = !(T > 0.0) | (t0 != 0.0);
          else badtime = !(T > 0.0) | !(T - t0 > 0.0) | (t0 < 0.0);
        } else {
          nonfinite |= !finite64(t) | !finite64(w);
          badtime |= !(T > 0.0);
        }
        if constexpr (GS) {
          if (live && a == 0) drow[i] = T;
        }
      },
      &cg,
      [&]() {
        st = drone_status(nonfinite | cg.invalid, badtime, singular);
        if (live && a == 0) status[tile * kDronesPerWave + dl] = st;
      });
}


// LDS of one 16-drone tile of the boundary-state solves (states_solve_kernel, gates_solve_kernel), in doubles:
//   Tr[NC/2][68][2] (order 9 only: the output transpose image) | Wraw[16][(M+1) 4] | Traw[16][M+1] |
//   S0[64][pitch] | S1[64][pitch] (start and end state of every lane) |
//   X[M][16] | G[M-1][NU NU][16] | Z[M-1][NU][64]
// The state blocks keep a lane's NU values side by side at an odd pitch (3 at order 7, 5 at order 9): ds_read_b64
// serves 32 lanes per cycle over 64 four-byte banks, and 2 pitch l mod 64 is one-to-one for l < 32 only if pitch is odd.
template <int K>
struct StatesLayout {
  static constexpr int NU = K - 1, NC = 2 * K;
  static constexpr int kPitch = NU | 1;
  static constexpr size_t kTrWords = NC == 8 ? 0 : (size_t)(NC / 2) * kTrPitch * 2;
  static constexpr size_t kStateWords = (size_t)kWave * kPitch;
  static constexpr size_t words(int M) {
    return kTrWords + (size_t)16 * (M + 1) * 5 + 2 * kStateWords + (size_t)16 * M +
           (size_t)(M - 1) * (16 * NU * NU + 64 * NU);
  }
  static constexpr size_t bytes(int M) { return words(M) * sizeof(double); }
  static constexpr int max_segments() {
    int M = 1;
    while (bytes(M + 1) <= kMaxLdsBytes) ++M;
    return M;
  }
};
static_assert(StatesLayout<4>::max_segments() == 47 && StatesLayout<5>::max_segments() == 32,
              "DESIGN.md K13, K21 and include/msnap.h quote these");

}  // namespace msnap
