// The rolled solve of one 16-drone tile: the body of solve_kernel<K, GS> (msnap_solve.hip, rest to rest), of
// states_solve_kernel<K> (msnap_states.hip, given end states) and of gates_solve_kernel<K> (msnap_gates.hip, prescribed
// derivatives at interior knots as well).  lane = 4 drone + axis; the tile's inputs are staged in
// LDS by the caller (GS: read from global memory here), the knot loops are rolled over Sweep<K>::step, X / G / Z are
// stashed in LDS or on a global slab, and every segment leaves through recover_segment and the full-line stores.
// The callers carve their own layouts -- they differ on purpose -- and pass the pointers; what the solves do
// differently is one `if constexpr` each below.
#pragma once

#include "msnap_sweep.h"

namespace msnap {

// Where the caller put a tile's images (doubles; sS0 / sS1, the lanes' end states at pitch (K - 1) | 1, for ENDS only).
// The output transpose image sTr (order 9) travels beside the struct as an argument of its own: in every layout it is
// the start of dynamic LDS, and passed as that constant the compiler folds it into store_segment_coalesced for all
// kernels of a translation unit at once -- through the struct it stops doing so for solve_kernel_reg<5, *> as well.
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

// The gates of a batch (GATES; msnap_solve_gates), in global memory as the caller gave them:
// fix[n_drones][M-1] the mask of interior knot i at [i-1] -- bit q-1: the q-th derivative is prescribed, on the
// drone's four axes -- and via[n_drones][M-1][4][K-1] the values.  fix == nullptr (wave-uniform): no gates.
struct RolledGates {
  const int32_t *fix;
  const double *via;
};

// GS: stash on a global slab, operands read from global memory, durations written here (nothing is staged).
// ENDS: the end knots' derivative vectors u_0, u_M are data (has_start / has_end: wave-uniform, a missing one is rest).
// GATES (with ENDS): interior knots may carry prescribed derivatives; a knot's mask and values are fetched from global
// memory one knot ahead, as tpre / wpre are from LDS, and the knot goes through Sweep<K>::step_masked.
template <int K, bool GS, bool ENDS, bool GATES = false>
__device__ __forceinline__ void rolled_solve_tile(const RolledTile &p, double2 *sTr, const double *__restrict__ wp,
                                                  const double *__restrict__ tt, int shared_times, bool has_start,
                                                  bool has_end, int M, int tile, int nvalid, int lane,
                                                  double *__restrict__ coef, double *__restrict__ dur,
                                                  int32_t *__restrict__ status, RolledGates gates = {}) {
  using SW = Sweep<K>;
  using C = HermiteConsts<K>;
  constexpr int NU = SW::NU, NC = SW::NC, KK = SW::KK, PM = SW::PM, PITCH = NU | 1;
  static_assert(!(GS && ENDS), "the boundary-state solve has no slab variant");
  static_assert(!GATES || ENDS, "gates ride on the boundary-state solve");
  const int dl = lane >> 2;
  const int a = lane & 3;
  const int wpitch = (M + 1) * 4;
  const int tpitch = M + 1;
  double *sX = p.sX, *sG = p.sG, *sZ = p.sZ;

  // lanes past the end of the batch replay the last valid drone (and store on top of its results)
  const bool live = dl < nvalid;
  const int dloc = live ? dl : nvalid - 1;
  const int d = tile * kDronesPerWave + dloc;
  const double *wrow = wp + (size_t)d * (size_t)wpitch + a;
  const double *trow = shared_times ? tt : tt + (size_t)d * (size_t)tpitch;
  double *drow = dur + (size_t)d * M;
  const double *lw = p.sWraw + dloc * wpitch + a;
  const double *lt = p.sTraw + (shared_times ? 0 : dloc * tpitch);
  auto Wv = [&](int i) -> double { if constexpr (GS) return wrow[(size_t)i * 4]; else return lw[i * 4]; };
  auto Tv = [&](int i) -> double { if constexpr (GS) return trow[i]; else return lt[i]; };

  // GATES: the mask and the lane's NU values of the next knot (an unused value may be anything: it is only selected).
  // Knot 1's are asked for here, ahead of everything: they come from global memory, the rest of the set-up from LDS.
  [[maybe_unused]] const bool has_gates = GATES && gates.fix != nullptr && M >= 2;
  [[maybe_unused]] const int32_t *frow = nullptr;
  [[maybe_unused]] const double *grow = nullptr;
  [[maybe_unused]] int mpre = 0;
  [[maybe_unused]] double gpre[NU];
  if constexpr (GATES) {
#pragma unroll
    for (int q = 0; q < NU; ++q) gpre[q] = 0.0;
    if (has_gates) {
      frow = gates.fix + (size_t)d * (size_t)(M - 1);
      grow = gates.via + ((size_t)d * (size_t)(M - 1) * 4 + a) * NU;
      mpre = frow[0];
#pragma unroll
      for (int q = 0; q < NU; ++q) gpre[q] = grow[q];
    }
  }

  // ---------------- start of the chain: the end knots' derivatives ----------------
  double u0[NU], uM[NU];
  bool nonfinite = false;
#pragma unroll
  for (int q = 0; q < NU; ++q) {
    if constexpr (ENDS) {      // data, and checked like every other input
      const int sl = (dloc * 4 + a) * PITCH;
      u0[q] = has_start ? p.sS0[sl + q] : 0.0;
      uM[q] = has_end ? p.sS1[sl + q] : 0.0;
      nonfinite |= !finite64(u0[q]) | !finite64(uM[q]);
    } else {                   // rest
      u0[q] = uM[q] = 0.0;
    }
  }

  // ---------------- segment 0 ----------------
  const double t0 = Tv(0);
  double tcur = Tv(1);
  const double w0 = Wv(0);
  double wcur = Wv(1);
  nonfinite |= !(finite64(t0) & finite64(tcur) & finite64(w0) & finite64(wcur));
  double T = tcur - t0;
  bool badtime;
  double x;
  if constexpr (ENDS) {
    // the first time must be 0: the start-row quirk below has no meaning for a path that starts from a moving state
    badtime = !(T > 0.0) | (t0 != 0.0);
    x = rcp64(T);
  } else {
    // the reference takes segment 0's start rows at local time t[0] (Appendix-A quirk, see taylor_shift())
    const double Teff = T - t0;
    badtime = !(T > 0.0) | !(Teff > 0.0) | (t0 < 0.0);
    if constexpr (GS) {
      if (live && a == 0) drow[0] = T;
    }
    x = rcp64(Teff);
  }
  sX[0 * 16 + dl] = x;
  SW sw;
  sw.init(x, wcur - w0);
  if constexpr (ENDS) {
    // knot 1 sees the start state through the coupling block of segment 0: Otz = O_0^T u_0 (y_1 = -yb_1 - Otz)
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

  // ---------------- forward block LDL^T sweep over interior knots ----------------
  // operands of knot i+1 are fetched one iteration ahead (LDS latency off the chain)
  double tpre = Tv(M >= 2 ? 2 : M);
  double wpre = Wv(M >= 2 ? 2 : M);
  double tacc = 0.0;      // ENDS: the durations before the current segment, summed as msnap_eval_flat sums them
  for (int i = 1; i < M; ++i) {
    const double tnext = tpre;
    const double wnext = wpre;
    if constexpr (ENDS) tacc = tacc + T;
    {
      const int ip = (i + 2 <= M) ? i + 2 : M;
      tpre = Tv(ip);
      wpre = Wv(ip);
    }
    [[maybe_unused]] unsigned mask = 0u;
    [[maybe_unused]] double gv[NU];
    if constexpr (GATES) {
      const int mi = mpre;
#pragma unroll
      for (int q = 0; q < NU; ++q) gv[q] = gpre[q];
      if (has_gates) {
        const int kn = (i + 1 < M) ? i : M - 2;      // knot i+1 sits at [i]; the last knot is read twice
        mpre = frow[kn];
#pragma unroll
        for (int q = 0; q < NU; ++q) gpre[q] = grow[(size_t)kn * (4 * NU) + q];
      }
      // a mask outside 0 .. 2^NU - 1, or a prescribed value that is not finite, fails the drone like any other input
      nonfinite |= (mi < 0) | (mi >= (1 << NU));
      mask = (unsigned)mi & ((1u << NU) - 1u);
#pragma unroll
      for (int q = 0; q < NU; ++q) nonfinite |= (bool)((mask >> q) & 1u) & !finite64(gv[q]);
    }
    nonfinite |= !finite64(tnext) | !finite64(wnext);
    T = tnext - tcur;
    badtime |= !(T > 0.0);
    if constexpr (GS) {
      if (live && a == 0) drow[i] = T;
    }
    x = rcp64(T);
    sX[i * 16 + dl] = x;
    double G[NU][NU], z[NU];
    if constexpr (GATES) {
      // one wave-uniform test per knot: a knot no drone of the tile gates takes the plain step (the same bits as the
      // masked one with empty masks, without its selects)
      if (__builtin_amdgcn_ballot_w64(mask != 0u) != 0) sw.template step_masked<true>(x, wnext - wcur, mask, gv, G, z);
      else sw.step(x, wnext - wcur, G, z);
    } else {
      sw.step(x, wnext - wcur, G, z);
    }
    double *g = sG + (size_t)(i - 1) * (NU * NU * 16) + dl;
    double *zz = sZ + (size_t)(i - 1) * (NU * 64) + lane;
#pragma unroll
    for (int r = 0; r < NU; ++r) {
#pragma unroll
      for (int c = 0; c < NU; ++c) g[(r * NU + c) * 16] = G[r][c];
      zz[r * 64] = z[r];
    }
    tcur = tnext;
    wcur = wnext;
  }

  const int st = drone_status(nonfinite, badtime, sw.singular);
  if (live && a == 0) status[tile * kDronesPerWave + dl] = st;
  const bool bad = st != 0;

  // ---------------- backward sweep + coefficient recovery ----------------
  // u_i = z_i - G_i u_{i+1} from u_M (the stash holds G of every knot, the last one included; with two segments the one
  // knot receives both end terms); operands of segment i-1 are fetched while segment i is being recovered
  double un[NU], zq[NU], gq[NU][NU];
#pragma unroll
  for (int r = 0; r < NU; ++r) un[r] = uM[r];
  double wn = wcur;   // w_M
  // ENDS: the local time msnap_eval_state evaluates the last segment at when asked for the sum of the durations
  const double tl_end = (tacc + T) - tacc;
  double wq = Wv(M - 1), xq1 = sX[(M - 1) * 16 + dl];
  if (M >= 2) {      // stash slot M-2 holds knot M-1
    const double *zz = sZ + (size_t)(M - 2) * (NU * 64) + lane;
    const double *g = sG + (size_t)(M - 2) * (NU * NU * 16) + dl;
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      zq[r] = zz[r * 64];
#pragma unroll
      for (int c = 0; c < NU; ++c) gq[r][c] = g[(r * NU + c) * 16];
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
      wq = Wv(i - 1);
      xq1 = sX[(i - 1) * 16 + dl];
      if (i >= 2) {
        const double *zz = sZ + (size_t)(i - 2) * (NU * 64) + lane;
        const double *g = sG + (size_t)(i - 2) * (NU * NU * 16) + dl;
#pragma unroll
        for (int r = 0; r < NU; ++r) {
          zq[r] = zz[r * 64];
#pragma unroll
          for (int c = 0; c < NU; ++c) gq[r][c] = g[(r * NU + c) * 16];
        }
      }
    }
    double c[NC];
    recover_segment<K>(wi, wn - wi, xi, u, un, c);
    if constexpr (ENDS) {
      // the last segment takes one refinement step on its end conditions
      if (i == M - 1) refine_end<K>(c, tl_end, xi, wn, un);
    } else {
      // segment 0 was solved in s - t0
      if (i == 0 && t0 != 0.0) taylor_shift<NC>(c, -t0);
    }
    if constexpr (NC == 8)
      store_segment_quad8(MSNAP_SEG_BASE(coef, tile, M, i, NC), MSNAP_SEG_STRIDE(M, NC), nvalid, lane, c, bad);
    else
      store_segment_coalesced<NC>(sTr, MSNAP_SEG_BASE(coef, tile, M, i, NC), MSNAP_SEG_STRIDE(M, NC), nvalid, lane, c,
                                  bad);
#pragma unroll
    for (int r = 0; r < NU; ++r) un[r] = u[r];
    wn = wi;
  }
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
