// The arithmetic every solve variant shares, and their common input / output helpers: the forward recurrence
// Sweep<K>, recover_segment, the coalesced store helpers and the LDS input stage.  Included by msnap_solve.hip
// (K1) and msnap_timeopt.hip (K8), so that both run the same instruction sequence per knot and segment.
#pragma once

#include "msnap_consts.h"
#include "msnap_twist_consts.h"
#include "msnap_internal.h"
#include "msnap_solve_plan.h"   // kTrPitch
#include "msnap_energy.h"
#include "msnap_wave.h"

namespace msnap {

__device__ __forceinline__ constexpr int sidx(int r, int c) {  // symmetric lower, r >= c
  return r * (r + 1) / 2 + c;
}

__device__ __forceinline__ double rcp64(double v) {
  // v_rcp_f64 seed (2^-24) + two Newton steps (1 ulp, tools/micro/rcp_micro.hip); inputs are
  // durations / SPD pivots in a sane range (status flags catch the rest), so no denormal/overflow fix-up.
  double r = __builtin_amdgcn_rcp(v);
  double e = __builtin_fma(-v, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-v, r, 1.0);
  r = __builtin_fma(r, e, r);
  return r;
}

__device__ __forceinline__ bool finite64(double v) { return __builtin_isfinite(v); }

// Where knot_geom_xp / end_side / recover_segment take their Hermite constants from.  The default is the literal:
// every kernel but the twisted one compiles exactly as if the bodies named HermiteConsts<K> themselves.
template <int K>
struct LiteralHermite {
  using C = HermiteConsts<K>;
  __device__ __forceinline__ double hss(int n, int m) const { return C::HSS[n][m]; }
  __device__ __forceinline__ double hee(int n, int m) const { return C::HEE[n][m]; }
  __device__ __forceinline__ double hse(int n, int m) const { return C::HSE[n][m]; }
  __device__ __forceinline__ double cs(int m, int n) const { return C::CS[m][n]; }
  __device__ __forceinline__ double ce(int m, int n) const { return C::CE[m][n]; }
  __device__ __forceinline__ double invfact(int n) const { return C::INVFACT[n]; }
};

// The same constants held in (scalar) registers that the caller filled from the table of msnap_twist_consts.h:
// `sw` the sweep set, `rc` the recovery set.  A code of 0 keeps the literal (inline operands).
template <int K, bool REC = true>   // REC false: the recovery set stays literal (the registers do not hold both sets)
struct TableHermite {
  using C = HermiteConsts<K>;
  using L = TwistConstLayout<K>;
  static constexpr int NSW = L::n_sweep, NRC = REC ? L::n_rec : 0;
  double sw[NSW], rc[REC ? L::n_rec : 1];
  __device__ __forceinline__ static double pick(int code, double lit, const double *tab) {
    return code == 0 ? lit : tab[code - 1];
  }
  __device__ __forceinline__ double hss(int n, int m) const { return pick(TwistMapOf<K>::map.hss[n][m], C::HSS[n][m], sw); }
  __device__ __forceinline__ double hee(int n, int m) const { return pick(TwistMapOf<K>::map.hee[n][m], C::HEE[n][m], sw); }
  __device__ __forceinline__ double hse(int n, int m) const { return pick(TwistMapOf<K>::map.hse[n][m], C::HSE[n][m], sw); }
  __device__ __forceinline__ double cs(int m, int n) const { return pick(!REC ? 0 : TwistMapOf<K>::map.cs[m][n], C::CS[m][n], rc); }
  __device__ __forceinline__ double ce(int m, int n) const { return pick(!REC ? 0 : TwistMapOf<K>::map.ce[m][n], C::CE[m][n], rc); }
  __device__ __forceinline__ double invfact(int n) const { return pick(!REC ? 0 : TwistMapOf<K>::map.inv[n], C::INVFACT[n], rc); }
};

// ------------------------------------------------------------------------------------
// the forward recurrence carried from knot to knot
// ------------------------------------------------------------------------------------
template <int K>
struct Sweep {
  static constexpr int NU = K - 1;            // unknown derivatives per interior knot
  static constexpr int NC = 2 * K;            // coefficients per segment
  static constexpr int KK = 2 * K - 1;        // polynomial order
  static constexpr int NS = NU * (NU + 1) / 2;
  static constexpr int PM = 2 * K - 2;        // highest power of 1/T in the sweep
  using C = HermiteConsts<K>;

  double E[NS], re[NU];                       // end side of the previous segment
  double OtG[NS], Otz[NU];                    // O_{i-1}^T G_{i-1} (symmetric) and O_{i-1}^T z_{i-1}
  bool singular;

  __device__ __forceinline__ static void powers(double x, double (&xp)[PM + 1]) {
    xp[0] = 1.0;
    xp[1] = x;
#pragma unroll
    for (int p = 2; p <= PM; ++p) xp[p] = xp[p - 1] * x;
  }

  template <class P = LiteralHermite<K>>
  __device__ __forceinline__ void end_side(const double (&xp)[PM + 1], double dw, P hc = P()) {
#pragma unroll
    for (int n = 1; n <= NU; ++n) {
#pragma unroll
      for (int m = 1; m <= n; ++m) E[sidx(n - 1, m - 1)] = hc.hee(n, m) * xp[KK - n - m];
      re[n - 1] = (hc.hee(n, 0) * xp[KK - n]) * dw;
    }
  }

  // segment 0 (x = 1/T_0, dw = w_1 - w_0): only its end side feeds knot 1
  template <class P = LiteralHermite<K>>
  __device__ __forceinline__ void init(double x, double dw, P hc = P()) {
    double xp[PM + 1];
    powers(x, xp);
    end_side(xp, dw, hc);
    singular = false;
#pragma unroll
    for (int r = 0; r < NU; ++r) Otz[r] = 0.0;
#pragma unroll
    for (int e = 0; e < NS; ++e) OtG[e] = 0.0;
  }

  // Everything of knot i that depends on segment lengths and waypoints only (not on the
  // recurrence): diagonal block D_i, coupling block O_i, the right-hand side before the Schur
  // correction, and the end side of segment i for knot i+1.
  struct Knot {
    double D[NS], O[NU][NU], yb[NU], E[NS], re[NU];
  };

  // from segment i (x = 1/T_i, dw = w_{i+1} - w_i) and the end side (Eprev, reprev) of segment i-1
  __device__ __forceinline__ static void knot_geom(double x, double dw, const double (&Eprev)[NS],
                                                   const double (&reprev)[NU], Knot &k) {
    double xp[PM + 1];
    powers(x, xp);
    knot_geom_xp(xp, dw, Eprev, reprev, k);
  }

  // the same from the powers of x = 1/T_i (for callers that prepare them ahead of the recurrence)
  template <class P = LiteralHermite<K>>
  __device__ __forceinline__ static void knot_geom_xp(const double (&xp)[PM + 1], double dw,
                                                      const double (&Eprev)[NS], const double (&reprev)[NU],
                                                      Knot &k, P hc = P()) {
#pragma unroll
    for (int n = 1; n <= NU; ++n) {
#pragma unroll
      for (int m = 1; m <= n; ++m) {
        k.D[sidx(n - 1, m - 1)] = __builtin_fma(hc.hss(n, m), xp[KK - n - m], Eprev[sidx(n - 1, m - 1)]);
        k.E[sidx(n - 1, m - 1)] = hc.hee(n, m) * xp[KK - n - m];
      }
      k.yb[n - 1] = __builtin_fma(hc.hse(n, 0) * xp[KK - n], dw, reprev[n - 1]);
      k.re[n - 1] = (hc.hee(n, 0) * xp[KK - n]) * dw;
#pragma unroll
      for (int m = 1; m <= NU; ++m) k.O[n - 1][m - 1] = hc.hse(n, m) * xp[KK - n - m];
    }
  }

  // LDL^T of the symmetric block S in place (strict lower part -> L, dinv -> 1/d); returns true
  // if a pivot is not positive and finite
  __device__ __forceinline__ static bool ldl_factor(double (&S)[NS], double (&dinv)[NU]) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      double dj = S[sidx(j, j)];
#pragma unroll
      for (int p = 0; p < j; ++p) dj = __builtin_fma(-S[sidx(j, p)] * dinv[p], S[sidx(j, p)], dj);
      bad |= !(dj > 0.0) | !finite64(dj);   // bitwise: no short-circuit branches
      dinv[j] = rcp64(dj);
#pragma unroll
      for (int r = j + 1; r < NU; ++r) {
        double v = S[sidx(r, j)];
#pragma unroll
        for (int p = 0; p < j; ++p) v = __builtin_fma(-S[sidx(r, p)] * dinv[p], S[sidx(j, p)], v);
        S[sidx(r, j)] = v;     // w_rj = L_rj d_j until scaled below
      }
    }
#pragma unroll
    for (int r = 1; r < NU; ++r)
#pragma unroll
      for (int p = 0; p < r; ++p) S[sidx(r, p)] *= dinv[p];
    return bad;
  }

  // v <- S^-1 v with the factor of ldl_factor
  __device__ __forceinline__ static void ldl_solve(const double (&S)[NS], const double (&dinv)[NU], double (&v)[NU]) {
#pragma unroll
    for (int r = 1; r < NU; ++r)
#pragma unroll
      for (int p = 0; p < r; ++p) v[r] = __builtin_fma(-S[sidx(r, p)], v[p], v[r]);
#pragma unroll
    for (int r = 0; r < NU; ++r) v[r] *= dinv[r];
#pragma unroll
    for (int r = NU - 2; r >= 0; --r)
#pragma unroll
      for (int p = r + 1; p < NU; ++p) v[r] = __builtin_fma(-S[sidx(p, r)], v[p], v[r]);
  }

  // the recurrence proper: S_i = D_i - O_{i-1}^T G_{i-1}, LDL^T, G_i = S_i^-1 O_i, z_i = S_i^-1 y_i,
  // and the Schur terms carried to knot i+1.  Returns false if a pivot is not positive and finite.
  __device__ __forceinline__ bool chain(const Knot &k, double (&G)[NU][NU], double (&z)[NU]) {
    return chain_masked<false>(k, 0u, nullptr, G, z);
  }

  // The same with some components of u_i prescribed (GATED): bit c of `mask` fixes u_i[c] = g[c].
  // The known column goes to the right-hand side of the free rows, row and column c of S become those of the identity
  // and y[c] = g[c], and the G solves take O_i with row c zeroed -- so z[c] = g[c] and row c of G is zero exactly.  The
  // carry keeps the whole O_i: knot i+1's equations hold O_i^T u_i in full.  Masked terms are selected, never multiplied
  // in: an empty mask leaves every operation of chain() as it is, and g[c] under a clear bit is not used.
  template <bool GATED>
  __device__ __forceinline__ bool chain_masked(const Knot &k, unsigned mask, const double *g, double (&G)[NU][NU],
                                               double (&z)[NU]) {
    double S[NS], y[NU];
#pragma unroll
    for (int n = 0; n < NU; ++n) {
#pragma unroll
      for (int m = 0; m <= n; ++m) S[sidx(n, m)] = k.D[sidx(n, m)] - OtG[sidx(n, m)];
      y[n] = -k.yb[n] - Otz[n];
    }
    if constexpr (GATED) {
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        const bool fc = (mask >> c) & 1u;
#pragma unroll
        for (int r = 0; r < NU; ++r) {
          if (r == c) continue;
          const bool fr = (mask >> r) & 1u;
          const double s = S[r > c ? sidx(r, c) : sidx(c, r)];
          y[r] = (fc & !fr) ? __builtin_fma(-s, g[c], y[r]) : y[r];
        }
      }
#pragma unroll
      for (int n = 0; n < NU; ++n) {
        const bool fn = (mask >> n) & 1u;
#pragma unroll
        for (int m = 0; m < n; ++m) S[sidx(n, m)] = (fn | (bool)((mask >> m) & 1u)) ? 0.0 : S[sidx(n, m)];
        S[sidx(n, n)] = fn ? 1.0 : S[sidx(n, n)];
        y[n] = fn ? g[n] : y[n];
      }
    }

    double dinv[NU];
    const bool bad = ldl_factor(S, dinv);

    // NU + 1 solves with the factor: columns of O_i, then y
#pragma unroll
    for (int c = 0; c <= NU; ++c) {
      double v[NU];
#pragma unroll
      for (int r = 0; r < NU; ++r) v[r] = (c < NU) ? k.O[r][c < NU ? c : 0] : y[r];
      if constexpr (GATED) {
        if (c < NU) {
#pragma unroll
          for (int r = 0; r < NU; ++r) v[r] = ((mask >> r) & 1u) ? 0.0 : v[r];
        }
      }
      ldl_solve(S, dinv, v);
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        if (c < NU) G[r][c < NU ? c : 0] = v[r];
        else z[r] = v[r];
      }
    }

    // carry to knot i+1: the Schur terms O_i^T G_i, O_i^T z_i
#pragma unroll
    for (int n = 0; n < NU; ++n) {
#pragma unroll
      for (int m = 0; m <= n; ++m) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < NU; ++q) v = __builtin_fma(k.O[q][n], G[q][m], v);
        OtG[sidx(n, m)] = v;
      }
      double w = 0.0;
#pragma unroll
      for (int q = 0; q < NU; ++q) w = __builtin_fma(k.O[q][n], z[q], w);
      Otz[n] = w;
    }
    return !bad;
  }

  // knot i with segment i (x = 1/T_i, dw = w_{i+1} - w_i) on its right: geometry, then recurrence
  __device__ __forceinline__ void step(double x, double dw, double (&G)[NU][NU], double (&z)[NU]) {
    step_masked<false>(x, dw, 0u, nullptr, G, z);
  }
  template <bool GATED>
  __device__ __forceinline__ void step_masked(double x, double dw, unsigned mask, const double *g, double (&G)[NU][NU],
                                              double (&z)[NU]) {
    Knot k;
    knot_geom(x, dw, E, re, k);
    singular |= !chain_masked<GATED>(k, mask, g, G, z);
#pragma unroll
    for (int e = 0; e < NS; ++e) E[e] = k.E[e];
#pragma unroll
    for (int r = 0; r < NU; ++r) re[r] = k.re[r];
  }
};

// monomial coefficients of one segment from its endpoint states
// (u = d_i[1..k-1], un = d_{i+1}[1..k-1], xi = 1/T_i, dwi = w_{i+1} - w_i):
//   c_{K+m} = x^(K+m) [ CE_m0 dw + sum_n T^n (CS_mn u_n + CE_mn un_n) ]
//           = x^(m+1) [ CE_m0 dw x^(K-1) + sum_n (CS_mn x^(K-1-n) u_n + CE_mn x^(K-1-n) un_n) ]
// -- powers of x only, so callers need not keep T_i.
template <int K, class P = LiteralHermite<K>>
__device__ __forceinline__ void recover_segment(double wi, double dwi, double xi, const double (&u)[K - 1],
                                                const double (&un)[K - 1], double (&c)[2 * K], P hc = P()) {
  double xq[K + 1];
  xq[0] = 1.0;
#pragma unroll
  for (int m = 1; m <= K; ++m) xq[m] = xq[m - 1] * xi;
  c[0] = wi;
#pragma unroll
  for (int n = 1; n < K; ++n) c[n] = u[n - 1] * hc.invfact(n);
  double es[K], ee[K];
#pragma unroll
  for (int n = 1; n < K; ++n) {
    es[n] = (n == K - 1) ? u[n - 1] : xq[K - 1 - n] * u[n - 1];
    ee[n] = (n == K - 1) ? un[n - 1] : xq[K - 1 - n] * un[n - 1];
  }
  const double dwx = dwi * xq[K - 1];
#pragma unroll
  for (int m = 0; m < K; ++m) {
    double acc = hc.ce(m, 0) * dwx;
#pragma unroll
    for (int n = 1; n < K; ++n) {
      acc = __builtin_fma(hc.cs(m, n), es[n], acc);
      acc = __builtin_fma(hc.ce(m, n), ee[n], acc);
    }
    c[K + m] = acc * xq[m + 1];
  }
}

// p(s) = q(s - t0): the reference evaluates the start rows of segment 0 at local
// time t[0] (calculatingTrajectories.py:59,65-73), so that piece is a Hermite
// segment of length T_0 - t0 in the shifted variable (identity for t[0] == 0).
template <int NC>
__device__ __forceinline__ void taylor_shift(double (&c)[NC], double h) {
#pragma unroll
  for (int j = 0; j < NC - 1; ++j)
#pragma unroll
    for (int q = NC - 2; q >= j; --q) c[q] = __builtin_fma(h, c[q + 1], c[q]);
}

// Full-line output stores.  A lane owns the NC coefficients of one (drone, axis):
// stored directly, a wave instruction would scatter 64 x 16 B over 64 different
// 64-byte segments.  Instead the segment's 64 x NC doubles take a round trip
// through an LDS image [NC/2 rows][68 slots of 16 B] (row pitch 68 keeps
// ds_read_b128 conflict-free for NC = 8) and leave as 16-B-per-lane stores that
// are contiguous over each drone's 4*NC*8-byte block (256 B = two full lines).
// LDS is in-order within a wave; the wavefront-scope fences only pin the
// compiler's ordering (no vmcnt wait: output stores stay in flight).  (kTrPitch = 68: msnap_solve_plan.h)
#define MSNAP_SEG_BASE(coef, tile, M, i, NC) ((coef) + ((size_t)(tile) * kDronesPerWave * (M) + (i)) * (4 * (NC)))
#define MSNAP_SEG_STRIDE(M, NC) ((size_t)(M) * 4 * (NC))
template <int NC>
__device__ __forceinline__ void store_segment_coalesced(double2 *sTr, double *__restrict__ seg_base,
                                                        size_t drone_stride, int nvalid, int lane,
                                                        double (&c)[NC], bool bad) {
  constexpr int NJ = NC / 2;
  // a failed drone is rare: one wave-uniform test instead of 2 * NC selects per segment
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0)) {
    asm volatile("" ::: "memory");   // keep the block a branch: the compiler would flatten it into selects again
#pragma unroll
    for (int m = 0; m < NC; ++m) c[m] = bad ? __builtin_nan("") : c[m];
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) sTr[j * kTrPitch + lane] = make_double2(c[2 * j], c[2 * j + 1]);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int s = q * kWave + lane;          // flat 16-byte slot of the tile-segment
    const int drone = s / (4 * NJ);
    const int within = s - drone * (4 * NJ);
    const int a2 = within / NJ;
    const int j2 = within - a2 * NJ;
    const double2 v = sTr[j2 * kTrPitch + drone * 4 + a2];
    // The lanes past the batch end replay the tile's last valid drone (same inputs, same instruction
    // stream, bitwise the same coefficients), so their slots are stored ON TOP of that drone's instead
    // of being masked off: no exec-mask region and branch pair per store.
    const int dst = drone < nvalid ? drone : nvalid - 1;
    *reinterpret_cast<double2 *>(seg_base + (size_t)dst * drone_stride + within * 2) = v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
}

// Order-7 variant of the same idea without LDS: the 4 axis lanes of a drone hold a
// 4 x 4 grid of 16-byte pieces (lane = axis, piece = coefficient pair) of the drone's
// 256-byte block.  Two butterfly stages of quad-local exchanges transpose the grid, after
// which store q of lane a carries (axis q, pair a): the quad writes 64 contiguous bytes per
// instruction (whole 64-byte segments), with no LDS round trip and no wait on the critical
// path.  A stage exchanges (A, B) pairs between lanes that differ in one bit of the axis:
// lanes with the bit keep B and take the partner's B as their A, lanes without keep A and
// take the partner's A as their B.  Written as select-with-DPP-source, one instruction per
// dword and side:   B' = bit ? B : dpp(A)      (v_cndmask_b32_dpp, vcc = bit)
//                   A' = !bit ? A : dpp(B)     (v_cndmask_b32_dpp, vcc = !bit)
// -- 32 vector instructions per segment; select / v_mov_dpp / select, as the compiler emits
// the same exchange from C++, takes 64 (a quarter of the order-7 backward sweep).
// The leading s_nop covers the 2 wait states a DPP read needs after a VALU write.
#define MSNAP_QCND(d, s0, s1, QP) \
  "v_cndmask_b32_dpp %" #d ", %" #s0 ", %" #s1 ", vcc quad_perm:" QP " row_mask:0xf bank_mask:0xf\n\t"
#define MSNAP_QSTAGE(QP, out, src, keep, mask)                                                                     \
  asm("s_nop 1\n\ts_mov_b64 vcc, %16\n\t" MSNAP_QCND(0, 8, 17, QP) MSNAP_QCND(1, 9, 18, QP) MSNAP_QCND(2, 10, 19, QP) \
          MSNAP_QCND(3, 11, 20, QP) MSNAP_QCND(4, 12, 21, QP) MSNAP_QCND(5, 13, 22, QP) MSNAP_QCND(6, 14, 23, QP)      \
              MSNAP_QCND(7, 15, 24, QP)                                                                            \
      : "=&v"(out[0]), "=&v"(out[1]), "=&v"(out[2]), "=&v"(out[3]), "=&v"(out[4]), "=&v"(out[5]), "=&v"(out[6]),    \
        "=&v"(out[7])                                                                                              \
      : "v"(src[0]), "v"(src[1]), "v"(src[2]), "v"(src[3]), "v"(src[4]), "v"(src[5]), "v"(src[6]), "v"(src[7]),     \
        "s"(mask), "v"(keep[0]), "v"(keep[1]), "v"(keep[2]), "v"(keep[3]), "v"(keep[4]), "v"(keep[5]), "v"(keep[6]), \
        "v"(keep[7])                                                                                               \
      : "vcc")
// a, b: 4 doubles each as dwords (lo, hi); `bit` as a lane mask
template <int STAGE>   // 1: partner = lane ^ 1, 2: partner = lane ^ 2
__device__ __forceinline__ void quad_stage(uint32_t (&a)[8], uint32_t (&b)[8], unsigned long long bit) {
  uint32_t na[8], nb[8];
  const unsigned long long nbit = ~bit;
  if constexpr (STAGE == 1) {
    MSNAP_QSTAGE("[1,0,3,2]", nb, a, b, bit);
    MSNAP_QSTAGE("[1,0,3,2]", na, b, a, nbit);
  } else {
    MSNAP_QSTAGE("[2,3,0,1]", nb, a, b, bit);
    MSNAP_QSTAGE("[2,3,0,1]", na, b, a, nbit);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = na[k];
    b[k] = nb[k];
  }
}
#undef MSNAP_QSTAGE
#undef MSNAP_QCND

// `blk` is this lane's drone-segment block (4 axes x 8 coefficients); all 64 lanes must be active
// (the exchanges are quad-local and read their partners through DPP).
__device__ __forceinline__ void store_quad8_at(double *__restrict__ blk, int a, const double (&c)[8], bool bad) {
  double p[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = c[k];
  // a failed drone is rare: one wave-uniform test instead of 16 selects per segment
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0)) {
    asm volatile("" ::: "memory");   // keep the block a branch: the compiler would flatten it into selects again
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = bad ? __builtin_nan("") : p[k];
  }
  auto lo = [](double v) { return (uint32_t)__double2loint(v); };
  auto hi = [](double v) { return (uint32_t)__double2hiint(v); };
  // pieces P0..P3 = coefficient pairs (0,1) (2,3) (4,5) (6,7).  Stage 1 pairs (P0,P1) and (P2,P3):
  uint32_t A[8] = {lo(p[0]), hi(p[0]), lo(p[1]), hi(p[1]), lo(p[4]), hi(p[4]), lo(p[5]), hi(p[5])};   // P0 | P2
  uint32_t B[8] = {lo(p[2]), hi(p[2]), lo(p[3]), hi(p[3]), lo(p[6]), hi(p[6]), lo(p[7]), hi(p[7])};   // P1 | P3
  quad_stage<1>(A, B, __builtin_amdgcn_ballot_w64((a & 1) != 0));
  // stage 2 pairs (P0,P2) and (P1,P3)
  uint32_t A2[8] = {A[0], A[1], A[2], A[3], B[0], B[1], B[2], B[3]};   // P0 | P1
  uint32_t B2[8] = {A[4], A[5], A[6], A[7], B[4], B[5], B[6], B[7]};   // P2 | P3
  quad_stage<2>(A2, B2, __builtin_amdgcn_ballot_w64((a & 2) != 0));
  // now piece q = coefficient pair `a` of axis q
  uint4 *o = reinterpret_cast<uint4 *>(blk + a * 2);
  o[0] = make_uint4(A2[0], A2[1], A2[2], A2[3]);
  o[4] = make_uint4(A2[4], A2[5], A2[6], A2[7]);
  o[8] = make_uint4(B2[0], B2[1], B2[2], B2[3]);
  o[12] = make_uint4(B2[4], B2[5], B2[6], B2[7]);
}

// The quads past the batch end replay the tile's last valid drone (same inputs, same instruction
// stream, bitwise the same coefficients): they store on top of that drone's block instead of being
// masked off.
__device__ __forceinline__ void store_segment_quad8(double *__restrict__ seg_base, size_t drone_stride,
                                                    int nvalid, int lane, const double (&c)[8], bool bad) {
  const int dl = lane >> 2;
  store_quad8_at(seg_base + (size_t)(dl < nvalid ? dl : nvalid - 1) * drone_stride, lane & 3, c, bad);
}

// dur[d][i] = t[d][i+1] - t[d][i] for the whole tile, one contiguous sweep
// (`lane` runs over STRIDE threads: a wave, or the whole workgroup of a multi-wave instance)
template <int MAXCNT = 0, int STRIDE = kWave>   // MAXCNT: compile-time bound of drones x segments per tile (0: not known, scalar loop)
__device__ __forceinline__ void store_durations(const double *sTraw, int shared_times, int tpitch, int M,
                                                int nvalid, int lane, double *__restrict__ dur_tile) {
  // The loop whose lane-by-lane form `for (e = lane; e < cnt; e += 64)` faulted (uniform_for, msnap_wave.h, has the
  // account): the same wave-uniform scalar loop around a predicated body, written out here because the helper's
  // inlining order moves instructions in ten solve kernels and the headline kernels are held instruction for instruction
  const int cnt = nvalid * M;
  auto one = [&](int e) {
    if (e < cnt) {
      const int dl = e / M;
      const int i = e - dl * M;
      const double *lt = sTraw + (shared_times ? 0 : dl * tpitch);
      dur_tile[e] = lt[i + 1] - lt[i];
    }
  };
  if constexpr (MAXCNT > 0) {      // straight-line instances: two or three predicated rounds, no loop at all
#pragma unroll
    for (int e0 = 0; e0 < MAXCNT; e0 += STRIDE) one(e0 + lane);
  } else {
    for (int e0 = 0; e0 < cnt; e0 += STRIDE) one(e0 + lane);
  }
}

__device__ __forceinline__ int drone_status(bool nonfinite, bool badtime, bool singular) {
  int flags = (nonfinite ? 4 : 0) | (badtime ? 2 : 0) | (singular ? 1 : 0);
  flags |= __shfl_xor(flags, 1);   // combine the 4 axis lanes of the drone
  flags |= __shfl_xor(flags, 2);
  return (flags & 4) ? MSNAP_ST_NONFINITE : (flags & 2) ? MSNAP_ST_TIMES : (flags & 1) ? MSNAP_ST_SINGULAR : MSNAP_ST_OK;
}

// one coalesced sweep of the tile's waypoints and times into LDS, all loads in flight
__device__ __forceinline__ void stage_inputs(const double *__restrict__ wp, const double *__restrict__ tt,
                                             int shared_times, int tile, int nvalid, int wpitch, int tpitch,
                                             double *sWraw, double *sTraw, int lane) {
  const double2 *wsrc = reinterpret_cast<const double2 *>(wp + (size_t)tile * kDronesPerWave * wpitch);
  double2 *wdst = reinterpret_cast<double2 *>(sWraw);
  const int wcnt = nvalid * wpitch / 2;   // wpitch is a multiple of 4
  const double *tsrc = shared_times ? tt : tt + (size_t)tile * kDronesPerWave * tpitch;
  const int tcnt = shared_times ? tpitch : nvalid * tpitch;
  constexpr int UW = 8, UT = 4;           // the first round covers n_seg <= 14
  for (int e0 = 0, f0 = 0; e0 < wcnt || f0 < tcnt; e0 += UW * kWave, f0 += UT * kWave) {
    double2 vw[UW];
    double vt[UT];
#pragma unroll
    for (int u = 0; u < UW; ++u) {
      const int e = e0 + u * kWave + lane;
      vw[u] = wsrc[e < wcnt ? e : wcnt - 1];
    }
#pragma unroll
    for (int u = 0; u < UT; ++u) {
      const int f = f0 + u * kWave + lane;
      vt[u] = tsrc[f < tcnt ? f : tcnt - 1];
    }
    // pin: keeps the compiler from sinking each load next to its guarded store
#pragma unroll
    for (int u = 0; u < UW; ++u) asm volatile("" : "+v"(vw[u].x), "+v"(vw[u].y));
#pragma unroll
    for (int u = 0; u < UT; ++u) asm volatile("" : "+v"(vt[u]));
#pragma unroll
    for (int u = 0; u < UW; ++u) {
      const int e = e0 + u * kWave + lane;
      if (e < wcnt) wdst[e] = vw[u];
    }
#pragma unroll
    for (int u = 0; u < UT; ++u) {
      const int f = f0 + u * kWave + lane;
      if (f < tcnt) sTraw[f] = vt[u];
    }
  }
}

// The same sweep split in two for software pipelining across tiles in the persistent kernel (one round of
// (MAXM + 2) / 2 16-byte and (MAXM + 4) / 4 8-byte loads per lane): the loads of tile k+1 are issued near the end of
// tile k and land in LDS at the top of k+1.  Left to the compiler, hipcc waits for a
// prefetched load with vmcnt(0) once the wait sits behind the loop back-edge, which also
// drains the tile's 40 KB of output stores at every tile boundary.  The loads are therefore
// issued from inline asm (invisible to the compiler's wait-count pass) and retired with an
// exact s_waitcnt vmcnt(N), N = the store instructions issued after them, so the previous
// tile's stores stay in flight while the next tile starts.  (cdna_hip_programming.md 5.7:
// loads inside asm are counted and waited for by hand; the wait carries the registers as
// "+v" operands so no consumer can be scheduled above it.)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int MAXM>
struct StageRegsAsm {
  static constexpr int UW = (MAXM + 2) / 2;
  static constexpr int UT = (MAXM + 4) / 4;
  u32x4 vw[UW];
  double vt[UT];
};

template <int MAXM>
__device__ __forceinline__ void stage_load_asm(const double *__restrict__ wp, const double *__restrict__ tt,
                                               int shared_times, int tile, int nvalid, int wpitch, int tpitch,
                                               int lane, StageRegsAsm<MAXM> &r) {
  const double2 *wsrc = reinterpret_cast<const double2 *>(wp + (size_t)tile * kDronesPerWave * wpitch);
  const int wcnt = nvalid * wpitch / 2;
  const double *tsrc = shared_times ? tt : tt + (size_t)tile * kDronesPerWave * tpitch;
  const int tcnt = shared_times ? tpitch : nvalid * tpitch;
#pragma unroll
  for (int u = 0; u < StageRegsAsm<MAXM>::UW; ++u) {
    const int e = u * kWave + lane;
    const double2 *p = wsrc + (e < wcnt ? e : wcnt - 1);
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r.vw[u]) : "v"(p) : "memory");
  }
#pragma unroll
  for (int u = 0; u < StageRegsAsm<MAXM>::UT; ++u) {
    const int f = u * kWave + lane;
    const double *p = tsrc + (f < tcnt ? f : tcnt - 1);
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(r.vt[u]) : "v"(p) : "memory");
  }
}

// retire the prefetch: all but the YOUNGER most recent vector-memory operations are complete
template <int MAXM, int YOUNGER>
__device__ __forceinline__ void stage_wait_asm(StageRegsAsm<MAXM> &r) {
  wait_vmcnt<YOUNGER>();
  // tie the registers to this point so that no use is scheduled above the wait
#pragma unroll
  for (int u = 0; u < StageRegsAsm<MAXM>::UW; ++u) asm volatile("" : "+v"(r.vw[u]));
#pragma unroll
  for (int u = 0; u < StageRegsAsm<MAXM>::UT; ++u) asm volatile("" : "+v"(r.vt[u]));
}

template <int MAXM>
__device__ __forceinline__ void stage_store_asm(int shared_times, int nvalid, int wpitch, int tpitch,
                                                double *sWraw, double *sTraw, int lane, StageRegsAsm<MAXM> &r) {
  u32x4 *wdst = reinterpret_cast<u32x4 *>(sWraw);
  const int wcnt = nvalid * wpitch / 2;
  const int tcnt = shared_times ? tpitch : nvalid * tpitch;
#pragma unroll
  for (int u = 0; u < StageRegsAsm<MAXM>::UW; ++u) {
    const int e = u * kWave + lane;
    if (e < wcnt) wdst[e] = r.vw[u];
  }
#pragma unroll
  for (int u = 0; u < StageRegsAsm<MAXM>::UT; ++u) {
    const int f = u * kWave + lane;
    if (f < tcnt) sTraw[f] = r.vt[u];
  }
}

// one-wave workgroups: LDS is in-order within the wave, only the compiler must be held back
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// quad-local broadcast (DPP): the 4 axis lanes of a drone exchange values without LDS
template <int SRC>
__device__ __forceinline__ double quad_bcast(double v) {   // lane SRC of the quad to all four
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, SRC * 0x55, 0xf, 0xf, true);
  hi = __builtin_amdgcn_mov_dpp(hi, SRC * 0x55, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

}  // namespace msnap
