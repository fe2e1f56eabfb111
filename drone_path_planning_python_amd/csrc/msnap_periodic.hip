// K15 -- closed-loop paths (include/msnap.h, "periodic solve"): the minimum-snap solve whose last
// waypoint is joined to its first, msnap_solve_periodic.  The derivative vector of the seam, u_0 = u_M, is one more
// unknown, and the seam one more knot whose left segment is M-1 and whose right segment is 0, so the Hermite-form
// system of DESIGN.md §3 becomes block CYCLIC tridiagonal:
//     O_{i-1}^T u_{i-1} + D_i u_i + O_i u_{i+1} = y_i ,   i = 0..M-1,  indices mod M .
// periodic_solve_kernel<K> keeps the mapping of states_solve_kernel<K> (lane = 4 drone + axis, one wave per 16-drone
// tile, inputs staged in LDS, Sweep<K>'s geometry and LDL^T, recover_segment, refine_end, the full-line stores) and
// eliminates around the ring in four passes:
//   forward   knots 1..M-1 as the open chain does (S_i = D_i - O_{i-1}^T G_{i-1}, G_i = S_i^-1 O_i,
//             z_i = S_i^-1 (y_i - O_{i-1}^T z_{i-1})), with one more matrix per knot for the coupling to the seam:
//             H_1 = S_1^-1 O_0^T,  H_i = -S_i^-1 O_{i-1}^T H_{i-1},  so that  u_i = z_i - G_i u_{i+1} - H_i u_0.
//             H depends on the times only, like G: the four lanes of a quad compute it redundantly and stash it at
//             G's pitch.
//   backward  p_{M-1} = z_{M-1}, Q_{M-1} = G_{M-1} + H_{M-1} (u_M is u_0);  p_i = z_i - G_i p_{i+1},
//             Q_i = H_i - G_i Q_{i+1}, written over z and H:  u_i = p_i - Q_i u_0.
//   seam      (D_0 - O_{M-1}^T Q_{M-1} - O_0 Q_1) u_0 = y_0 - O_{M-1}^T p_{M-1} - O_0 p_1 : one more symmetric positive
//             definite block through ldl_factor / ldl_solve, its pivots tested like the others.
//   refine    one step of iterative refinement of all u_i: the residual of the ring's rows, r_i = y_i - O_{i-1}^T u_{i-1}
//             - D_i u_i - O_i u_{i+1}, accumulated with error-free products and sums (dd_submul), then the same
//             elimination for the correction: z'_i = S_i^-1 (r_i - O_{i-1}^T z'_{i-1}) with S_i factored again from the
//             stashed G, p'_i = z'_i - G_i p'_{i+1}, and the seam block's kept factor for du_0.  The ring has one more
//             unknown block than the open chain and, with few segments, a worse condition: at order 9 with two segments
//             the unrefined solve is 4 x further from the exact solution than msnap_solve_states given the exact seam
//             state; the step brings every segment count to that solve's level (DESIGN.md K15 has the figures).
//   recovery  u_i = (p_i - Q_i u_0) + (p'_i - Q_i du_0), recover_segment, and on the last segment refine_end with the
//             solved seam state as its end vector, so that msnap_eval_state at the sum of the durations returns what it
//             returns at 0.
// With two segments both couplings land on the one knot (Q_1 = G_1 + H_1) and the loops above run as written.
#include "msnap_api_util.h"
#include "msnap_ring.h"
#include "msnap_rolled.h"

namespace msnap {
namespace {

// LDS of one 16-drone tile, in doubles:
//   Tr[NC/2][68][2] (order 9 only: the output transpose image) | Wraw[16][(M+1) 4] | Traw[16][M+1] |
//   X[M][16] | G[M-1][NU NU][16] | H[M-1][NU NU][16] | Z[M-1][NU][64] | Z2[M-1][NU][64] (the correction's z', p')
// = 768 M - 592 at order 7, 1120 M - 264 at order 9; 160 KiB are 20480 doubles: 27 and 18 segments.
template <int K>
struct PeriodicLayout {
  static constexpr int NU = K - 1, NC = 2 * K;
  static constexpr size_t kTrWords = NC == 8 ? 0 : (size_t)(NC / 2) * kTrPitch * 2;
  static constexpr size_t words(int M) {
    return kTrWords + (size_t)16 * (M + 1) * 5 + (size_t)16 * M + (size_t)(M - 1) * (2 * 16 * NU * NU + 2 * 64 * NU);
  }
  static constexpr size_t bytes(int M) { return words(M) * sizeof(double); }
  static constexpr int max_segments() {
    int M = 2;
    while (bytes(M + 1) <= kMaxLdsBytes) ++M;
    return M;
  }
};
static_assert(PeriodicLayout<4>::bytes(2) <= kMaxLdsBytes && PeriodicLayout<5>::bytes(2) <= kMaxLdsBytes, "");
static_assert(PeriodicLayout<4>::max_segments() == 27 && PeriodicLayout<5>::max_segments() == 18,
              "DESIGN.md K15 and include/msnap.h quote these");

// (dd_submul, the error-free multiply-subtract of the refinement pass: msnap_ring.h)
template <int K>
__global__ void __launch_bounds__(kWave)
periodic_solve_kernel(const double *__restrict__ wp, const double *__restrict__ tt, int shared_times, int N, int M,
                      double *__restrict__ coef, double *__restrict__ dur, int32_t *__restrict__ status) {
  using L = PeriodicLayout<K>;
  using SW = Sweep<K>;
  using C = HermiteConsts<K>;
  constexpr int NU = SW::NU, NC = SW::NC, KK = SW::KK, PM = SW::PM, NS = SW::NS;

  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int lane = threadIdx.x;
  const int knots = M - 1;
  const int wpitch = (M + 1) * 4;
  const int tpitch = M + 1;
  const int tile = blockIdx.x;

  double2 *sTr = reinterpret_cast<double2 *>(lds);
  double *sWraw = lds + L::kTrWords;
  double *sTraw = sWraw + 16 * wpitch;
  double *sX = sTraw + 16 * tpitch;
  double *sG = sX + 16 * M;
  double *sH = sG + 16 * NU * NU * knots;
  double *sZ = sH + 16 * NU * NU * knots;
  double *sZ2 = sZ + 64 * NU * knots;

  const int left = N - tile * kDronesPerWave;
  const int nvalid = left < kDronesPerWave ? left : kDronesPerWave;

  stage_inputs(wp, tt, shared_times, tile, nvalid, wpitch, tpitch, sWraw, sTraw, lane);
  __syncthreads();
  store_durations(sTraw, shared_times, tpitch, M, nvalid, lane, dur + (size_t)tile * kDronesPerWave * M);

  const int dl = lane >> 2;
  const int a = lane & 3;
  // lanes past the end of the batch replay the last valid drone (and store on top of its results)
  const bool live = dl < nvalid;
  const int dloc = live ? dl : nvalid - 1;
  const double *lw = sWraw + dloc * wpitch + a;
  const double *lt = sTraw + (shared_times ? 0 : dloc * tpitch);
  auto Wv = [&](int i) -> double { return lw[i * 4]; };
  auto Tv = [&](int i) -> double { return lt[i]; };
  auto gslot = [&](double *base, int i) -> double * { return base + (size_t)(i - 1) * (NU * NU * 16) + dl; };   // knot i
  auto zslot = [&](int i) -> double * { return sZ + (size_t)(i - 1) * (NU * 64) + lane; };
  auto z2slot = [&](int i) -> double * { return sZ2 + (size_t)(i - 1) * (NU * 64) + lane; };

  // ---------------- segment 0 ----------------
  const double t0 = Tv(0);
  double tcur = Tv(1);
  const double w0 = Wv(0);
  double wcur = Wv(1);
  bool nonfinite = !(finite64(t0) & finite64(tcur) & finite64(w0) & finite64(wcur));
  double T = tcur - t0;
  bool badtime = !(T > 0.0) | (t0 != 0.0);
  double x = rcp64(T);
  const double x0 = x, dw0 = wcur - w0;
  sX[0 * 16 + dl] = x;
  SW sw;
  sw.init(x, dw0);
  // the carried right-hand side of H: O_0^T at knot 1, then -O_{i-1}^T H_{i-1}
  double Cy[NU][NU];
  {
    double xp[PM + 1];
    SW::powers(x, xp);
#pragma unroll
    for (int r = 0; r < NU; ++r)
#pragma unroll
      for (int c = 0; c < NU; ++c) Cy[r][c] = C::HSE[c + 1][r + 1] * xp[KK - (c + 1) - (r + 1)];
  }

  // ---------------- forward sweep over knots 1 .. M-1 ----------------
  double tacc = 0.0;      // the durations before the current segment, summed as msnap_eval_flat sums them
  for (int i = 1; i < M; ++i) {
    const double tnext = Tv(i + 1);
    const double wnext = Wv(i + 1);
    tacc = tacc + T;
    nonfinite |= !finite64(tnext) | !finite64(wnext);
    T = tnext - tcur;
    badtime |= !(T > 0.0);
    x = rcp64(T);
    sX[i * 16 + dl] = x;

    typename SW::Knot k;
    SW::knot_geom(x, wnext - wcur, sw.E, sw.re, k);
    double S[NS], y[NU], dinv[NU];
#pragma unroll
    for (int n = 0; n < NU; ++n) {
#pragma unroll
      for (int m = 0; m <= n; ++m) S[sidx(n, m)] = k.D[sidx(n, m)] - sw.OtG[sidx(n, m)];
      y[n] = -k.yb[n] - sw.Otz[n];
    }
    sw.singular |= SW::ldl_factor(S, dinv);

    double *g = gslot(sG, i), *h = gslot(sH, i), *zz = zslot(i);
    // G_i = S^-1 O_i column by column, and the Schur term O_i^T G_i (symmetric) for knot i+1
    double G[NU][NU];
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      double v[NU];
#pragma unroll
      for (int r = 0; r < NU; ++r) v[r] = k.O[r][c];
      SW::ldl_solve(S, dinv, v);
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        G[r][c] = v[r];
        g[(r * NU + c) * 16] = v[r];
      }
    }
    // z_i = S^-1 y_i
    SW::ldl_solve(S, dinv, y);
#pragma unroll
    for (int r = 0; r < NU; ++r) zz[r * 64] = y[r];
    // H_i = S^-1 Cy column by column; each column's carry -O_i^T H_i[:, c] replaces it
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      double v[NU];
#pragma unroll
      for (int r = 0; r < NU; ++r) v[r] = Cy[r][c];
      SW::ldl_solve(S, dinv, v);
#pragma unroll
      for (int r = 0; r < NU; ++r) h[(r * NU + c) * 16] = v[r];
#pragma unroll
      for (int n = 0; n < NU; ++n) {
        double w = 0.0;
#pragma unroll
        for (int q = 0; q < NU; ++q) w = __builtin_fma(-k.O[q][n], v[q], w);
        Cy[n][c] = w;
      }
    }
#pragma unroll
    for (int n = 0; n < NU; ++n) {
#pragma unroll
      for (int m = 0; m <= n; ++m) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < NU; ++q) v = __builtin_fma(k.O[q][n], G[q][m], v);
        sw.OtG[sidx(n, m)] = v;
      }
      double w = 0.0;
#pragma unroll
      for (int q = 0; q < NU; ++q) w = __builtin_fma(k.O[q][n], y[q], w);
      sw.Otz[n] = w;
    }
#pragma unroll
    for (int e = 0; e < NS; ++e) sw.E[e] = k.E[e];
#pragma unroll
    for (int r = 0; r < NU; ++r) sw.re[r] = k.re[r];
    tcur = tnext;
    wcur = wnext;
  }
  const double wM = wcur;
  // the local time msnap_eval_state evaluates the last segment at when asked for the sum of the durations
  const double tl_end = (tacc + T) - tacc;

  // ---------------- backward pass: u_i = p_i - Q_i u_0, p and Q over z and H ----------------
  double pn[NU], Qn[NU][NU];      // of knot i+1
  {
    const double *g = gslot(sG, M - 1), *zz = zslot(M - 1);
    double *h = gslot(sH, M - 1);
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      pn[r] = zz[r * 64];
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        Qn[r][c] = g[(r * NU + c) * 16] + h[(r * NU + c) * 16];
        h[(r * NU + c) * 16] = Qn[r][c];
      }
    }
  }
  double pL[NU], QL[NU][NU];      // of knot M-1, for the seam
#pragma unroll
  for (int r = 0; r < NU; ++r) {
    pL[r] = pn[r];
#pragma unroll
    for (int c = 0; c < NU; ++c) QL[r][c] = Qn[r][c];
  }
  for (int i = M - 2; i >= 1; --i) {
    const double *g = gslot(sG, i);
    double *h = gslot(sH, i), *zz = zslot(i);
    double gq[NU][NU], p[NU], Q[NU][NU];
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      p[r] = zz[r * 64];
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        gq[r][c] = g[(r * NU + c) * 16];
        Q[r][c] = h[(r * NU + c) * 16];
      }
    }
#pragma unroll
    for (int r = 0; r < NU; ++r) {
#pragma unroll
      for (int q = 0; q < NU; ++q) {
        p[r] = __builtin_fma(-gq[r][q], pn[q], p[r]);
#pragma unroll
        for (int c = 0; c < NU; ++c) Q[r][c] = __builtin_fma(-gq[r][q], Qn[q][c], Q[r][c]);
      }
    }
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      zz[r * 64] = p[r];
      pn[r] = p[r];
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        h[(r * NU + c) * 16] = Q[r][c];
        Qn[r][c] = Q[r][c];
      }
    }
  }
  // (pn, Qn are knot 1's now; with two segments knot 1 is knot M-1)

  // ---------------- the seam knot: left segment M-1, right segment 0 ----------------
  double u0[NU];
  typename SW::Knot k0;        // D_0 = E_{M-1} + SS_0, yb_0, O_0
  double OL[NU][NU];           // O_{M-1}
  double S0[NS], dinv0[NU];    // the seam block and its factor (kept for the correction)
  {
    SW::knot_geom(x0, dw0, sw.E, sw.re, k0);
    double xp[PM + 1];
    SW::powers(x, xp);         // x = 1 / T_{M-1}
#pragma unroll
    for (int n = 0; n < NU; ++n)
#pragma unroll
      for (int m = 0; m < NU; ++m) OL[n][m] = C::HSE[n + 1][m + 1] * xp[KK - (n + 1) - (m + 1)];
#pragma unroll
    for (int n = 0; n < NU; ++n) {
#pragma unroll
      for (int m = 0; m <= n; ++m) {
        double v = k0.D[sidx(n, m)];
#pragma unroll
        for (int q = 0; q < NU; ++q) v = __builtin_fma(-OL[q][n], QL[q][m], v);
#pragma unroll
        for (int q = 0; q < NU; ++q) v = __builtin_fma(-k0.O[n][q], Qn[q][m], v);
        S0[sidx(n, m)] = v;
      }
      double w = -k0.yb[n];
#pragma unroll
      for (int q = 0; q < NU; ++q) w = __builtin_fma(-OL[q][n], pL[q], w);
#pragma unroll
      for (int q = 0; q < NU; ++q) w = __builtin_fma(-k0.O[n][q], pn[q], w);
      u0[n] = w;
    }
    sw.singular |= SW::ldl_factor(S0, dinv0);
    SW::ldl_solve(S0, dinv0, u0);
  }

  const int st = drone_status(nonfinite, badtime, sw.singular);
  if (live && a == 0) status[tile * kDronesPerWave + dl] = st;
  const bool bad = st != 0;

  // ---------------- one refinement step: residual of the ring in extended precision, the same elimination ----------------
  // u_j of knot j from the stash (j = 0 and j = M: the seam)
  auto knot_u = [&](int j, double (&u)[NU]) {
    if (j >= 1 && j <= M - 1) {
      const double *h = gslot(sH, j), *zz = zslot(j);
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        double v = zz[r * 64];
#pragma unroll
        for (int c = 0; c < NU; ++c) v = __builtin_fma(-h[(r * NU + c) * 16], u0[c], v);
        u[r] = v;
      }
    } else {
#pragma unroll
      for (int r = 0; r < NU; ++r) u[r] = u0[r];
    }
  };
  // r = y - OP^T up - D uc - ON un, row by row
  auto residual = [&](const double (&yb)[NU], const double (&D)[NS], const double (&OP)[NU][NU],
                      const double (&ON)[NU][NU], const double (&up)[NU], const double (&uc)[NU],
                      const double (&un_)[NU], double (&r)[NU]) {
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      double s = -yb[n], e = 0.0;
#pragma unroll
      for (int q = 0; q < NU; ++q) dd_submul(s, e, OP[q][n], up[q]);
#pragma unroll
      for (int q = 0; q < NU; ++q) dd_submul(s, e, D[n >= q ? sidx(n, q) : sidx(q, n)], uc[q]);
#pragma unroll
      for (int q = 0; q < NU; ++q) dd_submul(s, e, ON[n][q], un_[q]);
      r[n] = s + e;
    }
  };
  double du0[NU];
  {
    SW s2;
    s2.init(x0, dw0);          // the end side of segment 0 again; s2.Otz carries O_{i-1}^T z'_{i-1}
    double OP[NU][NU];         // O_{i-1}
#pragma unroll
    for (int n = 0; n < NU; ++n)
#pragma unroll
      for (int m = 0; m < NU; ++m) OP[n][m] = k0.O[n][m];
    double up[NU], uc[NU], un_[NU];
    knot_u(0, up);
    knot_u(1, uc);
    double wc = Wv(1);
    for (int i = 1; i < M; ++i) {
      const double wnx = Wv(i + 1);
      const double xi = sX[i * 16 + dl];
      knot_u(i + 1, un_);
      typename SW::Knot k;
      SW::knot_geom(xi, wnx - wc, s2.E, s2.re, k);
      double S[NS], dinv[NU], r[NU];
      if (i >= 2) {            // S_i = D_i - O_{i-1}^T G_{i-1} from the stash, as the forward sweep formed it
        const double *g = gslot(sG, i - 1);
        double G[NU][NU];
#pragma unroll
        for (int rr = 0; rr < NU; ++rr)
#pragma unroll
          for (int c = 0; c < NU; ++c) G[rr][c] = g[(rr * NU + c) * 16];
#pragma unroll
        for (int n = 0; n < NU; ++n)
#pragma unroll
          for (int m = 0; m <= n; ++m) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < NU; ++q) v = __builtin_fma(OP[q][n], G[q][m], v);
            S[sidx(n, m)] = k.D[sidx(n, m)] - v;
          }
      } else {
#pragma unroll
        for (int e = 0; e < NS; ++e) S[e] = k.D[e] - 0.0;
      }
      SW::ldl_factor(S, dinv);
      residual(k.yb, k.D, OP, k.O, up, uc, un_, r);
#pragma unroll
      for (int n = 0; n < NU; ++n) r[n] = r[n] - s2.Otz[n];
      SW::ldl_solve(S, dinv, r);
      double *z2 = z2slot(i);
#pragma unroll
      for (int n = 0; n < NU; ++n) z2[n * 64] = r[n];
#pragma unroll
      for (int n = 0; n < NU; ++n) {
        double w = 0.0;
#pragma unroll
        for (int q = 0; q < NU; ++q) w = __builtin_fma(k.O[q][n], r[q], w);
        s2.Otz[n] = w;
      }
#pragma unroll
      for (int n = 0; n < NU; ++n) {
#pragma unroll
        for (int m = 0; m < NU; ++m) OP[n][m] = k.O[n][m];
        up[n] = uc[n];
        uc[n] = un_[n];
      }
#pragma unroll
      for (int e = 0; e < NS; ++e) s2.E[e] = k.E[e];
#pragma unroll
      for (int rr = 0; rr < NU; ++rr) s2.re[rr] = k.re[rr];
      wc = wnx;
    }
    // backward: p'_i = z'_i - G_i p'_{i+1} over z'
    double qn[NU], qL[NU];     // p' of knot i+1, of knot M-1
    {
      const double *z2 = z2slot(M - 1);
#pragma unroll
      for (int r = 0; r < NU; ++r) qn[r] = qL[r] = z2[r * 64];
    }
    for (int i = M - 2; i >= 1; --i) {
      const double *g = gslot(sG, i);
      double *z2 = z2slot(i);
      double q[NU];
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        double v = z2[r * 64];
#pragma unroll
        for (int c = 0; c < NU; ++c) v = __builtin_fma(-g[(r * NU + c) * 16], qn[c], v);
        q[r] = v;
      }
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        z2[r * 64] = q[r];
        qn[r] = q[r];
      }
    }
    // the seam row: left knot M-1, right knot 1 (up is u_{M-1} after the loop, uc is u_M = u_0)
    double u1[NU];
    knot_u(1, u1);
    residual(k0.yb, k0.D, OL, k0.O, up, uc, u1, du0);
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      double w = du0[n];
#pragma unroll
      for (int q = 0; q < NU; ++q) w = __builtin_fma(-OL[q][n], qL[q], w);
#pragma unroll
      for (int q = 0; q < NU; ++q) w = __builtin_fma(-k0.O[n][q], qn[q], w);
      du0[n] = w;
    }
    SW::ldl_solve(S0, dinv0, du0);
  }
  double us[NU];               // the refined seam state
#pragma unroll
  for (int r = 0; r < NU; ++r) us[r] = u0[r] + du0[r];

  // ---------------- recovery and stores, last segment first ----------------
  double un[NU];
#pragma unroll
  for (int r = 0; r < NU; ++r) un[r] = us[r];      // u_M = u_0
  double wn = wM;
  for (int i = M - 1; i >= 0; --i) {
    double u[NU];
    const double wi = Wv(i);
    const double xi = sX[i * 16 + dl];
    if (i >= 1) {
      const double *h = gslot(sH, i), *zz = zslot(i), *z2 = z2slot(i);
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        double v = zz[r * 64], dv = z2[r * 64];
#pragma unroll
        for (int c = 0; c < NU; ++c) {
          v = __builtin_fma(-h[(r * NU + c) * 16], u0[c], v);
          dv = __builtin_fma(-h[(r * NU + c) * 16], du0[c], dv);
        }
        u[r] = v + dv;
      }
    } else {
#pragma unroll
      for (int r = 0; r < NU; ++r) u[r] = us[r];
    }
    double c[NC];
    recover_segment<K>(wi, wn - wi, xi, u, un, c);
    // the last segment takes one refinement step on its end conditions, the solved seam state as its end vector
    if (i == M - 1) refine_end<K>(c, tl_end, xi, wn, un);
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

template <int K>
int launch_periodic_k(msnap_ctx *ctx, int N, int M, const double *wp, const double *t, int shared, double *coef,
                      double *dur, int32_t *status) {
  const size_t lds_bytes = PeriodicLayout<K>::bytes(M);
  // (beyond 64 KiB of dynamic LDS a kernel has to be told; an attribute of the function, no stream operation)
  if (lds_bytes > 64 * 1024)
    MSNAP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&periodic_solve_kernel<K>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes));
  const int ntiles = (N + kDronesPerWave - 1) / kDronesPerWave;
  hipLaunchKernelGGL((periodic_solve_kernel<K>), dim3(ntiles), dim3(kWave), lds_bytes, ctx->stream, wp, t, shared, N, M,
                     coef, dur, status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_solve_periodic(msnap_ctx *ctx, int N, int M, const double *wp, const double *t, int shared, double *coef,
                          double *dur, int32_t *status) {
  return ctx->khalf == 4 ? launch_periodic_k<4>(ctx, N, M, wp, t, shared, coef, dur, status)
                         : launch_periodic_k<5>(ctx, N, M, wp, t, shared, coef, dur, status);
}

int periodic_max_segments(int khalf) {
  return khalf == 4 ? PeriodicLayout<4>::max_segments() : PeriodicLayout<5>::max_segments();
}

// the periodic solve's own segment range (2 .. cap) on top of the context's
int solve_periodic_args(const msnap_ctx *ctx, int n_drones, int n_seg, std::initializer_list<const void *> ptrs) {
  if (!ctx || n_drones < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (n_seg < 2 || n_seg > periodic_max_segments(ctx->khalf)) return MSNAP_ESEGMENTS;
  if (n_drones == 0) return kNoWork;
  for (const void *p : ptrs)
    if (!p) return MSNAP_EINVAL;
  return MSNAP_OK;
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

int msnap_solve_periodic_max_segments(int order) {
  if (order != 7 && order != 9) return MSNAP_EORDER;
  return periodic_max_segments((order + 1) / 2);
}

int msnap_solve_periodic_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, double *coef, double *dur, int32_t *status) {
  MSNAP_ENTER(ctx, solve_periodic_args(ctx, n_drones, n_seg, {wp, t, coef, dur, status}));
  return launch_solve_periodic(ctx, n_drones, n_seg, wp, t, shared_times != 0, coef, dur, status);
}

int msnap_solve_periodic(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                         double *coef, double *dur, int32_t *status) {
  MSNAP_ENTER(ctx, solve_periodic_args(ctx, n_drones, n_seg, {wp, t, coef, dur, status}));
  const size_t b_t = (size_t)(shared_times ? 1 : n_drones) * (n_seg + 1) * 8;
  return staged(ctx, {upload(wp, (size_t)n_drones * (n_seg + 1) * 4 * 8), upload(t, b_t),
                      download(coef, coef_bytes(ctx, n_drones, n_seg)), download(dur, dur_bytes(n_drones, n_seg)),
                      download(status, (size_t)n_drones * 4)},
                [&](const DevPtr *d) {
                  return launch_solve_periodic(ctx, n_drones, n_seg, d[0], d[1], shared_times != 0, d[2], d[3], d[4]);
                });
}

}  // extern "C"
