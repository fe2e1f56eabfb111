// The ring elimination of closed-loop paths as one device function, ring_solve, the one text of it:
// periodic_solve_kernel<K> of msnap_periodic.hip (msnap_solve_periodic) runs it over a stash with the compile-time tile
// of 16 drones, the trial of the time allocation on closed loops, timeopt_kernel<K, kTimeoptRing>
// (msnap_timeopt_kernel.h), over one whose tile size is a run-time value.  lane = 4 drone + axis.
//
// The last waypoint is joined to the first.  The derivative vector of the seam, u_0 = u_M, is one more unknown, and the
// seam one more knot whose left segment is M-1 and whose right segment is 0, so the Hermite-form system of DESIGN.md §3
// becomes block CYCLIC tridiagonal:
//     O_{i-1}^T u_{i-1} + D_i u_i + O_i u_{i+1} = y_i ,   i = 0..M-1,  indices mod M .
// Sweep<K>'s geometry and LDL^T, recover_segment and refine_end are the open chain's (msnap_sweep.h, msnap_rolled.h);
// the elimination goes around the ring in these passes:
//   forward   knots 1..M-1 as the open chain does (S_i = D_i - O_{i-1}^T G_{i-1}, G_i = S_i^-1 O_i,
//             z_i = S_i^-1 (y_i - O_{i-1}^T z_{i-1})), with one more matrix per knot for the coupling to the seam:
//             H_1 = S_1^-1 O_0^T,  H_i = -S_i^-1 O_{i-1}^T H_{i-1},  so that  u_i = z_i - G_i u_{i+1} - H_i u_0.
//             H depends on the times only, like G: the four lanes of a quad compute it redundantly and stash it at
//             G's pitch.
//   backward  p_{M-1} = z_{M-1}, Q_{M-1} = G_{M-1} + H_{M-1} (u_M is u_0);  p_i = z_i - G_i p_{i+1},
//             Q_i = H_i - G_i Q_{i+1}, written over z and H:  u_i = p_i - Q_i u_0.
//   seam      (D_0 - O_{M-1}^T Q_{M-1} - O_0 Q_1) u_0 = y_0 - O_{M-1}^T p_{M-1} - O_0 p_1 : one more symmetric positive
//             definite block through ldl_factor / ldl_solve, its pivots tested like the others.
//   REFINE    one step of iterative refinement of all u_i: the residual of the ring's rows, r_i = y_i - O_{i-1}^T u_{i-1}
//             - D_i u_i - O_i u_{i+1}, accumulated with error-free products and sums (dd_submul), then the same
//             elimination for the correction: z'_i = S_i^-1 (r_i - O_{i-1}^T z'_{i-1}) with S_i factored again from the
//             stashed G, p'_i = z'_i - G_i p'_{i+1}, and the seam block's kept factor for du_0.  The ring has one more
//             unknown block than the open chain and, with few segments, a worse condition: at order 9 with two segments
//             the unrefined solve is 4 x further from the exact solution than msnap_solve_states given the exact seam
//             state; the step brings every segment count to that solve's level (DESIGN.md K15 has the figures).
//   recovery  u_i = (p_i - Q_i u_0) + (p'_i - Q_i du_0) (the second term with REFINE), recover_segment, last segment
//             first, each handed to `seg`; with REFINE the last segment takes refine_end with the solved seam state as
//             its end vector, so that msnap_eval_state at the sum of the durations returns what it returns at 0.
// With two segments both couplings land on the one knot (Q_1 = G_1 + H_1) and the loops run as written.
#pragma once

#include "msnap_rolled.h"

namespace msnap {

// (s + e) -= a b with the product and the sum error-free: s carries the running value, e collects what the roundings
// dropped (two-product by fma, Knuth's two-sum)
__device__ __forceinline__ void dd_submul(double &s, double &e, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  const double pe = __builtin_fma(a, b, -p);
  const double t = s - p;
  const double bb = t - s;
  const double err = (s - (t - bb)) + (-p - bb);
  s = t;
  e = e + (err - pe);
}

// One lane's view of its tile's stash, every pointer already at this lane's column.  TD is the tile size in drones:
// the template argument TILE of ring_solve when that is given (K15: 16), this struct's field otherwise (K16).
//   lw [(M+1)] at stride 4 (waypoints of this axis) | sT [M+1] (knots) at stride 1 with a compile-time tile (K15's
//   staged row, shared or per drone), at stride TD otherwise (K16's drone-interleaved iterate) |
//   sX [M] at stride TD (1/T, written here) | sG, sH [M-1][NU NU] at stride TD |
//   sZ, sZ2 [M-1][NU] at stride 4 TD (sZ2: REFINE only)
struct RingLane {
  const double *lw, *sT;
  double *sX, *sG, *sH, *sZ, *sZ2;
  int TD;
};

// seg(i, c, T_i): segment i's coefficients, i = M-1 .. 0.  `singular` is set before the first call of seg: true if a
// pivot, the seam block's included, is not positive and finite.
// see(t_{i+1}, w_{i+1}, T_i), i = 0 .. M-1: what the forward sweep reads of each segment, as it reads it, for a caller
// that checks its inputs on the way (K15; a pass of its own over the staged row in front of the sweep cost 0.3-1.2 us
// per launch, profiles/periodic_ring_ab.md) -- t_0 and w_0 are the caller's to look at.  The default sees nothing (K16
// has checked the input times once, and its iterates are its own).
// Nothing here acts on the knots' validity: through times that are not finite or not increasing the arithmetic runs on
// (rcp64 of such a duration, NaN after it), every loop is bounded by M and wave-uniform, and the caller discards the
// results.
struct RingUnchecked {
  __device__ __forceinline__ void operator()(double, double, double) const {}
};
template <int K, bool REFINE, int TILE = 0, class Seg, class See = RingUnchecked>
__device__ __forceinline__ void ring_solve(const RingLane &p, int M, bool &singular, Seg &&seg, See &&see = See{}) {
  using SW = Sweep<K>;
  using C = HermiteConsts<K>;
  constexpr int NU = SW::NU, NC = SW::NC, KK = SW::KK, PM = SW::PM, NS = SW::NS;
  const int TD = TILE ? TILE : p.TD, QL = 4 * TD;
  const int TS = TILE ? 1 : TD;      // the knots' stride
  const double *lw = p.lw, *sT = p.sT;
  double *sX = p.sX;
  auto gslot = [&](double *base, int i) -> double * { return base + (size_t)(i - 1) * (NU * NU * TD); };   // knot i
  auto zslot = [&](double *base, int i) -> double * { return base + (size_t)(i - 1) * (NU * QL); };

  // ---------------- segment 0 ----------------
  double tcur = sT[TS];
  const double w0 = lw[0];
  double wcur = lw[4];
  double T = tcur - sT[0];
  see(tcur, wcur, T);
  double x = rcp64(T);
  const double x0 = x, dw0 = wcur - w0;
  sX[0] = x;
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
    const double tnext = sT[(i + 1) * TS];
    const double wnext = lw[(i + 1) * 4];
    tacc = tacc + T;
    T = tnext - tcur;
    see(tnext, wnext, T);
    x = rcp64(T);
    sX[i * TD] = x;

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

    double *g = gslot(p.sG, i), *h = gslot(p.sH, i), *zz = zslot(p.sZ, i);
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
        g[(r * NU + c) * TD] = v[r];
      }
    }
    // z_i = S^-1 y_i
    SW::ldl_solve(S, dinv, y);
#pragma unroll
    for (int r = 0; r < NU; ++r) zz[r * QL] = y[r];
    // H_i = S^-1 Cy column by column; each column's carry -O_i^T H_i[:, c] replaces it
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      double v[NU];
#pragma unroll
      for (int r = 0; r < NU; ++r) v[r] = Cy[r][c];
      SW::ldl_solve(S, dinv, v);
#pragma unroll
      for (int r = 0; r < NU; ++r) h[(r * NU + c) * TD] = v[r];
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
  const double wM = wcur, tM = tcur;
  // the local time msnap_eval_state evaluates the last segment at when asked for the sum of the durations
  const double tl_end = (tacc + T) - tacc;

  // ---------------- backward pass: u_i = p_i - Q_i u_0, p and Q over z and H ----------------
  double pn[NU], Qn[NU][NU];      // of knot i+1
  {
    const double *g = gslot(p.sG, M - 1), *zz = zslot(p.sZ, M - 1);
    double *h = gslot(p.sH, M - 1);
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      pn[r] = zz[r * QL];
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        Qn[r][c] = g[(r * NU + c) * TD] + h[(r * NU + c) * TD];
        h[(r * NU + c) * TD] = Qn[r][c];
      }
    }
  }
  double pL[NU], QLm[NU][NU];      // of knot M-1, for the seam
#pragma unroll
  for (int r = 0; r < NU; ++r) {
    pL[r] = pn[r];
#pragma unroll
    for (int c = 0; c < NU; ++c) QLm[r][c] = Qn[r][c];
  }
  for (int i = M - 2; i >= 1; --i) {
    const double *g = gslot(p.sG, i);
    double *h = gslot(p.sH, i), *zz = zslot(p.sZ, i);
    double gq[NU][NU], pp[NU], Q[NU][NU];
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      pp[r] = zz[r * QL];
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        gq[r][c] = g[(r * NU + c) * TD];
        Q[r][c] = h[(r * NU + c) * TD];
      }
    }
#pragma unroll
    for (int r = 0; r < NU; ++r) {
#pragma unroll
      for (int q = 0; q < NU; ++q) {
        pp[r] = __builtin_fma(-gq[r][q], pn[q], pp[r]);
#pragma unroll
        for (int c = 0; c < NU; ++c) Q[r][c] = __builtin_fma(-gq[r][q], Qn[q][c], Q[r][c]);
      }
    }
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      zz[r * QL] = pp[r];
      pn[r] = pp[r];
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        h[(r * NU + c) * TD] = Q[r][c];
        Qn[r][c] = Q[r][c];
      }
    }
  }
  // (pn, Qn are knot 1's now; with two segments knot 1 is knot M-1)

  // ---------------- the seam knot: left segment M-1, right segment 0 ----------------
  double u0[NU];
  typename SW::Knot k0;        // D_0 = E_{M-1} + SS_0, yb_0, O_0
  double OL[NU][NU];           // O_{M-1}
  double S0[NS], dinv0[NU];    // the seam block and its factor (REFINE: kept for the correction)
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
        for (int q = 0; q < NU; ++q) v = __builtin_fma(-OL[q][n], QLm[q][m], v);
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
  singular = sw.singular;

  // ---------------- REFINE: residual of the ring in extended precision, the same elimination ----------------
  double du0[NU];
#pragma unroll
  for (int r = 0; r < NU; ++r) du0[r] = 0.0;
  if constexpr (REFINE) {
    // u_j of knot j from the stash (j = 0 and j = M: the seam)
    auto knot_u = [&](int j, double (&u)[NU]) {
      if (j >= 1 && j <= M - 1) {
        const double *h = gslot(p.sH, j), *zz = zslot(p.sZ, j);
#pragma unroll
        for (int r = 0; r < NU; ++r) {
          double v = zz[r * QL];
#pragma unroll
          for (int c = 0; c < NU; ++c) v = __builtin_fma(-h[(r * NU + c) * TD], u0[c], v);
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
    double wc = lw[4];
    for (int i = 1; i < M; ++i) {
      const double wnx = lw[(i + 1) * 4];
      const double xi = sX[i * TD];
      knot_u(i + 1, un_);
      typename SW::Knot k;
      SW::knot_geom(xi, wnx - wc, s2.E, s2.re, k);
      double S[NS], dinv[NU], r[NU];
      if (i >= 2) {            // S_i = D_i - O_{i-1}^T G_{i-1} from the stash, as the forward sweep formed it
        const double *g = gslot(p.sG, i - 1);
        double G[NU][NU];
#pragma unroll
        for (int rr = 0; rr < NU; ++rr)
#pragma unroll
          for (int c = 0; c < NU; ++c) G[rr][c] = g[(rr * NU + c) * TD];
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
      double *z2 = zslot(p.sZ2, i);
#pragma unroll
      for (int n = 0; n < NU; ++n) z2[n * QL] = r[n];
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
      const double *z2 = zslot(p.sZ2, M - 1);
#pragma unroll
      for (int r = 0; r < NU; ++r) qn[r] = qL[r] = z2[r * QL];
    }
    for (int i = M - 2; i >= 1; --i) {
      const double *g = gslot(p.sG, i);
      double *z2 = zslot(p.sZ2, i);
      double q[NU];
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        double v = z2[r * QL];
#pragma unroll
        for (int c = 0; c < NU; ++c) v = __builtin_fma(-g[(r * NU + c) * TD], qn[c], v);
        q[r] = v;
      }
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        z2[r * QL] = q[r];
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
  double us[NU];               // the seam state (REFINE: refined)
#pragma unroll
  for (int r = 0; r < NU; ++r) {
    if constexpr (REFINE) us[r] = u0[r] + du0[r];
    else us[r] = u0[r];
  }

  // ---------------- recovery, last segment first ----------------
  double un[NU];
#pragma unroll
  for (int r = 0; r < NU; ++r) un[r] = us[r];      // u_M = u_0
  double wn = wM, tn = tM;
  for (int i = M - 1; i >= 0; --i) {
    double u[NU];
    const double wi = lw[i * 4];
    const double ti = sT[i * TS];
    const double xi = sX[i * TD];
    const int kq = i >= 1 ? i : 1;      // (segment 0 starts from the seam state; its loads replay knot 1's)
    const double *h = gslot(p.sH, kq), *zz = zslot(p.sZ, kq);
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      double v = zz[r * QL];
#pragma unroll
      for (int c = 0; c < NU; ++c) v = __builtin_fma(-h[(r * NU + c) * TD], u0[c], v);
      if constexpr (REFINE) {
        double dv = zslot(p.sZ2, kq)[r * QL];
#pragma unroll
        for (int c = 0; c < NU; ++c) dv = __builtin_fma(-h[(r * NU + c) * TD], du0[c], dv);
        v = v + dv;
      }
      u[r] = i >= 1 ? v : us[r];
    }
    double c[NC];
    recover_segment<K>(wi, wn - wi, xi, u, un, c);
    if constexpr (REFINE) {
      // the last segment takes one refinement step on its end conditions, the solved seam state as its end vector
      if (i == M - 1) refine_end<K>(c, tl_end, xi, wn, un);
    }
    seg(i, c, tn - ti);
#pragma unroll
    for (int r = 0; r < NU; ++r) un[r] = u[r];
    wn = wi;
    tn = ti;
  }
}

}  // namespace msnap
