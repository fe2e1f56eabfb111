// K8 -- segment-time optimisation per drone, one launch for the whole iteration (include/msnap.h, "time allocation";
// DESIGN.md §5 K8).
//
// Per drone: minimise J(T) = sum_a w_a J_a over the segment durations with sum T_i and the waypoints fixed,
// T_i >= T_min.  dJ/dT_i = -sum_a w_a E_i,a with E the conserved Ostrogradsky energy of segment i (envelope theorem:
// no adjoint sweep), so one block-LDL^T solve gives cost and gradient.  Method: projected gradient descent with Armijo
// backtracking; the iterate is the knot times, a trial is "knots -> durations as the solve entries take them -> solve".
//
// Mapping as K1: lane = 4 * drone + axis, a wavefront carries one tile of 16 drones (8 when the 16-drone stash does
// not fit LDS; lanes 32..63 then replay the tile's last drone as the lanes past a batch end always do).  The
// solve of a trial is the solve entries' own text: chain_solve of msnap_rolled.h, the call rolled_solve_tile makes, here
// at a run-time tile size (closed loops: ring_solve).  Everything a drone carries between
// trials lives in LDS, drone-interleaved ([index][drone]): current and trial knots, the gradient at both, the descent
// direction, 1/T, G_i, z_i.  The four axis lanes of a drone write the same bits to the same address, so nothing one
// lane reads was written by another and no fence is needed after the input stage.
//
// Control flow.  Drones need different numbers of trials.  The trial loop runs while any lane of the wave has a trial
// to make (__ballot), every lane runs its body, and what a finished drone would change is held back by selects -- no
// loop the lanes leave one by one.  Cost and gradient are combined over the quad with quad_bcast in
// the fixed order ((x + y) + z) + yaw, so the four lanes hold the same bits and take the same decisions.
//
// Given end states (msnap_optimize_times_states): timeopt_kernel<K, kTimeoptEnds>.  The end knots' derivative vectors are data
// as in the boundary-state solve (chain_solve's ENDS); the gradient is the same expression -- the first and last
// segment's outer end states are fixed either way.  What differs from the rest-to-rest instance is one `if constexpr`
// each: the state images in LDS, their finiteness check, the end vectors handed to chain_solve, and its REFINE
// (refine_end on the last segment) when the coefficients leave -- so coef is msnap_solve_states' at t_out, bit for bit.
//
// Closed loops (msnap_optimize_times_periodic): timeopt_kernel<K, kTimeoptRing>.  "The solve for T" is
// msnap_solve_periodic's, so the trial is K15's ring elimination, ring_solve of msnap_ring.h -- the call K15's own
// kernel makes, here at a run-time tile size -- over a stash that is the one below plus H and, for the coefficients
// that leave, the correction's z'.  The envelope gradient holds on the ring
// (the seam state is a stationary unknown like every interior knot), so input stage, floor, direction, step rules and
// results are the lines below unchanged; the mode is one `if constexpr` around the trial's body.
//
// A free total duration (msnap_optimize_times_free): timeopt_kernel<K, kTimeoptFree>, the end-state
// mode with F(T) = J(T) + k_T sum_i T_i in place of J and a time weight k_T per drone.  The envelope statement never
// asked for a fixed sum, so dF/dT_i = k_T - sum_a w_a E_i,a comes out of the same solve and the projection goes: the
// direction is -g off the floor, one pass.  What differs from kTimeoptEnds is one `if constexpr` each: the weight's
// check, a raise of short durations nobody pays for, cost and gradient with the time term, the direction, a last knot
// that moves, and the current total in the stopping measure.
//
// Gates (msnap_optimize_times_gates): timeopt_kernel<K, kTimeoptGates>, the end-state mode whose
// interior knots may carry prescribed derivatives.  A gated component of u_i is data instead of a stationary unknown,
// which the envelope argument does not look at (as it does not look at the end states), so the gradient is the same
// expression.  What differs from kTimeoptEnds is one `if constexpr`: the trial hands its lane's ChainGates to
// chain_solve's GATES, which fetches masks and values from global memory one knot ahead as K21 does (no LDS of their
// own: the segment caps are the end-state mode's), and the first trial's `invalid` joins the input checks.  GATES is
// written beside FREE, not against it: a free total through gates is a matter of one more instance.
//
// One kernel text, four translation units: msnap_timeopt.hip instantiates the rest-to-rest and end-state modes and
// holds every mode's entry points and launch_optimize_times, the one launch function they call;
// msnap_timeopt_periodic.hip instantiates the ring mode, msnap_timeopt_free.hip the free-total mode and
// msnap_timeopt_gates.hip the gates mode, each behind one launch function of its own -- objects of their own, so that
// what is held of msnap_timeopt.o (its instructions, its kernel count, no register-pressure copy) stays true.
// Everything here has internal linkage.
#pragma once

#include <math.h>

#include <initializer_list>
#include <type_traits>

#include "msnap_internal.h"
#include "msnap_ring.h"
#include "msnap_rolled.h"
#include "msnap_sweep.h"

namespace msnap {
namespace {

constexpr double kArmijo = 1e-4;       // accept when J_new <= J - kArmijo * a * |P g|^2
constexpr int kMaxHalvings = 30;       // rejected trials in a row after which the line search gives up
constexpr double kBoundRel = 1e-9;     // a segment within T_min (1 + kBoundRel) is at its bound

struct TimeoptArgs {
  const double *wp, *tt;
  int shared_times, N, M, TD;
  double w[4];
  double min_fraction, tol;
  int max_iter;
  double *t_out, *coef, *dur;
  int32_t *status;
  double *cost, *pg;
  int32_t *iters;
};
// ENDS: the tile's end states, [n_drones][4][K-1] each (msnap_solve_states's layout); a null block is rest
struct TimeoptEndsArgs : TimeoptArgs {
  const double *start, *end;
};
// FREE: the price of a second per drone, [n_drones]
struct TimeoptFreeArgs : TimeoptEndsArgs {
  const double *time_weight;
};
// GATES: the masks [n_drones][M-1] and values [n_drones][M-1][4][K-1] (msnap_solve_gates' layout); fix null: no gates
struct TimeoptGatesArgs : TimeoptEndsArgs {
  const int32_t *fix;
  const double *via;
};

// w_0 v_0 + .. + w_3 v_3 over the quad, the same bits in its four lanes; an axis of weight 0 is not looked at
__device__ __forceinline__ double quad_weighted_sum(double v, double wa) {
  const double p = wa == 0.0 ? 0.0 : wa * v;
  return ((quad_bcast<0>(p) + quad_bcast<1>(p)) + quad_bcast<2>(p)) + quad_bcast<3>(p);
}

template <int MODE>
using TimeoptArgsOf = std::conditional_t<
    MODE == kTimeoptGates, TimeoptGatesArgs,
    std::conditional_t<MODE == kTimeoptFree, TimeoptFreeArgs,
                       std::conditional_t<MODE == kTimeoptEnds, TimeoptEndsArgs, TimeoptArgs>>>;

// ENDS: the end knots' derivative vectors u_0, u_M are data (msnap_optimize_times_states); the trial is chain_solve
// RING: the last waypoint is joined to the first (msnap_optimize_times_periodic), the trial is ring_solve
// FREE: ENDS with the total duration an unknown (msnap_optimize_times_free): F = J + k_T t[M], no projection
// GATES: ENDS with prescribed derivatives at interior knots (msnap_optimize_times_gates): chain_solve's GATES
template <int K, int MODE>
__global__ void __launch_bounds__(kWave)
timeopt_kernel(const TimeoptArgsOf<MODE> p) {
  constexpr bool FREE = MODE == kTimeoptFree, GATES = MODE == kTimeoptGates;
  constexpr bool ENDS = MODE == kTimeoptEnds || FREE || GATES, RING = MODE == kTimeoptRing;
  constexpr int NU = K - 1, NC = 2 * K, PITCH = NU | 1;

  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int lane = threadIdx.x;
  const int dl = lane >> 2;
  const int a = lane & 3;
  const int M = p.M, TD = p.TD, QL = 4 * p.TD;
  const int knots = M - 1;
  const int wpitch = (M + 1) * 4;
  const int tpitch = M + 1;
  const int tile = blockIdx.x;
  const int left = p.N - tile * TD;
  const int nvalid = left < TD ? left : TD;
  // lanes past the tile's drones replay its last one (and store on top of its results)
  const bool live = dl < nvalid;
  const int dloc = live ? dl : nvalid - 1;
  const int ql = dloc * 4 + a;
  const size_t d = (size_t)tile * TD + dloc;

  // LDS: Tr (order 9 only: output transpose image) | Wraw[TD][(M+1)*4] | Traw[TD][M+1] (inputs, then the final knots)
  //      | Tc, Tt [M+1][TD] | Gc, Gt, D, X [M][TD] | G[knots][NU*NU][TD] | Z[knots][NU][4 TD]
  //      | ENDS: S0, S1 [4 TD][PITCH] (start and end state of every lane, at K13's odd pitch)
  //      | RING: H[knots][NU*NU][TD] | Z2[knots][NU][4 TD] (the seam coupling; z' of the leaving solve's refinement)
  double2 *sTr = reinterpret_cast<double2 *>(lds);
  double *sWraw = lds + (NC == 8 ? 0 : (NC / 2) * kTrPitch * 2);
  double *sTraw = sWraw + TD * wpitch;
  double *sTc = sTraw + TD * tpitch + dloc;          // (this drone's column)
  double *sTt = sTc + TD * tpitch;                   // (this drone's column)
  double *sGc = sTraw + 3 * TD * tpitch;
  double *sGt = sGc + TD * M;
  double *sD = sGt + TD * M;
  double *sX = sD + TD * M;
  double *sG = sX + TD * M;
  double *sZ = sG + (size_t)TD * NU * NU * knots + ql;   // (this lane's column)
  double *sS = sG + (size_t)TD * (NU * NU + 4 * NU) * knots;   // (ENDS only; RING: H, then Z2)
  const double *sS0 = sS + ql * PITCH;                         // (this lane's rows)
  const double *sS1 = sS0 + QL * PITCH;

  // ENDS: the state blocks travel with the input stage, every load in flight before the first LDS store; a missing
  // block is staged as zeros, so nothing below asks which were given
  double v0[NU], v1[NU];
  if constexpr (ENDS) {
#pragma unroll
    for (int q = 0; q < NU; ++q) v0[q] = v1[q] = 0.0;
    if (p.start) load_states<NU, PITCH>(p.start + (size_t)tile * QL * NU, 0, nvalid, lane, v0);
    if (p.end) load_states<NU, PITCH>(p.end + (size_t)tile * QL * NU, 0, nvalid, lane, v1);
  }
  stage_inputs(p.wp + (size_t)tile * TD * wpitch, p.shared_times ? p.tt : p.tt + (size_t)tile * TD * tpitch,
               p.shared_times, 0, nvalid, wpitch, tpitch, sWraw, sTraw, lane);
  if constexpr (ENDS) {
    store_states<NU, PITCH>(sS, nvalid, lane, v0);
    store_states<NU, PITCH>(sS + QL * PITCH, nvalid, lane, v1);
  }
  __syncthreads();
  const double *lw = sWraw + dloc * wpitch + a;
  const double *lt = sTraw + (p.shared_times ? 0 : dloc * tpitch);
  const double wa = a == 0 ? p.w[0] : a == 1 ? p.w[1] : a == 2 ? p.w[2] : p.w[3];

  // ---------------- input checks, the floor, the start point ----------------
  const double t0 = lt[0];
  const double ttotal = lt[M];
  bool nonfinite = !finite64(t0) | !finite64(lw[0]);
  bool badtime = t0 != 0.0;
  for (int i = 0; i < M; ++i) {
    nonfinite |= !finite64(lt[i + 1]) | !finite64(lw[(i + 1) * 4]);
    badtime |= !(lt[i + 1] - lt[i] > 0.0);
  }
  if constexpr (ENDS) {      // data, and checked like every other input
#pragma unroll
    for (int q = 0; q < NU; ++q) nonfinite |= !finite64(sS0[q]) | !finite64(sS1[q]);
  }
  // FREE: the drone's time weight is data too; one that is not a positive number has no minimum to go to
  double kT = 0.0;
  if constexpr (FREE) {
    kT = p.time_weight[d];
    nonfinite |= !(finite64(kT) & (kT > 0.0));
  }
  const double Tmin = p.min_fraction * ttotal / (double)M;
  // durations below the floor are raised to it; the others keep T_min plus their excess over it scaled by one factor
  // that pays for the raise: the sum is kept, nothing falls below the floor, and a feasible input is not touched
  double excess = 0.0, slack = 0.0;
  bool anybelow = false;
  for (int i = 0; i < M; ++i) {
    const double T = lt[i + 1] - lt[i];
    const bool below = T < Tmin;
    anybelow |= below;
    excess += below ? Tmin - T : 0.0;
    slack += below ? 0.0 : T - Tmin;
  }
  const double keep = slack > 0.0 ? fmax(1.0 - excess / slack, 0.0) : 0.0;
  {
    double t = 0.0;
    sTc[0] = t0;
    for (int i = 0; i < M; ++i) {
      const double T = lt[i + 1] - lt[i];
      // FREE: nothing pays for the raise -- every other duration is the input's and the sum grows
      const double Tn = T < Tmin ? Tmin : FREE ? T : fma(T - Tmin, keep, Tmin);
      const double tn = !FREE && i == M - 1 ? ttotal : t + Tn;
      sTc[(i + 1) * TD] = anybelow ? tn : lt[i + 1];
      sD[i * TD + dloc] = 0.0;
      t = tn;
    }
  }

  // GATES: this lane's masks and values, in global memory as the caller gave them (the replayed drone's for lanes past
  // the tile's end); gatefault: a trial met a mask out of range or a non-finite value under a set bit
  [[maybe_unused]] const int32_t *frow = nullptr;
  [[maybe_unused]] const double *grow = nullptr;
  [[maybe_unused]] bool gatefault = false;
  if constexpr (GATES) {
    if (p.fix != nullptr && M >= 2) {
      frow = p.fix + d * (size_t)knots;
      grow = p.via + (d * (size_t)knots * 4 + a) * NU;
    }
  }

  // ---------------- one trial: solve for the knots sT, cost, gradient (EMIT: the coefficients leave) ----------------
  auto trial = [&](auto emit, const double *sT, double *sGrad, bool bad, double &Jw, bool &singular) {
    constexpr bool EMIT = decltype(emit)::value;
    // per segment, last first: cost and gradient of a trial, or the stores of the coefficients that leave.  Those take
    // the solve entries' refinement (K15's step on the ring, refine_end on the last segment); cost and gradient are
    // every trial's, the unrefined ones
    double Ja = 0.0;
    auto seg = [&](int i, double (&c)[NC], double Ti) {
      if constexpr (EMIT) {
        double *base = p.coef + ((size_t)tile * TD * M + i) * (4 * NC);
        if constexpr (NC == 8) store_segment_quad8(base, MSNAP_SEG_STRIDE(M, NC), nvalid, lane, c, bad);
        else store_segment_coalesced<NC>(sTr, base, MSNAP_SEG_STRIDE(M, NC), nvalid, lane, c, bad);
      } else {
        Ja += segment_cost<K>(c, Ti);
        const double gi = -quad_weighted_sum(ostrogradsky_energy<K>(c), wa);
        sGrad[i * TD + dloc] = FREE ? kT + gi : gi;      // (FREE: dF/dT_i = k_T - sum_a w_a E_i,a)
      }
    };
    if constexpr (RING) {
      // K15's elimination around the ring
      double *sZ2 = sS + (size_t)TD * NU * NU * knots + ql;
      const RingLane rl = {lw, sT, sX + dloc, sG + dloc, sS + dloc, sZ, sZ2, TD};
      ring_solve<K, EMIT>(rl, M, singular, seg);
    } else {
      // the open chain of the solve entries (the input stage has checked t[0] == 0, so rest to rest may take the
      // start-row form as it is: T_0 - 0 and the shift that is skipped are the same bits)
      double u0[NU], uM[NU];
#pragma unroll
      for (int q = 0; q < NU; ++q) {
        if constexpr (ENDS) u0[q] = sS0[q], uM[q] = sS1[q];
        else u0[q] = uM[q] = 0.0;
      }
      const ChainLane cl = {lw, sT, sX + dloc, sG + dloc, sZ, TD};
      if constexpr (GATES) {
        ChainGates cg = {frow, grow, false};
        chain_solve<K, true, EMIT, 0, true>(cl, M, u0, uM, singular, seg, ChainUnchecked{}, &cg);
        gatefault |= cg.invalid;
      } else {
        chain_solve<K, ENDS, ENDS && EMIT>(cl, M, u0, uM, singular, seg);
      }
    }
    Jw = quad_weighted_sum(Ja, wa);
    if constexpr (FREE) Jw = Jw + kT * sT[M * TD];      // F = J + k_T sum_i T_i
  };

  // ---------------- the iteration ----------------
  // Descent direction -P g at the current point (Tc, Gc) into D: the mean of g is removed over the free segments; a
  // segment at its bound whose direction points below it leaves the free set, until none does (bitmask: n_seg <= 128).
  // A pure function of (Tc, Gc): run again on an unchanged point it gives the same bits.
  struct Direction {
    double n2, dmax, Tsmall, cap;   // |P g|^2, max |d_i|, min T_i, the step that takes the first T_i to the floor
  };
  auto direction = [&]() -> Direction {
    if constexpr (FREE) {
      // no sum to keep, so no mean to remove and no free set to iterate: d = -g but on segments at their bound whose
      // gradient points below it
      Direction r = {0.0, 0.0, ttotal, __builtin_inf()};
      for (int i = 0; i < M; ++i) {
        const double gi = sGc[i * TD + dloc];
        const double T = sTc[(i + 1) * TD] - sTc[i * TD];
        const bool fixed = (T - Tmin <= kBoundRel * Tmin) & (gi > 0.0);
        const double di = fixed ? 0.0 : -gi;
        sD[i * TD + dloc] = di;
        r.n2 = fma(di, di, r.n2);
        r.dmax = fmax(r.dmax, fabs(di));
        r.Tsmall = fmin(r.Tsmall, T);
        const double reach = (T - Tmin) / (di < 0.0 ? -di : 1.0);
        r.cap = fmin(r.cap, di < 0.0 ? reach : __builtin_inf());
      }
      return r;
    }
    unsigned long long fix0 = 0, fix1 = 0;
    double mean = 0.0;
    bool changed = true;
    while (__ballot(changed) != 0) {
      double sum = 0.0;
      int cnt = 0;
      for (int i = 0; i < M; ++i) {
        const bool fixed = (((i < 64 ? fix0 : fix1) >> (i & 63)) & 1ull) != 0;
        sum += fixed ? 0.0 : sGc[i * TD + dloc];
        cnt += fixed ? 0 : 1;
      }
      const double m = sum / (double)(cnt > 0 ? cnt : 1);
      mean = cnt > 0 ? m : 0.0;
      changed = false;
      for (int i = 0; i < M; ++i) {
        const bool fixed = (((i < 64 ? fix0 : fix1) >> (i & 63)) & 1ull) != 0;
        const double T = sTc[(i + 1) * TD] - sTc[i * TD];
        const bool leaves = !fixed & (T - Tmin <= kBoundRel * Tmin) & (mean - sGc[i * TD + dloc] < 0.0);
        const unsigned long long bit = leaves ? 1ull << (i & 63) : 0ull;
        fix0 |= i < 64 ? bit : 0ull;
        fix1 |= i < 64 ? 0ull : bit;
        changed |= leaves;
      }
    }
    Direction r = {0.0, 0.0, ttotal, __builtin_inf()};
    for (int i = 0; i < M; ++i) {
      const bool fixed = (((i < 64 ? fix0 : fix1) >> (i & 63)) & 1ull) != 0;
      const double di = fixed ? 0.0 : mean - sGc[i * TD + dloc];
      const double T = sTc[(i + 1) * TD] - sTc[i * TD];
      sD[i * TD + dloc] = di;
      r.n2 = fma(di, di, r.n2);
      r.dmax = fmax(r.dmax, fabs(di));
      r.Tsmall = fmin(r.Tsmall, T);
      const double reach = (T - Tmin) / (di < 0.0 ? -di : 1.0);
      r.cap = fmin(r.cap, di < 0.0 ? reach : __builtin_inf());
    }
    return r;
  };
  // a trial counts when no pivot failed and its cost is finite: one answer for the four lanes
  auto usable = [&](bool singular, double Jn) {
    int f = (!singular & finite64(Jn)) ? 0 : 1;
    f |= __shfl_xor(f, 1);
    f |= __shfl_xor(f, 2);
    return f == 0;
  };
  const double sqrtM = sqrt((double)M);
  auto measure = [&](double n2, double Jc) {
    const double v = sqrt(n2) * (FREE ? sTc[M * TD] : ttotal) / (sqrtM * Jc);      // (FREE: the current total)
    return Jc > 0.0 ? v : 0.0;      // (a path that costs nothing is optimal)
  };

  // the start point
  double J;
  bool sing0;
  trial(std::false_type{}, sTc, sGc, false, J, sing0);
  if constexpr (GATES) nonfinite |= gatefault;      // (the gates are data, seen whole by this first solve)
  const int st_in = drone_status(nonfinite, badtime, false);
  const int st = st_in ? st_in : (usable(sing0, J) ? MSNAP_ST_OK : MSNAP_ST_SINGULAR);
  const double J0 = J;
  Direction dr = direction();
  double pgm = measure(dr.n2, J);
  // first proposal: a quarter of the smallest segment for the largest component; the step is the proposal, capped
  double prop = 0.25 * dr.Tsmall / dr.dmax;
  double step = fmin(prop, dr.cap);
  int iters = 0, nback = 0;
  bool run = (st == MSNAP_ST_OK) & (pgm > p.tol) & (p.max_iter > 0) & (dr.dmax > 0.0) & (step > 0.0);
  while (__ballot(run) != 0) {
    // trial knots: T_i + step * d_i, not below the floor, summed from 0; the last knot is the input's, bit for bit
    {
      double t = 0.0;
      sTt[0] = sTc[0];
      for (int i = 0; i < M; ++i) {
        const double Tn = fmax(fma(step, sD[i * TD + dloc], sTc[(i + 1) * TD] - sTc[i * TD]), Tmin);
        const double tn = !FREE && i == M - 1 ? ttotal : t + Tn;      // (FREE: the last knot moves with the rest)
        sTt[(i + 1) * TD] = tn;
        t = tn;
      }
    }
    double Jn;
    bool singular;
    trial(std::false_type{}, sTt, sGt, false, Jn, singular);
    const bool accept = run & usable(singular, Jn) & (Jn <= J - kArmijo * step * dr.n2);
    const bool capped = step >= dr.cap;
    J = accept ? Jn : J;
    iters += accept ? 1 : 0;
    for (int i = 0; i < M; ++i) {
      sTc[(i + 1) * TD] = accept ? sTt[(i + 1) * TD] : sTc[(i + 1) * TD];
      sGc[i * TD + dloc] = accept ? sGt[i * TD + dloc] : sGc[i * TD + dloc];
    }
    dr = direction();          // (unchanged bits where the point did not move)
    pgm = measure(dr.n2, J);
    // next proposal: twice an accepted step (the proposal again when the floor cut the step short), half a rejected one
    const double up = capped ? prop : 2.0 * step;
    const double nprop = accept ? up : 0.5 * step;
    nback = accept ? 0 : nback + 1;
    const double next = fmin(nprop, dr.cap);
    const bool done = accept ? (!(pgm > p.tol) | (iters >= p.max_iter) | !(dr.dmax > 0.0) | !(next > 0.0))
                             : (nback >= kMaxHalvings);
    step = run ? next : step;
    prop = run ? nprop : prop;
    run = run & !done;
  }

  // ---------------- results ----------------
  const bool bad = st != MSNAP_ST_OK;
  {
    double Jf;
    bool sf;
    trial(std::true_type{}, sTc, sGt, bad, Jf, sf);
  }
  // the knots in drone-major order for the coalesced sweeps (Traw: the inputs are dead)
  wave_lds_fence();
  for (int i = 0; i <= M; ++i) sTraw[dloc * tpitch + i] = bad ? __builtin_nan("") : sTc[i * TD];
  wave_lds_fence();
  store_durations(sTraw, 0, tpitch, M, nvalid, lane, p.dur + (size_t)tile * TD * M);
  {
    const int cnt = nvalid * tpitch;
    double *dst = p.t_out + (size_t)tile * TD * tpitch;
    for (int e0 = 0; e0 < cnt; e0 += kWave) {      // (uniform_for of msnap_wave.h written out, as store_durations is:
      const int e = e0 + lane;                      // the helper's inlining order moves instructions in this kernel)
      if (e < cnt) dst[e] = sTraw[e];
    }
  }
  if (live && a == 0) {
    p.status[d] = st;
    if (p.cost) {
      p.cost[2 * d] = bad ? __builtin_nan("") : J0;
      p.cost[2 * d + 1] = bad ? __builtin_nan("") : J;
    }
    if (p.pg) p.pg[d] = bad ? __builtin_nan("") : pgm;
    if (p.iters) p.iters[d] = iters;
  }
}

// doubles of LDS one tile of TD drones needs (kTimeoptEnds, kTimeoptFree, kTimeoptGates: with the two state images --
// the gates stay in global memory; kTimeoptRing: with H and Z2)
constexpr size_t timeopt_lds_words(int khalf, int M, int TD, int mode) {
  const size_t nu = (size_t)khalf - 1, knots = (size_t)M - 1, m = (size_t)M;
  const size_t tr = khalf == 4 ? 0 : (size_t)khalf * kTrPitch * 2;
  const size_t states =
      mode == kTimeoptEnds || mode == kTimeoptFree || mode == kTimeoptGates ? 2 * (size_t)TD * 4 * (nu | 1) : 0;
  const size_t ring = mode == kTimeoptRing ? (size_t)TD * (nu * nu + 4 * nu) * knots : 0;
  return tr + (size_t)TD * ((m + 1) * 4 + (m + 1) + 2 * (m + 1) + 4 * m + nu * nu * knots + 4 * nu * knots) + states +
         ring;
}
// the largest n_seg a tile of TD drones fits (the direction's bitmask ends at 128)
constexpr int timeopt_tile_segments(int khalf, int TD, int mode) {
  int m = 1;
  while (m < 128 && timeopt_lds_words(khalf, m + 1, TD, mode) * sizeof(double) <= kMaxLdsBytes) ++m;
  return m;
}
// closed loops: a tile is 848 M - 560 (order 7) or 1200 M - 232 (order 9) doubles at 16 drones, 424 M - 280 or
// 600 M + 224 at 8; 160 KiB are 20480 doubles
static_assert(timeopt_tile_segments(4, 16, kTimeoptRing) == 24 && timeopt_tile_segments(5, 16, kTimeoptRing) == 17 &&
                  timeopt_tile_segments(4, 8, kTimeoptRing) == 48 && timeopt_tile_segments(5, 8, kTimeoptRing) == 33,
              "DESIGN.md K16 and include/msnap.h quote these");
// gates: no LDS of their own, so the end-state mode's caps
static_assert(timeopt_tile_segments(4, 16, kTimeoptGates) == 39 && timeopt_tile_segments(5, 16, kTimeoptGates) == 28 &&
                  timeopt_tile_segments(4, 8, kTimeoptGates) == 79 && timeopt_tile_segments(5, 8, kTimeoptGates) == 57 &&
                  timeopt_tile_segments(4, 8, kTimeoptGates) == timeopt_tile_segments(4, 8, kTimeoptEnds) &&
                  timeopt_tile_segments(5, 8, kTimeoptGates) == timeopt_tile_segments(5, 8, kTimeoptEnds),
              "DESIGN.md K22 and include/msnap.h quote these");

// One mode's launch of a call whose pointers are the device's (TimeoptCall, msnap_internal.h): the tile size, the
// kernels' dynamic-LDS limit (raised to the full 160 KiB once per context and mode: a function attribute is a property
// of the device's module), the arguments.
template <int MODE>
int timeopt_launch(msnap_ctx *ctx, const TimeoptCall &c) {
  if (c.n_drones == 0) return MSNAP_OK;
  // 16 drones per wave while their stash fits LDS, 8 above
  const int TD =
      timeopt_lds_words(ctx->khalf, c.n_seg, kDronesPerWave, MODE) * sizeof(double) <= kMaxLdsBytes ? kDronesPerWave : 8;
  const size_t lds_bytes = timeopt_lds_words(ctx->khalf, c.n_seg, TD, MODE) * sizeof(double);
  if (lds_bytes > kMaxLdsBytes) return MSNAP_ESEGMENTS;
  if (!(ctx->timeopt_ready & (1 << MODE))) {
    for (const void *k : {reinterpret_cast<const void *>(&timeopt_kernel<4, MODE>),
                          reinterpret_cast<const void *>(&timeopt_kernel<5, MODE>)})
      MSNAP_HIP(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes));
    ctx->timeopt_ready |= 1 << MODE;
  }
  TimeoptArgsOf<MODE> a;
  a.wp = c.wp;
  a.tt = c.t;
  a.shared_times = c.shared_times ? 1 : 0;
  a.N = c.n_drones;
  a.M = c.n_seg;
  a.TD = TD;
  for (int q = 0; q < 4; ++q) a.w[q] = c.weights[q];
  a.min_fraction = c.min_fraction;
  a.tol = c.tol;
  a.max_iter = c.max_iter;
  a.t_out = c.t_out;
  a.coef = c.coef;
  a.dur = c.dur;
  a.status = c.status;
  a.cost = c.cost;
  a.pg = c.pg;
  a.iters = c.iters;
  if constexpr (MODE == kTimeoptEnds || MODE == kTimeoptFree || MODE == kTimeoptGates) {
    a.start = c.start;
    a.end = c.end;
  }
  if constexpr (MODE == kTimeoptGates) {
    a.fix = c.fix;
    a.via = c.via;
  }
  if constexpr (MODE == kTimeoptFree) a.time_weight = c.time_weight;
  const int ntiles = (c.n_drones + TD - 1) / TD;
  if (ctx->khalf == 4)
    hipLaunchKernelGGL((timeopt_kernel<4, MODE>), dim3(ntiles), dim3(kWave), lds_bytes, ctx->stream, a);
  else
    hipLaunchKernelGGL((timeopt_kernel<5, MODE>), dim3(ntiles), dim3(kWave), lds_bytes, ctx->stream, a);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

}  // namespace
}  // namespace msnap
