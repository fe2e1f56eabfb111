// K13 -- replanning in flight (include/msnap.h, "boundary-state solve"): the minimum-snap solve whose
// end derivatives are data instead of zero (msnap_solve_states), and the evaluator that reads a path's full state --
// position and derivatives 1 .. K-1 per axis -- at one time per drone (msnap_eval_state).
//
// Solve.  In the Hermite form of DESIGN.md §3 the derivative vectors u_0, u_M of the end knots are not unknowns; given
// as data they only move to the right-hand side of the block tridiagonal system
//     O_{i-1}^T u_{i-1} + D_i u_i + O_i u_{i+1} = r_i ,   i = 1..M-1 .
// states_solve_kernel<K> carves StatesLayout<K>, stages the inputs and the two state blocks in LDS, and solves its tile
// with rolled_solve_tile<K, false, true> of msnap_rolled.h -- the wrapper it shares with the generic solve_kernel<K, false>
// of msnap_solve.hip around chain_solve, the one text of the open-chain elimination.  ENDS = true there: u_0 / u_M are
// read from the state blocks (a missing one is rest) and checked; x = 1 / T_0 and the first time must be 0
// (MSNAP_ST_TIMES otherwise; no Taylor shift: the reference's start-row quirk has no meaning for a path that starts
// from a moving state); knot 1 sees u_0 through Otz = O_0^T u_0; the backward sweep starts from u_M through the last
// knot's G, u_{M-1} = z_{M-1} - G_{M-1} u_M (with two segments the one knot receives both terms); and the last segment
// takes refine_end, so that msnap_eval_state at the sum of the durations returns the given end state to the
// evaluator's own rounding.
//
// Host side.  This unit also holds what the three tile solves beside K1 share above their kernels -- this one, the
// gates (msnap_gates.hip) and the closed loop (msnap_periodic.hip): the argument check, the entry body with its staging
// block and the entry points, over one call record (SolveCall, msnap_internal.h), as msnap_timeopt.hip does for the
// allocators.  Each unit keeps its kernels and one launch_solve_* behind launch_tiles (msnap_api_util.h).
//
// Evaluator.  One thread per drone: msnap_eval_flat's piece lookup (t <= acc + T_i: a knot belongs to the earlier
// segment) and horner_derivs' arithmetic of msnap_aux.hip carried to derivative K-1, no contraction.
#include "msnap_api_util.h"
#include "msnap_rolled.h"

namespace msnap {
namespace {

// (StatesLayout<K>, the LDS of one 16-drone tile, is in msnap_rolled.h: gates_solve_kernel<K> carves the same)
template <int K>
__global__ void __launch_bounds__(kWave)
states_solve_kernel(const double *__restrict__ wp, const double *__restrict__ tt, int shared_times,
                    const double *__restrict__ start, const double *__restrict__ end, int N, int M,
                    double *__restrict__ coef, double *__restrict__ dur, int32_t *__restrict__ status) {
  using L = StatesLayout<K>;
  constexpr int NU = K - 1, PITCH = L::kPitch;

  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int lane = threadIdx.x;
  const int knots = M - 1;
  const int wpitch = (M + 1) * 4;
  const int tpitch = M + 1;
  const int tile = blockIdx.x;

  RolledTile p;
  p.sWraw = lds + L::kTrWords;
  p.sTraw = p.sWraw + 16 * wpitch;
  p.sS0 = p.sTraw + 16 * tpitch;
  p.sS1 = p.sS0 + L::kStateWords;
  p.sX = p.sS1 + L::kStateWords;
  p.sG = p.sX + 16 * M;
  p.sZ = p.sG + 16 * NU * NU * knots;

  const int left = N - tile * kDronesPerWave;
  const int nvalid = left < kDronesPerWave ? left : kDronesPerWave;

  // ---------------- inputs: one sweep, every load in flight before the first LDS store ----------------
  const bool has_start = start != nullptr, has_end = end != nullptr;   // (wave-uniform: kernel arguments)
  double v0[NU], v1[NU];
#pragma unroll
  for (int q = 0; q < NU; ++q) v0[q] = v1[q] = 0.0;
  if (has_start) load_states<NU, PITCH>(start, tile, nvalid, lane, v0);
  if (has_end) load_states<NU, PITCH>(end, tile, nvalid, lane, v1);
  stage_inputs(wp, tt, shared_times, tile, nvalid, wpitch, tpitch, p.sWraw, p.sTraw, lane);
  if (has_start) store_states<NU, PITCH>(p.sS0, nvalid, lane, v0);
  if (has_end) store_states<NU, PITCH>(p.sS1, nvalid, lane, v1);
  __syncthreads();
  store_durations(p.sTraw, shared_times, tpitch, M, nvalid, lane, dur + (size_t)tile * kDronesPerWave * M);

  rolled_solve_tile<K, false, true>(p, wp, tt, shared_times, has_start, has_end, M, tile, nvalid, lane, coef,
                                    dur, status);
}

// ------------------------------------------------------------------------------------
// state evaluator: position and derivatives 1 .. K-1 of the four axes at one time per drone
// ------------------------------------------------------------------------------------
constexpr int kEvalThreads = 256;

template <int NC>
__global__ void __launch_bounds__(kEvalThreads)
state_eval_kernel(const double *__restrict__ coef, const double *__restrict__ dur, const double *__restrict__ tq, int N,
                  int M, double *__restrict__ pos, double *__restrict__ deriv) {
#pragma clang fp contract(off)
  constexpr int ND = NC / 2 - 1;      // derivatives per axis
  const double nan = __builtin_nan("");
  uniform_for<size_t>(
      threadIdx.x, (size_t)N, (size_t)gridDim.x * blockDim.x,
      [&](size_t d) {
#pragma clang fp contract(off)
        const double t = tq[d];
        const double *dr = dur + d * M;
        double acc_t = 0.0;
        int seg = -1;
        for (int i = 0; i < M; ++i) {
          const double Ti = dr[i];
          if (seg < 0) {
            if (t <= acc_t + Ti) seg = i;
            else acc_t = acc_t + Ti;
          }
        }
        const bool inside = t >= 0.0 && seg >= 0;
        const double tl = t - acc_t;
        const double *c = coef + (d * M + (seg < 0 ? 0 : seg)) * 4 * NC;
#pragma unroll
        for (int ax = 0; ax < 4; ++ax) {
          // horner_derivs of msnap_aux.hip: each derivative array is (i + 1) * previous[i + 1]; Horner with a separate
          // multiply and add
          double dd[NC];
#pragma unroll
          for (int i = 0; i < NC; ++i) dd[i] = c[ax * NC + i];
          double p = 0.0;
#pragma unroll
          for (int i = NC - 1; i >= 0; --i) p = p * tl + dd[i];
          pos[d * 4 + ax] = inside ? p : nan;
#pragma unroll
          for (int q = 1; q <= ND; ++q) {
#pragma unroll
            for (int i = 0; i < NC - q; ++i) dd[i] = (double)(i + 1) * dd[i + 1];
            p = 0.0;
#pragma unroll
            for (int i = NC - 1 - q; i >= 0; --i) p = p * tl + dd[i];
            deriv[(d * 4 + ax) * ND + (q - 1)] = inside ? p : nan;
          }
        }
      },
      (size_t)blockIdx.x * blockDim.x);
}

int launch_eval_state(msnap_ctx *ctx, int N, int M, const double *coef, const double *dur, const double *tq,
                      double *pos, double *deriv) {
  unsigned blocks = blocks_of((size_t)N, kEvalThreads);
  if (blocks > (unsigned)ctx->n_cu * 16) blocks = (unsigned)ctx->n_cu * 16;
  if (ctx->order == 7)
    hipLaunchKernelGGL((state_eval_kernel<8>), dim3(blocks), dim3(kEvalThreads), 0, ctx->stream, coef, dur, tq, N, M,
                       pos, deriv);
  else
    hipLaunchKernelGGL((state_eval_kernel<10>), dim3(blocks), dim3(kEvalThreads), 0, ctx->stream, coef, dur, tq, N, M,
                       pos, deriv);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

size_t state_bytes(const msnap_ctx *ctx, int n_drones) { return (size_t)n_drones * 4 * (ctx->khalf - 1) * 8; }

// the cap of a mode from its LDS layout (the gates take no LDS: theirs is the boundary-state solve's)
int solve_max_segments(int khalf, int mode) {
  if (mode == kSolveRing) return periodic_max_segments(khalf);
  return khalf == 4 ? StatesLayout<4>::max_segments() : StatesLayout<5>::max_segments();
}

int launch_solve(msnap_ctx *ctx, int mode, const SolveCall &c) {
  switch (mode) {
    case kSolveRing: return launch_solve_periodic(ctx, c);
    case kSolveGates: return launch_solve_gates(ctx, c);
    default: return launch_solve_states(ctx, c);
  }
}

// The argument check every tile-solve entry and its _device twin make: the mode's own segment range on top of the
// context's, then the pointers every mode requires; a mask needs its values
int solve_args(const msnap_ctx *ctx, int mode, const SolveCall &c) {
  if (!ctx || c.n_drones < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, c.n_seg)) return rc;
  if (c.n_seg > solve_max_segments(ctx->khalf, mode)) return MSNAP_ESEGMENTS;
  if (mode == kSolveRing && c.n_seg < 2) return MSNAP_ESEGMENTS;      // (a loop has two segments at least)
  if (c.n_drones == 0) return kNoWork;
  if (int rc = all_required({c.wp, c.t, c.coef, c.dur, c.status})) return rc;
  if (c.fix && !c.via) return MSNAP_EINVAL;
  return MSNAP_OK;
}

// Every tile-solve entry: check, then launch on the caller's device pointers (on_device), or stage the caller's host
// arrays, launch on the staged copies and read back.  (Values without a mask are not read: the kernel asks for the mask.)
int solve_entry(msnap_ctx *ctx, int mode, const SolveCall &c, bool on_device) {
  MSNAP_ENTER(ctx, solve_args(ctx, mode, c));
  if (on_device) return launch_solve(ctx, mode, c);
  const size_t n = (size_t)c.n_drones, m1 = (size_t)c.n_seg + 1, b_s = state_bytes(ctx, c.n_drones);
  const size_t n_knots = c.fix ? n * (c.n_seg - 1) : 0;
  // (a region without a source is not copied: a NULL state or mask stays NULL for the launcher)
  return staged(ctx, {upload(c.wp, n * m1 * 4 * 8), upload(c.t, (c.shared_times ? 1 : n) * m1 * 8),
                      upload(c.start, c.start ? b_s : 0), upload(c.end, c.end ? b_s : 0), upload(c.fix, n_knots * 4),
                      upload(c.via, n_knots * 4 * (ctx->khalf - 1) * 8),
                      download(c.coef, coef_bytes(ctx, c.n_drones, c.n_seg)),
                      download(c.dur, dur_bytes(c.n_drones, c.n_seg)), download(c.status, n * 4)},
                [&](const DevPtr *d) {
                  SolveCall dev = c;
                  dev.wp = d[0];
                  dev.t = d[1];
                  dev.start = c.start ? (const double *)d[2] : nullptr;
                  dev.end = c.end ? (const double *)d[3] : nullptr;
                  dev.fix = c.fix ? (const int32_t *)d[4] : nullptr;
                  dev.via = c.fix ? (const double *)d[5] : nullptr;
                  dev.coef = d[6];
                  dev.dur = d[7];
                  dev.status = d[8];
                  return launch_solve(ctx, mode, dev);
                });
}

int max_segments_entry(int order, int mode) {
  if (order != 7 && order != 9) return MSNAP_EORDER;
  return solve_max_segments((order + 1) / 2, mode);
}

}  // namespace

int launch_solve_states(msnap_ctx *ctx, const SolveCall &c) {
  auto go = [&](auto kernel, size_t lds_bytes) {
    return launch_tiles(ctx, kernel, lds_bytes, c.n_drones, c.wp, c.t, c.shared_times ? 1 : 0, c.start, c.end,
                        c.n_drones, c.n_seg, c.coef, c.dur, c.status);
  };
  return ctx->khalf == 4 ? go(&states_solve_kernel<4>, StatesLayout<4>::bytes(c.n_seg))
                         : go(&states_solve_kernel<5>, StatesLayout<5>::bytes(c.n_seg));
}

}  // namespace msnap

using namespace msnap;

extern "C" {

// The tile-solve entries fill the call record in its field order (a mode without end states or gates leaves them null)
// and differ in the mode and in whose pointers they take.
int msnap_solve_states_max_segments(int order) { return max_segments_entry(order, kSolveEnds); }

int msnap_solve_states_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                              int shared_times, const double *start, const double *end, double *coef, double *dur,
                              int32_t *status) {
  const SolveCall c = {n_drones, n_seg, wp, t, shared_times, start, end, nullptr, nullptr, coef, dur, status};
  return solve_entry(ctx, kSolveEnds, c, true);
}

int msnap_solve_states(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                       const double *start, const double *end, double *coef, double *dur, int32_t *status) {
  const SolveCall c = {n_drones, n_seg, wp, t, shared_times, start, end, nullptr, nullptr, coef, dur, status};
  return solve_entry(ctx, kSolveEnds, c, false);
}

int msnap_solve_gates_max_segments(int order) { return max_segments_entry(order, kSolveGates); }

int msnap_solve_gates_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                             int shared_times, const double *start, const double *end, const int32_t *fix,
                             const double *via, double *coef, double *dur, int32_t *status) {
  const SolveCall c = {n_drones, n_seg, wp, t, shared_times, start, end, fix, via, coef, dur, status};
  return solve_entry(ctx, kSolveGates, c, true);
}

int msnap_solve_gates(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                      const double *start, const double *end, const int32_t *fix, const double *via, double *coef,
                      double *dur, int32_t *status) {
  const SolveCall c = {n_drones, n_seg, wp, t, shared_times, start, end, fix, via, coef, dur, status};
  return solve_entry(ctx, kSolveGates, c, false);
}

int msnap_solve_periodic_max_segments(int order) { return max_segments_entry(order, kSolveRing); }

int msnap_solve_periodic_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, double *coef, double *dur, int32_t *status) {
  const SolveCall c = {n_drones, n_seg, wp, t, shared_times, nullptr, nullptr, nullptr, nullptr, coef, dur, status};
  return solve_entry(ctx, kSolveRing, c, true);
}

int msnap_solve_periodic(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                         double *coef, double *dur, int32_t *status) {
  const SolveCall c = {n_drones, n_seg, wp, t, shared_times, nullptr, nullptr, nullptr, nullptr, coef, dur, status};
  return solve_entry(ctx, kSolveRing, c, false);
}

int msnap_eval_state_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                            const double *tq, double *pos, double *deriv) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {coef, dur, tq, pos, deriv}));
  return launch_eval_state(ctx, n_drones, n_seg, coef, dur, tq, pos, deriv);
}

int msnap_eval_state(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, const double *tq,
                     double *pos, double *deriv) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {coef, dur, tq, pos, deriv}));
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(tq, (size_t)n_drones * 8), download(pos, (size_t)n_drones * 4 * 8),
                      download(deriv, state_bytes(ctx, n_drones))},
                [&](const DevPtr *d) { return launch_eval_state(ctx, n_drones, n_seg, d[0], d[1], d[2], d[3], d[4]); });
}

}  // extern "C"
