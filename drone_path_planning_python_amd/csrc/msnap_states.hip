// K13 -- replanning in flight (include/msnap.h, "boundary-state solve"): the minimum-snap solve whose
// end derivatives are data instead of zero (msnap_solve_states), and the evaluator that reads a path's full state --
// position and derivatives 1 .. K-1 per axis -- at one time per drone (msnap_eval_state).
//
// Solve.  In the Hermite form of DESIGN.md §3 the derivative vectors u_0, u_M of the end knots are not unknowns; given
// as data they only move to the right-hand side of the block tridiagonal system
//     O_{i-1}^T u_{i-1} + D_i u_i + O_i u_{i+1} = r_i ,   i = 1..M-1 .
// states_solve_kernel<K> carves StatesLayout<K>, stages the inputs and the two state blocks in LDS, and solves its tile
// with rolled_solve_tile<K, false, true> of msnap_rolled.h -- the body it shares with the generic solve_kernel<K, false>
// of msnap_solve.hip.  ENDS = true turns on, in that body:
//   start      u_0 / u_M are read from the state blocks (a missing one is rest) and checked for finiteness;
//   segment 0  x = 1 / T_0, and the first time must be 0 (MSNAP_ST_TIMES otherwise): the reference's start-row quirk --
//              segment 0's start rows taken at local time t[0] -- has no meaning for a path that starts from a moving
//              state, so there is no Taylor shift here;
//   knot 1     the sweep's carried term starts as Otz = O_0^T u_0 (y_1 = -yb_1 - Otz), not 0;
//   forward    the durations before the current segment are summed as msnap_eval_flat sums them;
//   knot M-1   the sweep stores G_{M-1} = S^-1 O_{M-1} for every knot, the last one included, and the backward sweep
//              starts from un = u_M:  u_{M-1} = z_{M-1} - G_{M-1} u_M, which is S^-1 (y_{M-1} - O_{M-1} u_M).  With two
//              segments the one knot receives both terms;
//   recovery   segment M-1 ends in u_M, segment 0 starts from u_0; one segment is recover_segment alone.  The last
//              segment then takes one refinement step on its end conditions (refine_end), so that msnap_eval_state at
//              the sum of the durations returns the given end state to the evaluator's own rounding.
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
  double2 *sTr = reinterpret_cast<double2 *>(lds);
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

  rolled_solve_tile<K, false, true>(p, sTr, wp, tt, shared_times, has_start, has_end, M, tile, nvalid, lane, coef,
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

template <int K>
int launch_states_k(msnap_ctx *ctx, int N, int M, const double *wp, const double *t, int shared, const double *start,
                    const double *end, double *coef, double *dur, int32_t *status) {
  const size_t lds_bytes = StatesLayout<K>::bytes(M);
  // (beyond 64 KiB of dynamic LDS a kernel has to be told; an attribute of the function, no stream operation)
  if (lds_bytes > 64 * 1024)
    MSNAP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&states_solve_kernel<K>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes));
  const int ntiles = (N + kDronesPerWave - 1) / kDronesPerWave;
  hipLaunchKernelGGL((states_solve_kernel<K>), dim3(ntiles), dim3(kWave), lds_bytes, ctx->stream, wp, t, shared, start,
                     end, N, M, coef, dur, status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_solve_states(msnap_ctx *ctx, int N, int M, const double *wp, const double *t, int shared,
                        const double *start, const double *end, double *coef, double *dur, int32_t *status) {
  return ctx->khalf == 4 ? launch_states_k<4>(ctx, N, M, wp, t, shared, start, end, coef, dur, status)
                         : launch_states_k<5>(ctx, N, M, wp, t, shared, start, end, coef, dur, status);
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

int states_max_segments(int khalf) {
  return khalf == 4 ? StatesLayout<4>::max_segments() : StatesLayout<5>::max_segments();
}

// the boundary-state solve's own segment range on top of the context's
int solve_states_args(const msnap_ctx *ctx, int n_drones, int n_seg, std::initializer_list<const void *> ptrs) {
  if (!ctx || n_drones < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (n_seg > states_max_segments(ctx->khalf)) return MSNAP_ESEGMENTS;
  if (n_drones == 0) return kNoWork;
  return all_required(ptrs);
}

size_t state_bytes(const msnap_ctx *ctx, int n_drones) { return (size_t)n_drones * 4 * (ctx->khalf - 1) * 8; }

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

int msnap_solve_states_max_segments(int order) {
  if (order != 7 && order != 9) return MSNAP_EORDER;
  return states_max_segments((order + 1) / 2);
}

int msnap_solve_states_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                              int shared_times, const double *start, const double *end, double *coef, double *dur,
                              int32_t *status) {
  MSNAP_ENTER(ctx, solve_states_args(ctx, n_drones, n_seg, {wp, t, coef, dur, status}));
  return launch_solve_states(ctx, n_drones, n_seg, wp, t, shared_times != 0, start, end, coef, dur, status);
}

int msnap_solve_states(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                       const double *start, const double *end, double *coef, double *dur, int32_t *status) {
  MSNAP_ENTER(ctx, solve_states_args(ctx, n_drones, n_seg, {wp, t, coef, dur, status}));
  const size_t b_t = (size_t)(shared_times ? 1 : n_drones) * (n_seg + 1) * 8;
  const size_t b_s = state_bytes(ctx, n_drones);
  // (a region without a source is not copied: a NULL state stays NULL for the launcher)
  return staged(ctx, {upload(wp, (size_t)n_drones * (n_seg + 1) * 4 * 8), upload(t, b_t), upload(start, start ? b_s : 0),
                      upload(end, end ? b_s : 0), download(coef, coef_bytes(ctx, n_drones, n_seg)),
                      download(dur, dur_bytes(n_drones, n_seg)), download(status, (size_t)n_drones * 4)},
                [&](const DevPtr *d) {
                  return launch_solve_states(ctx, n_drones, n_seg, d[0], d[1], shared_times != 0,
                                             start ? (const double *)d[2] : nullptr,
                                             end ? (const double *)d[3] : nullptr, d[4], d[5], d[6]);
                });
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
