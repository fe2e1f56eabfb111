// K21 -- prescribed derivatives at interior waypoints (include/msnap.h, "gates"): the boundary-state
// solve of msnap_states.hip whose interior knots may carry given velocity, acceleration, jerk (and snap at order 9).
//
// In the Hermite form of DESIGN.md §3 a prescribed component of u_i = (v, a, j[, s]) at knot i is no unknown: its
// stationarity condition leaves the system and its column moves to the right-hand side.  In the block LDL^T sweep that
// is a local edit of the knot's Schur complement (Sweep<K>::chain_masked, msnap_sweep.h); the matrix stays SPD, block
// tridiagonal and shared by a drone's four axes, so lane = 4 drone + axis and the rolled body of msnap_rolled.h carry
// over.  gates_solve_kernel<K> is states_solve_kernel<K> with GATES on in that body: same LDS layout (StatesLayout<K>),
// same input stage, same end states and refine_end; the knot's mask and the lane's K-1 values come from global memory
// one knot ahead of the sweep (no LDS of their own, so the segment range is msnap_solve_states').  A knot that no
// drone of the tile gates takes the plain step behind one wave-uniform test: the same bits, without the selects.
#include "msnap_api_util.h"
#include "msnap_rolled.h"

namespace msnap {
namespace {

// the gates take no LDS: the cap is the boundary-state solve's
static_assert(StatesLayout<4>::max_segments() >= 20 && StatesLayout<5>::max_segments() >= 20,
              "msnap_solve_gates promises at least 20 segments at both orders");

template <int K>
__global__ void __launch_bounds__(kWave)
gates_solve_kernel(const double *__restrict__ wp, const double *__restrict__ tt, int shared_times,
                   const double *__restrict__ start, const double *__restrict__ end, const int32_t *__restrict__ fix,
                   const double *__restrict__ via, int N, int M, double *__restrict__ coef, double *__restrict__ dur,
                   int32_t *__restrict__ status) {
  // (the mapping and the input stage are states_solve_kernel's, written out again: shared through a function of
  // msnap_rolled.h, the boundary-state kernels came out with other instructions than they have today)
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

  rolled_solve_tile<K, false, true, true>(p, sTr, wp, tt, shared_times, has_start, has_end, M, tile, nvalid, lane, coef,
                                          dur, status, RolledGates{fix, via});
}

template <int K>
int launch_gates_k(msnap_ctx *ctx, int N, int M, const double *wp, const double *t, int shared, const double *start,
                   const double *end, const int32_t *fix, const double *via, double *coef, double *dur,
                   int32_t *status) {
  const size_t lds_bytes = StatesLayout<K>::bytes(M);
  // (beyond 64 KiB of dynamic LDS a kernel has to be told; an attribute of the function, no stream operation)
  if (lds_bytes > 64 * 1024)
    MSNAP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&gates_solve_kernel<K>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes));
  const int ntiles = (N + kDronesPerWave - 1) / kDronesPerWave;
  hipLaunchKernelGGL((gates_solve_kernel<K>), dim3(ntiles), dim3(kWave), lds_bytes, ctx->stream, wp, t, shared, start,
                     end, fix, via, N, M, coef, dur, status);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

int launch_solve_gates(msnap_ctx *ctx, int N, int M, const double *wp, const double *t, int shared,
                       const double *start, const double *end, const int32_t *fix, const double *via, double *coef,
                       double *dur, int32_t *status) {
  return ctx->khalf == 4 ? launch_gates_k<4>(ctx, N, M, wp, t, shared, start, end, fix, via, coef, dur, status)
                         : launch_gates_k<5>(ctx, N, M, wp, t, shared, start, end, fix, via, coef, dur, status);
}

int gates_max_segments(int khalf) {
  return khalf == 4 ? StatesLayout<4>::max_segments() : StatesLayout<5>::max_segments();
}

// msnap_solve_states' checks, and a mask needs its values
int solve_gates_args(const msnap_ctx *ctx, int n_drones, int n_seg, const void *fix, const void *via,
                     std::initializer_list<const void *> ptrs) {
  if (!ctx || n_drones < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (n_seg > gates_max_segments(ctx->khalf)) return MSNAP_ESEGMENTS;
  if (n_drones == 0) return kNoWork;
  if (int rc = all_required(ptrs)) return rc;
  if (fix && !via) return MSNAP_EINVAL;
  return MSNAP_OK;
}

}  // namespace
}  // namespace msnap

using namespace msnap;

extern "C" {

int msnap_solve_gates_max_segments(int order) {
  if (order != 7 && order != 9) return MSNAP_EORDER;
  return gates_max_segments((order + 1) / 2);
}

int msnap_solve_gates_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                             int shared_times, const double *start, const double *end, const int32_t *fix,
                             const double *via, double *coef, double *dur, int32_t *status) {
  MSNAP_ENTER(ctx, solve_gates_args(ctx, n_drones, n_seg, fix, via, {wp, t, coef, dur, status}));
  return launch_solve_gates(ctx, n_drones, n_seg, wp, t, shared_times != 0, start, end, fix, fix ? via : nullptr, coef,
                            dur, status);
}

int msnap_solve_gates(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                      const double *start, const double *end, const int32_t *fix, const double *via, double *coef,
                      double *dur, int32_t *status) {
  MSNAP_ENTER(ctx, solve_gates_args(ctx, n_drones, n_seg, fix, via, {wp, t, coef, dur, status}));
  const size_t b_t = (size_t)(shared_times ? 1 : n_drones) * (n_seg + 1) * 8;
  const size_t b_s = (size_t)n_drones * 4 * (ctx->khalf - 1) * 8;
  const size_t n_knots = (size_t)n_drones * (n_seg - 1);
  // (a region without a source is not copied: a NULL state or mask stays NULL for the launcher)
  return staged(ctx, {upload(wp, (size_t)n_drones * (n_seg + 1) * 4 * 8), upload(t, b_t), upload(start, start ? b_s : 0),
                      upload(end, end ? b_s : 0), upload(fix, fix ? n_knots * 4 : 0),
                      upload(via, fix ? n_knots * 4 * (ctx->khalf - 1) * 8 : 0),
                      download(coef, coef_bytes(ctx, n_drones, n_seg)), download(dur, dur_bytes(n_drones, n_seg)),
                      download(status, (size_t)n_drones * 4)},
                [&](const DevPtr *d) {
                  return launch_solve_gates(ctx, n_drones, n_seg, d[0], d[1], shared_times != 0,
                                            start ? (const double *)d[2] : nullptr,
                                            end ? (const double *)d[3] : nullptr,
                                            fix ? (const int32_t *)d[4] : nullptr,
                                            fix ? (const double *)d[5] : nullptr, d[6], d[7], d[8]);
                });
}

}  // extern "C"
