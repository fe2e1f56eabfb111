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
// (The entry points and their argument check are msnap_states.hip's, shared by the three tile solves.)
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

  rolled_solve_tile<K, false, true, true>(p, wp, tt, shared_times, has_start, has_end, M, tile, nvalid, lane, coef,
                                          dur, status, RolledGates{fix, via});
}

}  // namespace

int launch_solve_gates(msnap_ctx *ctx, const SolveCall &c) {
  auto go = [&](auto kernel, size_t lds_bytes) {
    return launch_tiles(ctx, kernel, lds_bytes, c.n_drones, c.wp, c.t, c.shared_times ? 1 : 0, c.start, c.end, c.fix,
                        c.via, c.n_drones, c.n_seg, c.coef, c.dur, c.status);
  };
  return ctx->khalf == 4 ? go(&gates_solve_kernel<4>, StatesLayout<4>::bytes(c.n_seg))
                         : go(&gates_solve_kernel<5>, StatesLayout<5>::bytes(c.n_seg));
}

}  // namespace msnap
