// K15 -- closed-loop paths (include/msnap.h, "periodic solve"): the minimum-snap solve whose last
// waypoint is joined to its first, msnap_solve_periodic.  The system is block cyclic tridiagonal; its elimination
// around the ring, with one refinement step, is ring_solve of msnap_ring.h, which has the derivation and is the text
// the time allocation on loops runs as its trial (K16).  periodic_solve_kernel<K> keeps the mapping of
// states_solve_kernel<K> (lane = 4 drone + axis, one wave per 16-drone tile, inputs staged in LDS, the full-line stores)
// and is what stands around that call: stage the inputs, store the durations, check the inputs, hand ring_solve the
// tile's stash at the compile-time tile size, store each segment as it comes back, write the status.
// (The entry points and their argument check are msnap_states.hip's, shared by the three tile solves.)
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

template <int K>
__global__ void __launch_bounds__(kWave)
periodic_solve_kernel(const double *__restrict__ wp, const double *__restrict__ tt, int shared_times, int N, int M,
                      double *__restrict__ coef, double *__restrict__ dur, int32_t *__restrict__ status) {
  using L = PeriodicLayout<K>;
  constexpr int NU = K - 1, NC = 2 * K;

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

  // input checks: the first knot here, every later knot and duration as the forward sweep reads it (the last lambda);
  // the elimination runs whatever they find, and the status masks the stores
  bool nonfinite = !finite64(lt[0]) | !finite64(lw[0]);
  bool badtime = lt[0] != 0.0;

  // the ring elimination with its refinement step; each segment is stored as it is recovered
  const RingLane rl = {lw, lt, sX + dl, sG + dl, sH + dl, sZ + lane, sZ2 + lane, kDronesPerWave};
  bool singular;
  int st = MSNAP_ST_OK;
  ring_solve<K, /*REFINE*/ true, kDronesPerWave>(
      rl, M, singular,
      [&](int i, double (&c)[NC], double) {
        // (the first segment handed over: every input has been seen and every pivot taken)
        if (i == M - 1) st = drone_status(nonfinite, badtime, singular);
        if constexpr (NC == 8)
          store_segment_quad8(MSNAP_SEG_BASE(coef, tile, M, i, NC), MSNAP_SEG_STRIDE(M, NC), nvalid, lane, c, st != 0);
        else
          store_segment_coalesced<NC>(sTr, MSNAP_SEG_BASE(coef, tile, M, i, NC), MSNAP_SEG_STRIDE(M, NC), nvalid, lane,
                                      c, st != 0);
      },
      [&](double t, double w, double T) {
        nonfinite |= !finite64(t) | !finite64(w);
        badtime |= !(T > 0.0);
      });
  if (live && a == 0) status[tile * kDronesPerWave + dl] = st;
}

}  // namespace

int launch_solve_periodic(msnap_ctx *ctx, const SolveCall &c) {
  auto go = [&](auto kernel, size_t lds_bytes) {
    return launch_tiles(ctx, kernel, lds_bytes, c.n_drones, c.wp, c.t, c.shared_times ? 1 : 0, c.n_drones, c.n_seg,
                        c.coef, c.dur, c.status);
  };
  return ctx->khalf == 4 ? go(&periodic_solve_kernel<4>, PeriodicLayout<4>::bytes(c.n_seg))
                         : go(&periodic_solve_kernel<5>, PeriodicLayout<5>::bytes(c.n_seg));
}

int periodic_max_segments(int khalf) {
  return khalf == 4 ? PeriodicLayout<4>::max_segments() : PeriodicLayout<5>::max_segments();
}

}  // namespace msnap
