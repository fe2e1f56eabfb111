// K15 -- closed-loop paths (include/msnap.h, "periodic solve"): the minimum-snap solve whose last
// waypoint is joined to its first, msnap_solve_periodic.  The system is block cyclic tridiagonal; its elimination
// around the ring, with one refinement step, is ring_solve of msnap_ring.h, which has the derivation and is the text
// the time allocation on loops runs as its trial (K16).  periodic_solve_kernel<K> keeps the mapping of
// states_solve_kernel<K> (lane = 4 drone + axis, one wave per 16-drone tile, inputs staged in LDS, the full-line stores)
// and is what stands around that call: stage the inputs, store the durations, check the inputs, hand ring_solve the
// tile's stash at the compile-time tile size, store each segment as it comes back, write the status.
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
  return all_required(ptrs);
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
