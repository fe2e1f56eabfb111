// K8 -- segment-time optimisation per drone, one launch for the whole iteration (include/msnap.h, "time allocation";
// DESIGN.md §5 K8).  The kernel text, its LDS layout and the launcher are msnap_timeopt_kernel.h; this translation unit
// instantiates the rest-to-rest and the end-state mode and holds the entry points of the three fixed-total modes,
// msnap_timeopt_periodic.hip the ring mode (msnap_optimize_times_periodic), msnap_timeopt_free.hip the free-total mode
// with its own entries (msnap_optimize_times_free).
#include "msnap_timeopt_kernel.h"

namespace msnap {

int timeopt_max_segments(int khalf, int mode) { return timeopt_tile_segments(khalf, 8, mode); }

// mode 0: msnap_optimize_times; 1: msnap_optimize_times_states (start / end: device pointers or null); 2:
// msnap_optimize_times_periodic
int launch_optimize_times(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                          int mode, const double *start, const double *end, const double *weights,
                          double min_fraction, int max_iter, double tol, double *t_out, double *coef, double *dur,
                          int32_t *status, double *cost, double *pg, int32_t *iters) {
  if (mode == kTimeoptRing)
    return launch_optimize_times_ring(ctx, n_drones, n_seg, wp, t, shared_times, weights, min_fraction, max_iter, tol,
                                      t_out, coef, dur, status, cost, pg, iters);
  if (mode == kTimeoptEnds)
    return timeopt_launch<kTimeoptEnds>(ctx, n_drones, n_seg, wp, t, shared_times, start, end, weights, min_fraction,
                                        max_iter, tol, t_out, coef, dur, status, cost, pg, iters);
  return timeopt_launch<kTimeoptRest>(ctx, n_drones, n_seg, wp, t, shared_times, nullptr, nullptr, weights,
                                      min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters);
}

}  // namespace msnap

// ------------------------------------------------------------------ C-ABI (include/msnap.h, "time allocation")
using namespace msnap;

extern "C" {

int msnap_snap_cost_grad_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                double *grad) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {coef, dur, grad}));
  return launch_snap_cost_grad(ctx, n_drones, n_seg, coef, grad);
}

int msnap_snap_cost_grad(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, double *grad) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {coef, dur, grad}));
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), download(grad, (size_t)n_drones * n_seg * 4 * 8)},
                [&](const DevPtr *d) { return launch_snap_cost_grad(ctx, n_drones, n_seg, d[0], d[1]); });
}

// ------------------------------------------------------------------ time allocation (msnap_timeopt.hip)
// weights is a host array in both versions; cost, pg and iters are optional (the argument check: timeopt_args of
// msnap_timeopt_kernel.h)
namespace {
// the host entries: stage, launch, read back (start / end: host pointers or null, looked at with kTimeoptEnds only)
int optimize_times_host(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                        int mode, const double *start, const double *end, const double *weights, double min_fraction,
                        int max_iter, double tol, double *t_out, double *coef, double *dur, int32_t *status,
                        double *cost, double *pg, int32_t *iters) {
  const size_t n = (size_t)n_drones, m1 = (size_t)n_seg + 1;
  const size_t b_s = n * 4 * (ctx->khalf - 1) * 8;
  const bool ends = mode == kTimeoptEnds;
  // (a region without a source is not copied: a NULL state stays NULL for the launcher)
  return staged(ctx, {upload(wp, n * m1 * 4 * 8), upload(t, (shared_times ? 1 : n) * m1 * 8), download(t_out, n * m1 * 8),
                      download(coef, coef_bytes(ctx, n_drones, n_seg)), download(dur, dur_bytes(n_drones, n_seg)),
                      download(status, n * 4), download(cost, cost ? n * 16 : 0), download(pg, pg ? n * 8 : 0),
                      download(iters, iters ? n * 4 : 0), upload(start, ends && start ? b_s : 0),
                      upload(end, ends && end ? b_s : 0)},
                [&](const DevPtr *d) {
                  return launch_optimize_times(ctx, n_drones, n_seg, d[0], d[1], shared_times ? 1 : 0, mode,
                                               ends && start ? (const double *)d[9] : nullptr,
                                               ends && end ? (const double *)d[10] : nullptr, weights, min_fraction,
                                               max_iter, tol, d[2], d[3], d[4], d[5], cost ? (double *)d[6] : nullptr,
                                               pg ? (double *)d[7] : nullptr, iters ? (int32_t *)d[8] : nullptr);
                });
}
}  // namespace

int msnap_optimize_times_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, const double weights[4], double min_fraction, int max_iter,
                                double tol, double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                double *pg, int32_t *iters) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, n_drones, n_seg, kTimeoptRest, weights, min_fraction, max_iter, tol,
                                {wp, t, t_out, coef, dur, status}));
  return launch_optimize_times(ctx, n_drones, n_seg, wp, t, shared_times ? 1 : 0, kTimeoptRest, nullptr, nullptr, weights,
                               min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters);
}

int msnap_optimize_times(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                         const double weights[4], double min_fraction, int max_iter, double tol, double *t_out,
                         double *coef, double *dur, int32_t *status, double *cost, double *pg, int32_t *iters) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, n_drones, n_seg, kTimeoptRest, weights, min_fraction, max_iter, tol,
                                {wp, t, t_out, coef, dur, status}));
  return optimize_times_host(ctx, n_drones, n_seg, wp, t, shared_times, kTimeoptRest, nullptr, nullptr, weights, min_fraction,
                             max_iter, tol, t_out, coef, dur, status, cost, pg, iters);
}

int msnap_optimize_times_states_max_segments(int order) {
  if (order != 7 && order != 9) return MSNAP_EORDER;
  return timeopt_max_segments((order + 1) / 2, kTimeoptEnds);
}

int msnap_optimize_times_states_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                       int shared_times, const double *start, const double *end,
                                       const double weights[4], double min_fraction, int max_iter, double tol,
                                       double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                       double *pg, int32_t *iters) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, n_drones, n_seg, kTimeoptEnds, weights, min_fraction, max_iter, tol,
                                {wp, t, t_out, coef, dur, status}));
  return launch_optimize_times(ctx, n_drones, n_seg, wp, t, shared_times ? 1 : 0, kTimeoptEnds, start, end, weights,
                               min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters);
}

int msnap_optimize_times_states(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, const double *start, const double *end, const double weights[4],
                                double min_fraction, int max_iter, double tol, double *t_out, double *coef, double *dur,
                                int32_t *status, double *cost, double *pg, int32_t *iters) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, n_drones, n_seg, kTimeoptEnds, weights, min_fraction, max_iter, tol,
                                {wp, t, t_out, coef, dur, status}));
  return optimize_times_host(ctx, n_drones, n_seg, wp, t, shared_times, kTimeoptEnds, start, end, weights, min_fraction,
                             max_iter, tol, t_out, coef, dur, status, cost, pg, iters);
}

int msnap_optimize_times_periodic_max_segments(int order) {
  if (order != 7 && order != 9) return MSNAP_EORDER;
  return timeopt_max_segments((order + 1) / 2, kTimeoptRing);
}

int msnap_optimize_times_periodic_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                         int shared_times, const double weights[4], double min_fraction, int max_iter,
                                         double tol, double *t_out, double *coef, double *dur, int32_t *status,
                                         double *cost, double *pg, int32_t *iters) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, n_drones, n_seg, kTimeoptRing, weights, min_fraction, max_iter, tol,
                                {wp, t, t_out, coef, dur, status}));
  return launch_optimize_times(ctx, n_drones, n_seg, wp, t, shared_times ? 1 : 0, kTimeoptRing, nullptr, nullptr,
                               weights, min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters);
}

int msnap_optimize_times_periodic(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                  int shared_times, const double weights[4], double min_fraction, int max_iter,
                                  double tol, double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                  double *pg, int32_t *iters) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, n_drones, n_seg, kTimeoptRing, weights, min_fraction, max_iter, tol,
                                {wp, t, t_out, coef, dur, status}));
  return optimize_times_host(ctx, n_drones, n_seg, wp, t, shared_times, kTimeoptRing, nullptr, nullptr, weights,
                             min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters);
}

}  // extern "C"
