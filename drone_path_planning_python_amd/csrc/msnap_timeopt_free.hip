// K17 -- time allocation with a free total duration (include/msnap.h, msnap_optimize_times_free):
// the free-total mode of the one kernel text in msnap_timeopt_kernel.h, F(T) = J(T) + k_T sum_i T_i from and to given
// end states.  The two instances and their entry points live in this object of their own, so that what is held of
// msnap_timeopt.o (four kernels, their instructions) stays true.
#include "msnap_timeopt_kernel.h"

using namespace msnap;

extern "C" {

int msnap_optimize_times_free_max_segments(int order) {
  if (order != 7 && order != 9) return MSNAP_EORDER;
  return timeopt_max_segments((order + 1) / 2, kTimeoptFree);
}

int msnap_optimize_times_free_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                     int shared_times, const double *start, const double *end,
                                     const double weights[4], const double *time_weight, double min_fraction,
                                     int max_iter, double tol, double *t_out, double *coef, double *dur,
                                     int32_t *status, double *cost, double *pg, int32_t *iters) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, n_drones, n_seg, kTimeoptFree, weights, min_fraction, max_iter, tol,
                                {wp, t, time_weight, t_out, coef, dur, status}));
  return timeopt_launch<kTimeoptFree>(ctx, n_drones, n_seg, wp, t, shared_times ? 1 : 0, start, end, weights,
                                      min_fraction, max_iter, tol, t_out, coef, dur, status, cost, pg, iters,
                                      time_weight);
}

int msnap_optimize_times_free(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                              int shared_times, const double *start, const double *end, const double weights[4],
                              const double *time_weight, double min_fraction, int max_iter, double tol, double *t_out,
                              double *coef, double *dur, int32_t *status, double *cost, double *pg, int32_t *iters) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, n_drones, n_seg, kTimeoptFree, weights, min_fraction, max_iter, tol,
                                {wp, t, time_weight, t_out, coef, dur, status}));
  const size_t n = (size_t)n_drones, m1 = (size_t)n_seg + 1;
  const size_t b_s = n * 4 * (ctx->khalf - 1) * 8;
  // (a region without a source is not copied: a NULL state stays NULL for the launcher)
  return staged(ctx, {upload(wp, n * m1 * 4 * 8), upload(t, (shared_times ? 1 : n) * m1 * 8), download(t_out, n * m1 * 8),
                      download(coef, coef_bytes(ctx, n_drones, n_seg)), download(dur, dur_bytes(n_drones, n_seg)),
                      download(status, n * 4), download(cost, cost ? n * 16 : 0), download(pg, pg ? n * 8 : 0),
                      download(iters, iters ? n * 4 : 0), upload(start, start ? b_s : 0), upload(end, end ? b_s : 0),
                      upload(time_weight, n * 8)},
                [&](const DevPtr *d) {
                  return timeopt_launch<kTimeoptFree>(
                      ctx, n_drones, n_seg, d[0], d[1], shared_times ? 1 : 0, start ? (const double *)d[9] : nullptr,
                      end ? (const double *)d[10] : nullptr, weights, min_fraction, max_iter, tol, d[2], d[3], d[4],
                      d[5], cost ? (double *)d[6] : nullptr, pg ? (double *)d[7] : nullptr,
                      iters ? (int32_t *)d[8] : nullptr, d[11]);
                });
}

}  // extern "C"
