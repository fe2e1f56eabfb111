// K8 -- segment-time optimisation per drone, one launch for the whole iteration (include/msnap.h, "time allocation";
// DESIGN.md §5 K8).  The kernel text, its LDS layout and the launcher are msnap_timeopt_kernel.h; this translation unit
// instantiates the rest-to-rest and the end-state mode and holds what every mode shares above the kernel: the one
// launch function, the argument check, the staging of a host-pointer call and the entry points of all five modes.
// msnap_timeopt_periodic.hip holds the ring mode's instances (msnap_optimize_times_periodic), msnap_timeopt_free.hip
// the free-total mode's (msnap_optimize_times_free), msnap_timeopt_gates.hip the gates mode's
// (msnap_optimize_times_gates).
#include "msnap_api_util.h"
#include "msnap_timeopt_kernel.h"

namespace msnap {

int timeopt_max_segments(int khalf, int mode) { return timeopt_tile_segments(khalf, 8, mode); }

int launch_optimize_times(msnap_ctx *ctx, int mode, const TimeoptCall &call) {
  switch (mode) {
    case kTimeoptRing: return launch_optimize_times_ring(ctx, call);
    case kTimeoptFree: return launch_optimize_times_free(ctx, call);
    case kTimeoptGates: return launch_optimize_times_gates(ctx, call);
    case kTimeoptEnds: return timeopt_launch<kTimeoptEnds>(ctx, call);
    default: return timeopt_launch<kTimeoptRest>(ctx, call);
  }
}

namespace {

// The argument check every allocation entry and its _device twin make (the pointers a mode requires: TimeoptCall)
int timeopt_args(const msnap_ctx *ctx, int mode, const TimeoptCall &c) {
  if (!ctx || c.n_drones < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, c.n_seg)) return rc;
  if (c.n_seg > timeopt_max_segments(ctx->khalf, mode)) return MSNAP_ESEGMENTS;
  if (mode == kTimeoptRing && c.n_seg < 2) return MSNAP_ESEGMENTS;      // (a loop has two segments at least)
  if (!c.weights || !(c.min_fraction > 0.0 && c.min_fraction <= 1.0) || c.max_iter < 0 || !(c.tol >= 0.0))
    return MSNAP_EINVAL;
  for (int q = 0; q < 4; ++q)
    if (!(c.weights[q] >= 0.0) || !(c.weights[q] <= 1.79769313486231570815e308)) return MSNAP_EINVAL;   // negative, NaN, Inf
  if (c.n_drones == 0) return kNoWork;
  if (!c.wp || !c.t || !c.t_out || !c.coef || !c.dur || !c.status) return MSNAP_EINVAL;
  if (mode == kTimeoptFree && !c.time_weight) return MSNAP_EINVAL;
  if (mode == kTimeoptGates && c.fix && !c.via) return MSNAP_EINVAL;      // (masks without values)
  return MSNAP_OK;
}

// Every allocation entry: check, then launch on the caller's device pointers (on_device), or stage the caller's host
// arrays, launch on the staged copies and read back.
int optimize_times_entry(msnap_ctx *ctx, int mode, const TimeoptCall &c, bool on_device) {
  MSNAP_ENTER(ctx, timeopt_args(ctx, mode, c));
  if (on_device) return launch_optimize_times(ctx, mode, c);
  const size_t n = (size_t)c.n_drones, m1 = (size_t)c.n_seg + 1;
  const bool gated = mode == kTimeoptGates && c.fix && c.n_seg >= 2;
  const bool ends = mode == kTimeoptEnds || mode == kTimeoptFree || mode == kTimeoptGates, free_total = mode == kTimeoptFree;
  const size_t b_s = ends ? n * 4 * (ctx->khalf - 1) * 8 : 0, b_k = free_total ? n * 8 : 0;
  const size_t b_f = gated ? n * (m1 - 2) * 4 : 0, b_v = gated ? n * (m1 - 2) * 4 * (ctx->khalf - 1) * 8 : 0;
  // (a region without a source is not copied: a NULL state stays NULL for the launcher)
  return staged(ctx, {upload(c.wp, n * m1 * 4 * 8), upload(c.t, (c.shared_times ? 1 : n) * m1 * 8),
                      download(c.t_out, n * m1 * 8), download(c.coef, coef_bytes(ctx, c.n_drones, c.n_seg)),
                      download(c.dur, dur_bytes(c.n_drones, c.n_seg)), download(c.status, n * 4),
                      download(c.cost, c.cost ? n * 16 : 0), download(c.pg, c.pg ? n * 8 : 0),
                      download(c.iters, c.iters ? n * 4 : 0), upload(c.start, c.start ? b_s : 0),
                      upload(c.end, c.end ? b_s : 0), upload(c.time_weight, b_k), upload(c.fix, b_f),
                      upload(c.via, b_v)},
                [&](const DevPtr *d) {
                  TimeoptCall dev = c;
                  dev.wp = d[0];
                  dev.t = d[1];
                  dev.t_out = d[2];
                  dev.coef = d[3];
                  dev.dur = d[4];
                  dev.status = d[5];
                  if (c.cost) dev.cost = d[6];
                  if (c.pg) dev.pg = d[7];
                  if (c.iters) dev.iters = d[8];
                  dev.start = ends && c.start ? (const double *)d[9] : nullptr;
                  dev.end = ends && c.end ? (const double *)d[10] : nullptr;
                  dev.time_weight = free_total ? (const double *)d[11] : nullptr;
                  dev.fix = gated ? (const int32_t *)d[12] : nullptr;
                  dev.via = gated ? (const double *)d[13] : nullptr;
                  return launch_optimize_times(ctx, mode, dev);
                });
}

int max_segments_entry(int order, int mode) {
  if (order != 7 && order != 9) return MSNAP_EORDER;
  return timeopt_max_segments((order + 1) / 2, mode);
}

}  // namespace
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

// The allocation entries fill the call record in its field order (a mode without end states, a time weight or gates
// leaves them null) and differ in the mode and in whose pointers they take; weights is a host array in both versions.
int msnap_optimize_times_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, const double weights[4], double min_fraction, int max_iter,
                                double tol, double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, nullptr, nullptr, weights, nullptr, min_fraction,
                         max_iter, tol, t_out, coef, dur, status, cost, pg, iters};
  return optimize_times_entry(ctx, kTimeoptRest, c, true);
}

int msnap_optimize_times(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared_times,
                         const double weights[4], double min_fraction, int max_iter, double tol, double *t_out,
                         double *coef, double *dur, int32_t *status, double *cost, double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, nullptr, nullptr, weights, nullptr, min_fraction,
                         max_iter, tol, t_out, coef, dur, status, cost, pg, iters};
  return optimize_times_entry(ctx, kTimeoptRest, c, false);
}

int msnap_optimize_times_states_max_segments(int order) { return max_segments_entry(order, kTimeoptEnds); }

int msnap_optimize_times_states_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                       int shared_times, const double *start, const double *end,
                                       const double weights[4], double min_fraction, int max_iter, double tol,
                                       double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                       double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, start, end, weights, nullptr, min_fraction, max_iter,
                         tol, t_out, coef, dur, status, cost, pg, iters};
  return optimize_times_entry(ctx, kTimeoptEnds, c, true);
}

int msnap_optimize_times_states(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                int shared_times, const double *start, const double *end, const double weights[4],
                                double min_fraction, int max_iter, double tol, double *t_out, double *coef, double *dur,
                                int32_t *status, double *cost, double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, start, end, weights, nullptr, min_fraction, max_iter,
                         tol, t_out, coef, dur, status, cost, pg, iters};
  return optimize_times_entry(ctx, kTimeoptEnds, c, false);
}

int msnap_optimize_times_periodic_max_segments(int order) { return max_segments_entry(order, kTimeoptRing); }

int msnap_optimize_times_periodic_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                         int shared_times, const double weights[4], double min_fraction, int max_iter,
                                         double tol, double *t_out, double *coef, double *dur, int32_t *status,
                                         double *cost, double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, nullptr, nullptr, weights, nullptr, min_fraction,
                         max_iter, tol, t_out, coef, dur, status, cost, pg, iters};
  return optimize_times_entry(ctx, kTimeoptRing, c, true);
}

int msnap_optimize_times_periodic(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                  int shared_times, const double weights[4], double min_fraction, int max_iter,
                                  double tol, double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                                  double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, nullptr, nullptr, weights, nullptr, min_fraction,
                         max_iter, tol, t_out, coef, dur, status, cost, pg, iters};
  return optimize_times_entry(ctx, kTimeoptRing, c, false);
}

int msnap_optimize_times_free_max_segments(int order) { return max_segments_entry(order, kTimeoptFree); }

int msnap_optimize_times_free_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                     int shared_times, const double *start, const double *end,
                                     const double weights[4], const double *time_weight, double min_fraction,
                                     int max_iter, double tol, double *t_out, double *coef, double *dur,
                                     int32_t *status, double *cost, double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, start, end, weights, time_weight, min_fraction, max_iter,
                         tol, t_out, coef, dur, status, cost, pg, iters};
  return optimize_times_entry(ctx, kTimeoptFree, c, true);
}

int msnap_optimize_times_free(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                              int shared_times, const double *start, const double *end, const double weights[4],
                              const double *time_weight, double min_fraction, int max_iter, double tol, double *t_out,
                              double *coef, double *dur, int32_t *status, double *cost, double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, start, end, weights, time_weight, min_fraction, max_iter,
                         tol, t_out, coef, dur, status, cost, pg, iters};
  return optimize_times_entry(ctx, kTimeoptFree, c, false);
}

int msnap_optimize_times_gates_max_segments(int order) { return max_segments_entry(order, kTimeoptGates); }

int msnap_optimize_times_gates_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                                      int shared_times, const double *start, const double *end, const int32_t *fix,
                                      const double *via, const double weights[4], double min_fraction, int max_iter,
                                      double tol, double *t_out, double *coef, double *dur, int32_t *status,
                                      double *cost, double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, start, end, weights, nullptr, min_fraction, max_iter,
                         tol, t_out, coef, dur, status, cost, pg, iters, fix, via};
  return optimize_times_entry(ctx, kTimeoptGates, c, true);
}

int msnap_optimize_times_gates(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                               int shared_times, const double *start, const double *end, const int32_t *fix,
                               const double *via, const double weights[4], double min_fraction, int max_iter,
                               double tol, double *t_out, double *coef, double *dur, int32_t *status, double *cost,
                               double *pg, int32_t *iters) {
  const TimeoptCall c = {n_drones, n_seg, wp, t, shared_times, start, end, weights, nullptr, min_fraction, max_iter,
                         tol, t_out, coef, dur, status, cost, pg, iters, fix, via};
  return optimize_times_entry(ctx, kTimeoptGates, c, false);
}

}  // extern "C"
