/* Plain-C consumer of the time-allocation entries of include/msnap.h: optimises the times of BASELINE.json
 * configs[0] (4 waypoints, t = 0,1,3,4) on the GPU, checks the contract's guarantees and the gradient entry against
 * the solve's own cost by central differences.  Built and run by tests/test_timeopt_gpu.py::test_c_abi_from_plain_c. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "msnap.h"

static double total_cost(msnap_ctx *ctx, const double *wp, const double *t) {
  double coef[3][4][8], dur[3], cost[4];
  int32_t status[1];
  if (msnap_solve_batch(ctx, 1, 3, wp, t, 0, &coef[0][0][0], dur, status) != MSNAP_OK || status[0] != MSNAP_ST_OK) exit(20);
  if (msnap_snap_cost(ctx, 1, 3, &coef[0][0][0], dur, cost) != MSNAP_OK) exit(21);
  return ((cost[0] + cost[1]) + cost[2]) + cost[3];
}

int main(void) {
  const double wp[4][4] = {{0, 0, 0, 0}, {2, 2.2, 0.3, 0}, {4, 8, 0.8, 0}, {1, 2, 0.4, 0.5}};
  const double t[4] = {0, 1, 3, 4};
  const double w[4] = {1, 1, 1, 1}, wneg[4] = {1, 1, -1, 1};
  double t_out[4], coef[3][4][8], dur[3], cost[2], pg[1], grad[3][4];
  int32_t status[1], iters[1];
  msnap_ctx *ctx = NULL;
  int rc = msnap_create(&ctx, 0, 7, 16);
  if (rc != MSNAP_OK) {
    fprintf(stderr, "msnap_create: %s\n", msnap_strerror(rc));
    return 2;
  }
  if (msnap_version() < 400) return 3;
  /* argument errors write nothing */
  t_out[1] = -7.0;
  if (msnap_optimize_times(ctx, 1, 3, &wp[0][0], t, 0, wneg, 0.1, 10, 1e-4, t_out, &coef[0][0][0], dur, status, cost, pg,
                           iters) != MSNAP_EINVAL) return 4;
  if (msnap_optimize_times(ctx, 1, 3, &wp[0][0], t, 0, w, 0.0, 10, 1e-4, t_out, &coef[0][0][0], dur, status, cost, pg,
                           iters) != MSNAP_EINVAL) return 5;
  if (msnap_optimize_times(ctx, 1, 17, &wp[0][0], t, 0, w, 0.1, 10, 1e-4, t_out, &coef[0][0][0], dur, status, cost, pg,
                           iters) != MSNAP_ESEGMENTS) return 6;
  if (t_out[1] != -7.0) return 7;
  rc = msnap_optimize_times(ctx, 1, 3, &wp[0][0], t, 0, w, 0.1, 200, 1e-4, t_out, &coef[0][0][0], dur, status, cost, pg, iters);
  if (rc != MSNAP_OK || status[0] != MSNAP_ST_OK) {
    fprintf(stderr, "msnap_optimize_times: %s (%s), status %d\n", msnap_strerror(rc), msnap_last_hip_error(ctx), status[0]);
    return 8;
  }
  if (t_out[0] != 0.0 || t_out[3] != t[3]) return 9;
  for (int i = 0; i < 3; ++i)
    if (dur[i] != t_out[i + 1] - t_out[i] || dur[i] < 0.1 * t[3] / 3 * (1 - 1e-12)) return 10;
  if (!(cost[1] < cost[0]) || iters[0] < 1 || !(pg[0] <= 1e-4)) return 11;
  if (fabs(cost[0] - total_cost(ctx, &wp[0][0], t)) > 1e-9 * cost[0]) return 12;
  if (fabs(cost[1] - total_cost(ctx, &wp[0][0], t_out)) > 1e-9 * cost[1]) return 13;
  /* cost, pg, iters are optional */
  double t2[4];
  if (msnap_optimize_times(ctx, 1, 3, &wp[0][0], t, 0, w, 0.1, 200, 1e-4, t2, &coef[0][0][0], dur, status, NULL, NULL,
                           NULL) != MSNAP_OK) return 14;
  for (int i = 0; i < 4; ++i)
    if (t2[i] != t_out[i]) return 15;
  /* the gradient entry at the input times against central differences of solve + cost */
  double c0[3][4][8], d0[3];
  if (msnap_solve_batch(ctx, 1, 3, &wp[0][0], t, 0, &c0[0][0][0], d0, status) != MSNAP_OK) return 16;
  if (msnap_snap_cost_grad(ctx, 1, 3, &c0[0][0][0], d0, &grad[0][0]) != MSNAP_OK) return 17;
  double worst = 0.0;
  for (int i = 0; i < 3; ++i) {
    const double h = 1e-5 * d0[i];
    double tp[4] = {t[0], t[1], t[2], t[3]}, tm[4] = {t[0], t[1], t[2], t[3]};
    for (int k = i + 1; k < 4; ++k) {
      tp[k] += h;
      tm[k] -= h;
    }
    const double fd = (total_cost(ctx, &wp[0][0], tp) - total_cost(ctx, &wp[0][0], tm)) / (2 * h);
    const double g = ((grad[i][0] + grad[i][1]) + grad[i][2]) + grad[i][3];
    worst = fmax(worst, fabs(fd - g) / fabs(g));
  }
  msnap_destroy(ctx);
  printf("version %d  t_out %.6f %.6f  cost %.6e -> %.6e  iters %d  pg %.2e  gradient rel err %.2e\n", msnap_version(),
         t_out[1], t_out[2], cost[0], cost[1], (int)iters[0], pg[0], worst);
  return worst < 1e-6 ? 0 : 1;
}
