// K17 -- time allocation with a free total duration (include/msnap.h, msnap_optimize_times_free):
// the free-total mode of the one kernel text in msnap_timeopt_kernel.h, F(T) = J(T) + k_T sum_i T_i from and to given
// end states.  The two instances live in this object of their own, so that what is held of msnap_timeopt.o (four
// kernels, their instructions) stays true.  The entry points are msnap_timeopt.hip's; they reach the instances through
// launch_optimize_times.
#include "msnap_timeopt_kernel.h"

namespace msnap {

int launch_optimize_times_free(msnap_ctx *ctx, const TimeoptCall &call) {
  return timeopt_launch<kTimeoptFree>(ctx, call);
}

}  // namespace msnap
