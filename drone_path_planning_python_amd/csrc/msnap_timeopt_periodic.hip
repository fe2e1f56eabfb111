// K16 -- time allocation on closed loops (include/msnap.h, msnap_optimize_times_periodic): the ring
// mode of the one kernel text in msnap_timeopt_kernel.h, whose trial is ring_solve of msnap_ring.h.  The instances
// live in this object of their own: at order 9 they fill the 256 architectural VGPRs and keep 166 values in
// accumulation registers (no scratch), and msnap_timeopt.o is held to no such copy at all.  The entry points are
// msnap_timeopt.hip's; they reach the instances through launch_optimize_times.
#include "msnap_timeopt_kernel.h"

namespace msnap {

int launch_optimize_times_ring(msnap_ctx *ctx, const TimeoptCall &call) {
  return timeopt_launch<kTimeoptRing>(ctx, call);
}

}  // namespace msnap
