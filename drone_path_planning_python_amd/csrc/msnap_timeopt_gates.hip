// K22 -- time allocation through gates (include/msnap.h, msnap_optimize_times_gates): the gates mode
// of the one kernel text in msnap_timeopt_kernel.h, the end-state mode with prescribed derivatives at interior knots
// as data of every trial (chain_solve's GATES, as msnap_solve_gates runs it).  The two instances live in this object of
// their own, so that what is held of msnap_timeopt.o (four kernels, their instructions) stays true.  The entry points
// are msnap_timeopt.hip's; they reach the instances through launch_optimize_times.
#include "msnap_timeopt_kernel.h"

namespace msnap {

int launch_optimize_times_gates(msnap_ctx *ctx, const TimeoptCall &call) {
  return timeopt_launch<kTimeoptGates>(ctx, call);
}

}  // namespace msnap
