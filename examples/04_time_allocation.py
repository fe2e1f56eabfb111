"""Time allocation: the node's uniform grid -> per-drone optimised segment times -> retimed to dynamic limits.

    python examples/04_time_allocation.py

Prints, per drone, the snap cost at the optimised times over the cost on the uniform grid, and the common scale the
limits then ask for.  Needs the MI355X (there is no CPU fallback)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from drone_path_planning_python_amd import Context  # noqa: E402


def main():
    rng = np.random.default_rng(4)
    n, m = 8, 12
    wp = np.cumsum(rng.normal(size=(n, m + 1, 4)) * [1.0, 1.0, 0.4, 0.2], axis=1)
    t = np.arange(m + 1) * (10.0 / (m + 1))                      # the node's grid (shared by the batch)
    with Context(order=7, max_segments=64) as ctx:
        coef0, dur0, status = ctx.solve_batch(wp, t)
        assert (status == 0).all()
        t_out, coef, dur, status, info = ctx.optimize_times(wp, t, min_fraction=0.1, max_iter=200, tol=1e-4)
        assert (status == 0).all()
        ratio = info["cost"][:, 1] / info["cost"][:, 0]
        for d in range(n):
            print(f"drone {d}: cost ratio {ratio[d]:.3f} after {int(info['iters'][d])} steps (measure {info['pg'][d]:.1e}); "
                  f"shortest segment {dur[d].min():.3f} s of {dur[d].sum():.3f} s")
        # the distribution of time is set; now the total, to the limits (one scale: the drones fly together)
        peak0, _, _ = ctx.dynamic_peaks(coef0, dur0)
        peak, _, _ = ctx.dynamic_peaks(coef, dur)
        print("peak speed on the uniform grid %.2f m/s, optimised %.2f m/s" % (peak0[:, 0].max(), peak[:, 0].max()))
        coef_r, dur_r, scale = ctx.retime_to_limits(coef, dur, v_max=2.0, a_max=4.0, fit=True, common=True)
        print("common scale to meet 2 m/s, 4 m/s^2: %.3f -> flight time %.2f s" % (scale[0], dur_r[0].sum()))


if __name__ == "__main__":
    main()
