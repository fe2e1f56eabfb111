"""Inputs for the caps and edges of msnap_optimize_times_gates that tests/golden/make_timeopt_gates_golden.py does not
reach (include/msnap.h, msnap_optimize_times_gates): tests/test_timeopt_gates_edges_cpu.py holds the
structure of every builder, tests/golden/make_timeopt_gates_edges_golden.py records the reference figures of the groups
below, tests/test_timeopt_gates_edges_gpu.py holds the kernel on the same inputs.

Every builder is a pure NumPy function with fixed seeds and returns (wp, t, start, end, fix, via) in the layout of
tests/gates_cases.py; a drone whose combination lacks a block has a row of zeros in it.  The waypoints, times and end
states are SE.case's, the gate values GC.values', the six-segment families GC's own.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gates_cases as GC  # noqa: E402
import states_exact as SE  # noqa: E402

W1 = (1.0, 1.0, 1.0, 1.0)
CAP = {7: 79, 9: 57}                # msnap_optimize_times_gates_max_segments: a full 8-drone tile fills the LDS there
N_CAP = 11                          # a full 8-drone tile and a tail of 3
# the end-state combination of place d mod 4: place 3 carries no gate, and drones 7 (the last of the full tile) and 10
# (the last of the call) carry an `end` block -- the last words of the two state images in LDS
CAP_COMBOS = ("start", "neither", "both", "end")
WORD = 64                           # segments 64 .. live in the second word of the free-set bitmask
FLOOR_FRACTION = 0.5                # B
SQUEEZED = tuple(range(60, 79, 4))  # B: the segments whose durations are multiplied by SQUEEZE
SQUEEZE = 0.15


EXACT_BAR = 1e-10                   # norm_rel to 60 digits: the bar msnap_solve_gates is held to (K21)
# Where float64 itself misses that bar: drone 0 of the order-9 cap groups at its allocated times (durations 11 : 1 with
# gates, 17 : 1 without).  The figures are the NumPy restatement's norm_rel to the 60-digit solve at its own t_out
# (tol 1e-4, 500 steps); tests/test_timeopt_gates_edges_cpu.py measures them again, and the kernel's coefficients of that
# drone are held to 10 times the figure, the margin prefix_sens gets.
RESTATED_AT_T_OUT = {("cap9", 0): 1.94e-10, ("cap9_plain", 0): 1.51e-8}


def exact_bar(name, d, max_iter):
    """the bar on norm_rel(coef, 60 digits at t_out) of drone d of the fixture's group `name`"""
    return 10.0 * RESTATED_AT_T_OUT[name, d] if max_iter > 0 and (name, d) in RESTATED_AT_T_OUT else EXACT_BAR


def combo_of(d):
    return CAP_COMBOS[d % 4]


def always_gated(order):
    """the knots every gated drone of the cap groups gates: the first two, the last two, and at order 7 the three
    around the word boundary of the free-set bitmask"""
    M = CAP[order]
    return (1, 2, M - 2, M - 1) + ((WORD - 1, WORD, WORD + 1) if M > WORD + 2 else ())


def cap_masks(order):
    """fix [11, M-1] at the cap: drones at place 3 mod 4 carry nothing; a gated drone gates always_gated(order) and,
    one in two, the knots between; the gated knots take the non-empty mask values 1 .. 2^(K-1) - 1 in turn."""
    M = CAP[order]
    nm = 2 ** (GC.half(order) - 1)
    rng = np.random.default_rng(260000 + order)
    fix = np.zeros((N_CAP, M - 1), dtype=np.int32)
    always, count = always_gated(order), 0
    for d in range(N_CAP):
        if d % 4 == 3:
            continue
        for i in range(1, M):
            if i in always or rng.random() < 0.5:
                fix[d, i - 1] = 1 + count % (nm - 1)
                count += 1
    return fix


# ---- A. the caps ----------------------------------------------------------------------------------------------------
def cap(order, gated=True):
    """SE.case(order, cap, 11) with the four end-state combinations cycling (CAP_COMBOS) and cap_masks' gates;
    gated False: the same drones with an empty mask everywhere and NaN values (the end-state mode's problem)"""
    M = CAP[order]
    wp, t, start, end = SE.case(order, M, N_CAP)
    for d in range(N_CAP):
        if combo_of(d) not in ("start", "both"):
            start[d] = 0.0
        if combo_of(d) not in ("end", "both"):
            end[d] = 0.0
    fix = cap_masks(order) if gated else np.zeros((N_CAP, M - 1), dtype=np.int32)
    return wp, t, start, end, fix, GC.values(order, fix, 270000 + order)


# ---- B. the floor beyond segment 64 ---------------------------------------------------------------------------------
def floor():
    """A's order-7 batch -- waypoints, end states, masks -- with the durations of segments 60, 64, 68, 72 and 76 times
    0.15: at min_fraction = 0.5 the input lies below the floor there (and wherever a drawn duration does), on both
    sides of segment 64.  The gate values are drawn from a seed of the group's own, the first of those tried that
    leaves segments 64 .. at their floor at the optimum of four drones and more."""
    wp, t, start, end, fix, via = cap(7)
    return wp, squeezed(t), start, end, fix, GC.values(7, fix, 280008)


def squeezed(t):
    """t [.., M+1] with the durations of the segments SQUEEZED times SQUEEZE"""
    dur = np.diff(t, axis=-1)
    dur[..., list(SQUEEZED)] *= SQUEEZE
    return np.concatenate([np.zeros(t.shape[:-1] + (1,)), np.cumsum(dur, axis=-1)], axis=-1)


# ---- the groups of the fixture --------------------------------------------------------------------------------------
def groups(z=None):
    """[(name, order, min_fraction, combos [N], batch)]: one call of the GPU test per entry, in the fixture's order.
    With the loaded fixture `z`, the drones its generator had to draw again (the two reference methods ended in
    different minima) are the ones it recorded: everything but the masks of such a drone comes from the file."""
    out = built()
    if z is None:
        return out
    first = {int(g): int(np.flatnonzero(z["group"] == g)[0]) for g in np.unique(z["group"])}
    for j, k in enumerate(z["r_k"].tolist()):
        g = int(z["group"][k])
        name, order, mf, combos, batch = out[g]
        d, nd, M = k - first[g], half(order) - 1, batch[0].shape[1] - 1
        lo, glo = int(z["r_off"][j]), int(z["r_goff"][j])
        wp, t, start, end, fix, via = batch
        wp[d], t[d] = z["r_wp"][lo:lo + M + 1].astype(np.float64), z["r_t"][lo:lo + M + 1]
        start[d], end[d], via[d] = z["r_start"][j][:, :nd], z["r_end"][j][:, :nd], z["r_via"][glo:glo + M - 1, :, :nd]
    return out


def half(order):
    return GC.half(order)


def built():
    """groups() as the seeds alone give them"""
    out = []
    combos = [combo_of(d) for d in range(N_CAP)]
    for order in (7, 9):
        out.append((f"cap{order}", order, 0.1, combos, cap(order)))
    for order in (7, 9):
        out.append((f"cap{order}_plain", order, 0.1, combos, cap(order, gated=False)))
    out.append(("floor7", 7, FLOOR_FRACTION, combos, floor()))
    for order in (7, 9):
        case = GC.stiff(order)
        out.append((f"stiff{order}", order, 0.1, ["both"] * case[0].shape[0], case))
    return out


def drone_of(batch, combo, d):
    """(wp, t, start, end, fix, via) of drone d as the restatement takes them: a block the combination lacks is None"""
    wp, t, start, end, fix, via = batch
    return (wp[d], t[d], start[d] if combo in ("start", "both") else None, end[d] if combo in ("end", "both") else None,
            fix[d], via[d])


def unpack(z):
    """The fixture tests/golden/timeopt_gates_edges_golden.npz as {group name: [per-drone dict]}: k, J0, J_ref, J4,
    gap4, conv4, iters4, p_t (max_iter 1, 3), p_iters, p_margin, prefix_sens, active (segment indices)"""
    out = {}
    names = [str(x) for x in z["gname"]]
    for k in range(int(z["n"])):
        lo, hi = int(z["off"][k]), int(z["off"][k + 1])
        alo, ahi = int(z["aoff"][k]), int(z["aoff"][k + 1])
        out.setdefault(names[int(z["group"][k])], []).append({
            "k": k, "J0": float(z["J0"][k]), "J_ref": float(z["J_ref"][k]), "J4": float(z["J4"][k]),
            "gap4": float(z["gap4"][k]), "conv4": bool(z["conv4"][k]), "iters4": int(z["iters4"][k]),
            "p_t": (z["p_t1"][lo:hi], z["p_t3"][lo:hi]), "p_iters": z["p_iters"][k], "p_margin": z["p_margin"][k],
            "prefix_sens": z["prefix_sens"][k], "active": z["act"][alo:ahi], "n_below": int(z["n_below"][k])})
    return out
