"""Exact reference of the boundary-state solve (include/msnap.h, "replanning in flight") and the NumPy restatement of
msnap_eval_state.

exact_solve: the dense collocation system of tests/golden/make_order9_golden.py at 60 digits, generalised to given end
derivatives and to both orders -- 2K coefficients per segment; rows: position and derivatives 1..K-1 at both ends, the
position on both sides of every interior knot, continuity of derivatives 1..2K-2 there; one LU for all right-hand sides
(four axes, any number of end-state combinations).  The rows are ordered knot by knot, so the matrix is banded and the
LU only visits the band; the residual of every solution against the unfactored rows is asserted, which would expose a
band chosen too narrow.

eval_state_np: msnap_eval_state's arithmetic, operation by operation.
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 60


def falling(k, j):
    f = 1
    for q in range(k - j + 1, k + 1):
        f *= q
    return f


def deriv_row(nc, j, t):
    """j-th derivative of sum_k c_k t^k at t as a row over c (0**0 == 1)"""
    row = [mp.mpf(0)] * nc
    for k in range(j, nc):
        row[k] = falling(k, j) * (t ** (k - j) if k > j else mp.mpf(1))
    return row


def _assemble(T, K, t_start=None):
    """rows of the collocation matrix as (first column, values) and, per row, where its right-hand side comes from:
    ("w", i) the waypoint i, ("s", q) / ("e", q) the q-th derivative of the start / end state, None: zero.
    t_start: the local time of segment 0 at which its K start rows are taken (None: 0; tests/solve_exact.py passes
    t[0], the reference's start-row quirk)"""
    NC, M = 2 * K, len(T)
    zero = mp.mpf(0)
    rows, src = [], []
    for j in range(K):
        rows.append((0, deriv_row(NC, j, zero if t_start is None else t_start)))
        src.append(("w", 0) if j == 0 else ("s", j))
    for i in range(1, M):
        lo = NC * (i - 1)
        rows.append((lo, deriv_row(NC, 0, T[i - 1]) + [zero] * NC))
        src.append(("w", i))
        rows.append((lo, [zero] * NC + deriv_row(NC, 0, zero)))
        src.append(("w", i))
        for j in range(1, NC - 1):
            rows.append((lo, deriv_row(NC, j, T[i - 1]) + [-v for v in deriv_row(NC, j, zero)]))
            src.append(None)
    for j in range(K):
        rows.append((NC * (M - 1), deriv_row(NC, j, T[M - 1])))
        src.append(("w", M) if j == 0 else ("e", j))
    return rows, src


def _banded_lu_solve(rows, rhs, n, NC):
    """Gaussian elimination with partial pivoting on sparse rows given as (first column, values); rhs: list of columns.
    A row of knot i has its entries in columns [NC (i-1), NC (i+1)) and the rows are in knot order, so the candidates
    for the pivot of column c are among the next 3 NC rows; rows are kept as {column: value}, fill-in included."""
    A = [{lo + q: v for q, v in enumerate(vals) if v != 0} for lo, vals in rows]
    B = [list(col) for col in rhs]
    for c in range(n):
        hi = min(n, c + 3 * NC)
        best, p = mp.mpf(0), -1
        for r in range(c, hi):
            v = A[r].get(c)
            if v is not None and abs(v) > best:
                best, p = abs(v), r
        if p < 0:
            raise ZeroDivisionError("singular system")
        if p != c:
            A[c], A[p] = A[p], A[c]
            for b in B:
                b[c], b[p] = b[p], b[c]
        rowc = A[c]
        inv = 1 / rowc[c]
        tail = [(q, v) for q, v in rowc.items() if q != c]
        for r in range(c + 1, hi):
            rowr = A[r]
            v = rowr.pop(c, None)
            if v is None or v == 0:
                continue
            f = v * inv
            for q, w in tail:
                rowr[q] = rowr.get(q, 0) - f * w
            for b in B:
                if b[c] != 0:
                    b[r] -= f * b[c]
    X = []
    for b in B:
        x = [mp.mpf(0)] * n
        for r in range(n - 1, -1, -1):
            s = b[r]
            for q, w in A[r].items():
                if q != r:
                    s -= w * x[q]
            x[r] = s / A[r][r]
        X.append(x)
    return X


def exact_solve(times, wp, states, K):
    """times [M+1] and wp [M+1, 4] float64 (taken exactly); states: list of (start, end), each [4, K-1] float64 or
    None (rest).  Returns one float64 array [M, 4, 2K] per entry of `states`: the 60-digit solutions rounded once."""
    t = [mp.mpf(float(x)) for x in times]
    assert t[0] == 0
    return solve_checked(t, wp, states, K, None)


def solve_checked(t, wp, states, K, t_start):
    """exact_solve's body for knot times t given as mpf: assembly (start rows of segment 0 at local time t_start, see
    _assemble), the banded LU, the residual assertion against the unfactored rows, one rounding to float64"""
    NC = 2 * K
    M = len(t) - 1
    T = [t[i + 1] - t[i] for i in range(M)]
    n = NC * M
    rows, src = _assemble(T, K, t_start)
    assert len(rows) == n
    rhs = []
    for start, end in states:
        for a in range(4):
            col = []
            for s in src:
                if s is None:
                    col.append(mp.mpf(0))
                elif s[0] == "w":
                    col.append(mp.mpf(float(wp[s[1], a])))
                else:
                    blk = start if s[0] == "s" else end
                    col.append(mp.mpf(0) if blk is None else mp.mpf(float(blk[a, s[1] - 1])))
            rhs.append(col)
    X = _banded_lu_solve(rows, rhs, n, NC)
    # the solutions against the unfactored rows
    rows0, _ = _assemble(T, K, t_start)
    for x, col in zip(X, rhs):
        scale = max(abs(v) for v in x) + 1
        for (lo, vals), want in zip(rows0, col):
            got = sum((v * x[lo + q] for q, v in enumerate(vals) if v != 0), mp.mpf(0))
            assert abs(got - want) <= scale * mp.mpf(10) ** -45, "residual"
    out = []
    for k in range(len(states)):
        c = np.empty((M, 4, NC))
        for a in range(4):
            x = X[4 * k + a]
            for s in range(M):
                for q in range(NC):
                    c[s, a, q] = float(x[NC * s + q])
        out.append(c)
    return out


def exact_batch(wp, t, start, end, K):
    """wp [N, M+1, 4], t [N, M+1] or [M+1], start / end [N, 4, K-1] or None -> coef [N, M, 4, 2K]"""
    N = wp.shape[0]
    out = np.empty((N, wp.shape[1] - 1, 4, 2 * K))
    for d in range(N):
        tt = t if t.ndim == 1 else t[d]
        out[d] = exact_solve(tt, wp[d], [(None if start is None else start[d], None if end is None else end[d])], K)[0]
    return out


def hermite_two_point(T, w0, w1, s0, s1, K):
    """Closed form of the degree-(2K-1) polynomial with value and derivatives 1..K-1 given at 0 and T (two-point Taylor
    interpolation): with s = t / T,
        p = sum_q a_q T^q s^q / q! (1-s)^K sum_{j <= K-1-q} C(K-1+j, j) s^j
          + sum_q b_q (-T)^q (1-s)^q / q! s^K sum_{j <= K-1-q} C(K-1+j, j) (1-s)^j
    a = (w0, s0...), b = (w1, s1...).  Returns the 2K monomial coefficients in t as mpf."""
    NC = 2 * K
    T = mp.mpf(float(T))
    a = [mp.mpf(float(w0))] + [mp.mpf(float(v)) for v in s0]
    b = [mp.mpf(float(w1))] + [mp.mpf(float(v)) for v in s1]

    def mul(p, q):
        r = [mp.mpf(0)] * (len(p) + len(q) - 1)
        for i, x in enumerate(p):
            for j, y in enumerate(q):
                r[i + j] += x * y
        return r

    def power(p, e):
        r = [mp.mpf(1)]
        for _ in range(e):
            r = mul(r, p)
        return r

    s_, one_minus = [mp.mpf(0), mp.mpf(1)], [mp.mpf(1), mp.mpf(-1)]
    total = [mp.mpf(0)] * (NC + 1)
    for q in range(K):
        tail_s = [mp.binomial(K - 1 + j, j) for j in range(K - q)]                       # in s
        tail_m = [mp.mpf(0)]
        for j in range(K - q):
            term = [mp.binomial(K - 1 + j, j) * v for v in power(one_minus, j)]
            tail_m = [x + y for x, y in zip(tail_m + [mp.mpf(0)] * (len(term) - len(tail_m)), term)]
        pa = mul(mul(power(s_, q), power(one_minus, K)), tail_s)
        pb = mul(mul(power(one_minus, q), power(s_, K)), tail_m)
        fa = a[q] * T ** q / mp.factorial(q)
        fb = b[q] * (-T) ** q / mp.factorial(q)
        for i, v in enumerate(pa):
            total[i] += fa * v
        for i, v in enumerate(pb):
            total[i] += fb * v
    assert abs(total[NC]) < mp.mpf(10) ** -40
    return [total[i] / T ** i for i in range(NC)]


def eval_state_np(coef, dur, tq):
    """msnap_eval_state in NumPy: coef [N, M, 4, NC], dur [N, M], tq [N] -> pos [N, 4], deriv [N, 4, NC/2 - 1].
    msnap_eval_flat's lookup (first segment with t <= acc + T_i, the sums accumulated one by one), each derivative's
    coefficients (i + 1) * previous[i + 1], Horner with a separate multiply and add."""
    coef = np.asarray(coef, dtype=np.float64)
    dur = np.asarray(dur, dtype=np.float64)
    tq = np.asarray(tq, dtype=np.float64)
    N, M, _, NC = coef.shape
    ND = NC // 2 - 1
    pos = np.full((N, 4), np.nan)
    deriv = np.full((N, 4, ND), np.nan)
    for d in range(N):
        t = tq[d]
        acc, seg = np.float64(0.0), -1
        for i in range(M):
            if t <= acc + dur[d, i]:
                seg = i
                break
            acc = acc + dur[d, i]
        if not (t >= 0.0) or seg < 0:
            continue
        tl = t - acc
        for a in range(4):
            dd = coef[d, seg, a].copy()
            for q in range(ND + 1):
                if q:
                    dd = np.array([np.float64(i + 1) * dd[i + 1] for i in range(len(dd) - 1)])
                p = np.float64(0.0)
                for i in range(len(dd) - 1, -1, -1):
                    p = p * tl + dd[i]
                if q == 0:
                    pos[d, a] = p
                else:
                    deriv[d, a, q - 1] = p
    return pos, deriv


def eval_state_mp(coef_seg, tl, q):
    """q-th derivative of one axis' polynomial (float64 coefficients taken exactly) at local time tl, as mpf"""
    tl = mp.mpf(float(tl))
    return sum((falling(j, q) * mp.mpf(float(coef_seg[j])) * tl ** (j - q) for j in range(q, len(coef_seg))), mp.mpf(0))


# ---------------------------------------------------------------------------
# the cases of tests/test_states_gpu.py and their exact solutions
# ---------------------------------------------------------------------------
MAX_SEG = {7: 47, 9: 32}           # msnap_solve_states_max_segments (tests/test_states_cpu.py holds the library to it)
N_CASE = 17                        # one full 16-drone tile and a partial one
STATE_SCALE = (2.0, 2.0, 4.0, 8.0)   # |v| <= 2, |a| <= 2, |j| <= 4, |s| <= 8
COMBOS = ("start", "end", "both")


def case(order, M, N=N_CASE):
    """Seeded inputs: durations uniform in [0.5, 2] s, waypoint steps in [-2, 2] m, states within STATE_SCALE.
    Returns wp [N, M+1, 4], t [N, M+1], start, end [N, 4, K-1]."""
    K = (order + 1) // 2
    rng = np.random.default_rng(130000 + 100 * order + M)
    dur = rng.uniform(0.5, 2.0, (N, M))
    t = np.concatenate([np.zeros((N, 1)), np.cumsum(dur, axis=1)], axis=1)
    wp = np.cumsum(rng.uniform(-2.0, 2.0, (N, M + 1, 4)), axis=1)
    scale = np.array(STATE_SCALE[:K - 1])
    start = rng.uniform(-1.0, 1.0, (N, 4, K - 1)) * scale
    end = rng.uniform(-1.0, 1.0, (N, 4, K - 1)) * scale
    return wp, t, start, end


def combo_states(combo, start, end):
    return (start if combo in ("start", "both") else None, end if combo in ("end", "both") else None)


def golden_path(order):
    """The longest case of each order is recorded (about 8 s of mpmath each); one file per order keeps each under the
    size limit of a committed file."""
    import os
    name = "states_golden.npz" if order == 7 else "states_golden_order9.npz"
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)


_REF = {}


def reference(order, M):
    """{combo: coef [N, M, 4, 2K]} for case(order, M): computed here, or read from the recorded file for the longest"""
    key = (order, M)
    if key in _REF:
        return _REF[key]
    K = (order + 1) // 2
    wp, t, start, end = case(order, M)
    if M == MAX_SEG[order]:
        g = np.load(golden_path(order))
        for name, arr in (("wp", wp), ("t", t), ("start", start), ("end", end)):
            assert np.array_equal(g[name], arr), f"{golden_path(order)} was recorded for other inputs ({name})"
        ref = {c: g["coef_" + c] for c in COMBOS}
    else:
        ref = {c: np.empty((wp.shape[0], M, 4, 2 * K)) for c in COMBOS}
        for d in range(wp.shape[0]):
            sols = exact_solve(t[d], wp[d], [combo_states(c, start[d], end[d]) for c in COMBOS], K)
            for c, s in zip(COMBOS, sols):
                ref[c][d] = s
    _REF[key] = ref
    return ref
