"""NumPy reference of msnap_formation_near_pairs (include/msnap.h, "near pairs").

d2_ij is the plain sum of squares dx dx + dy dy + dz dz (the library forms fma(dz, dz, fma(dy, dy, dx dx)): both are
sums of three non-negative terms and differ by a few ulp at most), minimised over the samples with the minNum rule; the
limit is formed with the contract's operation order; pairs are kept by the strict compare and listed lexicographically.
A pair so close to its limit that the two forms of d2 could decide it differently is in the BAND:
|sqrt(d2) - lim| <= 1e-14 lim (about 45 ulp).  A test that compares lists asserts the band empty for its input."""
import warnings

import numpy as np

BAND_REL = 1e-14
DIST_ULPS = 8          # pair_dist against the reference: 8 ulp = 1.8e-15 relative


def all_d2(pos):
    """[N, N] squared sampled distances (+inf where a pair has no sample at which both drones are finite)."""
    pos = np.asarray(pos, dtype=np.float64)
    N = pos.shape[0]
    out = np.full((N, N), np.inf)
    with np.errstate(invalid="ignore", over="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for i in range(N):
            d = pos[i][None] - pos                                   # [N, S, 3]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            d2 = np.where(np.isnan(d2), np.inf, d2)                  # minNum: a non-finite sample never wins
            out[i] = d2.min(axis=1) if d2.shape[1] else np.inf
    return out


def limits(n, base, speed=None, gap=0.0, margin=0.0):
    v = np.zeros(n) if speed is None else np.asarray(speed, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float64(base) + (v[:, None] + v[None, :]) * np.float64(gap)) * (np.float64(1.0) + np.float64(margin))


def near_pairs(pos, base, speed=None, gap=0.0, margin=0.0):
    """(pairs int32 [P, 2] ascending, dist [P], band: the list of (i, j) too close to their limit to call)."""
    pos = np.asarray(pos, dtype=np.float64)
    N = pos.shape[0]
    if N < 2:
        return np.zeros((0, 2), dtype=np.int32), np.zeros((0,)), []
    dist = np.sqrt(all_d2(pos))
    lim = limits(N, base, speed, gap, margin)
    upper = np.triu(np.ones((N, N), dtype=bool), 1)
    with np.errstate(invalid="ignore"):
        keep = (dist < lim) & upper
        band = (np.abs(dist - lim) <= BAND_REL * np.abs(lim)) & upper & np.isfinite(dist)
    ii, jj = np.nonzero(keep)                                        # row-major: ascending (i, j)
    return (np.stack([ii, jj], axis=1).astype(np.int32), dist[ii, jj], [tuple(p) for p in np.argwhere(band)])


def assert_matches(pairs, dist, pos, base, speed=None, gap=0.0, margin=0.0):
    """The library's full list against the reference: empty band, equal lists in order, distances within 8 ulp."""
    rp, rd, band = near_pairs(pos, base, speed, gap, margin)
    assert band == [], f"pairs within 1e-14 of their limit: choose another seed ({band[:4]})"
    assert pairs.dtype == np.int32 and pairs.shape == rp.shape, (pairs.shape, rp.shape)
    assert np.array_equal(pairs, rp)
    if dist is not None:
        assert dist.shape == rd.shape
        assert (np.abs(dist - rd) <= DIST_ULPS * np.spacing(rd)).all()
    return rp, rd


GAP = 0.05


def base_for(pos, speed=None, frac=0.03):
    """The base at which ceil(frac pairs) pairs (at least one) are kept with gap = GAP and margin ~ 0: midway between
    the last kept and the first dropped pair's dist - (v_i + v_j) GAP."""
    n = pos.shape[0]
    v = np.zeros(n) if speed is None else speed
    iu = np.triu_indices(n, 1)
    e = np.sort(np.sqrt(all_d2(pos))[iu] - (v[:, None] + v[None, :])[iu] * GAP)
    k = max(1, int(np.ceil(frac * len(e))))
    return float(e[k - 1] + 0.01 if k >= len(e) else 0.5 * (e[k - 1] + e[k]))


def box_swarm(seed, n, s):
    """Seeded random walks that start in a unit box, and speeds: (pos [n, s, 3], speed [n])."""
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 1, 3)) + 0.05 * np.cumsum(rng.standard_normal((n, s, 3)), axis=1) / np.sqrt(s)
    return pos, 0.2 * rng.random(n)
