"""The map score in numpy, restated from its definition (include/ptudes_mi.h) - no GPU, no code shared with the kernels.

Per point q of a cloud of stored points:
  membership   p (q included) is a neighbour iff (dx dx + dy dy) + dz dz <= radius radius with d = p - q, evaluated in that order;
  covariance   n neighbours, m = mean of the offsets d, Sigma = (1/n) sum d d^T - m m^T in fp64;
  eigenvalues  of Sigma by cyclic Jacobi, a fixed number of sweeps, ascending, clipped below at 0;
  outputs      plane_var = lambda0, entropy = 0.5 (3 ln(2 pi e) + sum ln(lambda_i + sigma_floor^2));
  sparse       n < min_neighbours: n and two NaNs.
Candidates come from a uniform grid of cells a shade larger than the radius (27 cells per point); the membership test is the expression above.
"""
import numpy as np

SWEEPS = 8
LN_2PI_E = 1.0 + np.log(2.0 * np.pi)


def neighbour_pairs(pts, radius):
    """(i, j): every ordered pair with point j a neighbour of point i (i == j included), grouped by i"""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cell = np.floor(pts / (radius * (1.0 + 1e-9))).astype(np.int64)  # |d| <= radius: the cell indices differ by at most one
    cell -= cell.min(axis=0)
    dims = cell.max(axis=0) + 3  # one empty layer either side
    key = ((cell[:, 0] + 1) * dims[1] + (cell[:, 1] + 1)) * dims[2] + (cell[:, 2] + 1)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    r2 = radius * radius
    out_i, out_j = [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                want = key + (ox * dims[1] + oy) * dims[2] + oz
                lo, hi = np.searchsorted(skey, want, "left"), np.searchsorted(skey, want, "right")
                cnt = hi - lo
                total = int(cnt.sum())
                if total == 0:
                    continue
                i = np.repeat(np.arange(n), cnt)
                start = np.repeat(np.cumsum(cnt) - cnt, cnt)
                j = order[np.repeat(lo, cnt) + (np.arange(total) - start)]
                d = pts[j] - pts[i]
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                keep = d2 <= r2
                out_i.append(i[keep])
                out_j.append(j[keep])
    i, j = np.concatenate(out_i), np.concatenate(out_j)
    o = np.argsort(i, kind="stable")
    return i[o], j[o]


def _rotate(app, aqq, apq, arp, arq):
    """one Jacobi rotation that zeroes a_pq, for arrays of matrices; r is the third index"""
    live = apq != 0.0
    safe = np.where(live, apq, 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        theta = (aqq - app) / (2.0 * safe)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    t = np.where(live, t, 0.0)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    return app - t * apq, aqq + t * apq, np.where(live, 0.0, apq), c * arp - s * arq, s * arp + c * arq


def jacobi_eigenvalues(a00, a01, a02, a11, a12, a22):
    """eigenvalues (N, 3), ascending, clipped below at 0, of N symmetric 3 x 3 matrices: cyclic Jacobi, SWEEPS sweeps"""
    a00, a01, a02, a11, a12, a22 = (np.array(x, dtype=np.float64, ndmin=1) for x in (a00, a01, a02, a11, a12, a22))
    for _ in range(SWEEPS):
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02)
    lam = np.sort(np.stack([a00, a11, a22], axis=1), axis=1)
    return np.maximum(lam, 0.0)


def score_points(pts, radius, min_neighbours=5, sigma_floor=None):
    """(n int64 (N,), plane_var (N,), entropy (N,), eigenvalues (N, 3)) of every point; sparse points: NaN"""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    N = len(pts)
    if sigma_floor is None:
        sigma_floor = radius / 100.0
    i, j = neighbour_pairs(pts, radius)
    d = pts[j] - pts[i]
    n = np.bincount(i, minlength=N).astype(np.int64)
    nn = np.maximum(n, 1).astype(np.float64)

    def mean_of(w):
        return np.bincount(i, weights=w, minlength=N) / nn

    m = np.stack([mean_of(d[:, k]) for k in range(3)], axis=1)
    cov = {}
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        cov[a, b] = mean_of(d[:, a] * d[:, b]) - m[:, a] * m[:, b]
    lam = jacobi_eigenvalues(cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2])
    f2 = sigma_floor * sigma_floor
    ent = 0.5 * (3.0 * LN_2PI_E + ((np.log(lam[:, 0] + f2) + np.log(lam[:, 1] + f2)) + np.log(lam[:, 2] + f2)))
    pv = lam[:, 0].copy()
    sparse = n < min_neighbours
    pv[sparse] = np.nan
    ent[sparse] = np.nan
    lam = lam.copy()
    lam[sparse] = np.nan
    return n, pv, ent, lam


def summary(n, plane_var, entropy, min_neighbours=5):
    """the summary of the per-point values: counts, the means over the scored points (0 when there is none), mean neighbours over all"""
    n = np.asarray(n)
    scored = n >= min_neighbours
    k = int(scored.sum())
    return dict(n_points=len(n), n_scored=k, n_sparse=len(n) - k,
                mean_plane_var=float(np.mean(plane_var[scored])) if k else 0.0,
                mean_entropy=float(np.mean(entropy[scored])) if k else 0.0,
                mean_neighbours=float(np.mean(n)) if len(n) else 0.0)
