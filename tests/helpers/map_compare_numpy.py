"""The map distance (include/ptudes_mi.h ptl_icp_map_distance) restated in numpy, independently of the device code: brute
force over ALL stored points - no voxels, no 27-voxel neighbourhood.  That the device's neighbourhood search loses nothing is therefore what a
comparison with this file checks.

Per query q and reference points p (the map's stored points):
  d2(q) = min over p of (dx dx + dy dy) + dz dz, d = p - q, fp64 in this order (numpy evaluates element-wise: no contraction);
  matched iff d2 <= max_dist * max_dist (one product, a double); the per-point value is d2 when matched, +inf when not;
  a query with a non-finite coordinate is invalid: NaN;
  a query whose voxel index trunc(q / vs) lies outside [-2^20, 2^20) on an axis is unmatched;
  n_within[k] = number of queries with d2 <= thr_k * thr_k.
"""
import numpy as np

KEY_OFF = 1 << 20


def dist2(queries, ref_points, voxel_size, max_dist, block=2048):
    """per-point values (N,) of `queries` (N, 3) against `ref_points` (M, 3)"""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(ref_points, dtype=np.float64).reshape(-1, 3)
    max2 = np.float64(max_dist) * np.float64(max_dist)
    out = np.full(len(q), np.inf)
    finite = np.isfinite(q).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.trunc(np.where(finite[:, None], q, 0.0) / np.float64(voxel_size))
    in_keys = ((k >= -KEY_OFF) & (k < KEY_OFF)).all(axis=1)
    todo = np.flatnonzero(finite & in_keys)
    if len(p):
        for lo in range(0, len(todo), block):
            idx = todo[lo:lo + block]
            d = p[None, :, :] - q[idx, None, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            best = d2.min(axis=1)
            out[idx] = np.where(best <= max2, best, np.inf)
    out[~finite] = np.nan
    return out


def summary(d2, max_dist, thresholds):
    """the counts (exact) and the sums over the matched queries, added in query order"""
    d2 = np.asarray(d2, dtype=np.float64)
    matched = d2 <= np.float64(max_dist) * np.float64(max_dist)  # (NaN and +inf compare false)
    m = d2[matched]
    return dict(n_query=len(d2), n_invalid=int(np.isnan(d2).sum()), n_matched=int(matched.sum()),
                n_within=tuple(int((d2 <= np.float64(t) * np.float64(t)).sum()) for t in thresholds),
                sum_dist=float(np.sqrt(m).sum()), sum_dist2=float(m.sum()), max_dist2_seen=float(m.max()) if len(m) else 0.0)


def f_scores(acc, com):
    """(precision, recall, F) per threshold of two summaries: map -> reference and reference -> map"""
    out = []
    for a, c in zip(acc["n_within"], com["n_within"]):
        p = a / acc["n_query"] if acc["n_query"] else 0.0
        r = c / com["n_query"] if com["n_query"] else 0.0
        out.append((p, r, 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0))
    return out
