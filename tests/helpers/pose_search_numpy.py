"""The pose search's hit counts (include/ptudes_mi.h ptl_icp_pose_hits) restated in numpy, independently of the device code.

Per candidate T (4 x 4, the top three rows as given) and query point q (sensor frame):
  wx = ((T00 qx + T01 qy) + T02 qz) + T03, wy and wz likewise - numpy evaluates element-wise, every operation rounds on its own;
  d2(w) = the map distance of tests/helpers/map_compare_numpy.py (brute force over ALL stored points, no voxels), called as it is;
  hits[k][j] = number of points with d2 <= thr_j * thr_j (NaN and +inf compare false: a non-finite or out-of-range w is no hit);
  a candidate with a non-finite entry in its top three rows: hits = -1 at every threshold, no probe;
  best per threshold: the largest count over the valid candidates and the smallest index that attains it; none valid: index -1, hits 0.

`dist2_near` is the same per-point value for scenes too large for the brute force (a sweep against a map of 10^5 points): a k-d tree hands
over, per query, the stored points within max_dist (1 + 2^-20) - a superset of every point that can be within max_dist under the rounded
expression, whose relative error is a few 2^-53 - and the written-order expression then takes the exact minimum over those.  What the tree
leaves out cannot change a value <= max_dist^2, and every other value is +inf on both paths.  The CPU test holds the two paths against each
other on the small scenes."""
import numpy as np

from tests.helpers import map_compare_numpy as mc


def transform(points, pose):
    """(N, 3) world points of `points` (N, 3) under `pose` (4 x 4), the written order"""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def dist2_near(queries, ref_points, voxel_size, max_dist):
    """mc.dist2 through a k-d tree's neighbour lists (see above)"""
    from scipy.spatial import cKDTree
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(ref_points, dtype=np.float64).reshape(-1, 3)
    max2 = np.float64(max_dist) * np.float64(max_dist)
    out = np.full(len(q), np.inf)
    finite = np.isfinite(q).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.trunc(np.where(finite[:, None], q, 0.0) / np.float64(voxel_size))
    in_keys = ((k >= -mc.KEY_OFF) & (k < mc.KEY_OFF)).all(axis=1)
    todo = np.flatnonzero(finite & in_keys)
    if len(p) and len(todo):
        lists = cKDTree(p).query_ball_point(q[todo], float(max_dist) * (1.0 + 2.0 ** -20))
        lens = np.fromiter((len(l) for l in lists), dtype=np.int64, count=len(lists))
        if lens.sum():
            flat = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists if len(l)])
            qi = np.repeat(np.arange(len(todo)), lens)
            d = p[flat] - q[todo][qi]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            best = np.full(len(todo), np.inf)
            np.minimum.at(best, qi, d2)
            out[todo] = np.where(best <= max2, best, np.inf)
    out[~finite] = np.nan
    return out


def pose_valid(poses):
    """(K,) bool: every entry of the top three rows is finite"""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    return np.isfinite(P[:, :3, :]).all(axis=(1, 2))


def hits(points, poses, ref_points, voxel_size, max_dist, thresholds, near=False):
    """(K, T) int32 hit counts; near: per-point values by `dist2_near` instead of the brute force"""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    thr2 = [np.float64(t) * np.float64(t) for t in thresholds]
    out = np.full((len(P), len(thr2)), -1, dtype=np.int32)
    fn = dist2_near if near else mc.dist2
    for k in np.flatnonzero(pose_valid(P)):
        d2 = fn(transform(q, P[k]), ref_points, voxel_size, max_dist)
        out[k] = [int((d2 <= t).sum()) for t in thr2]
    return out


def summary(points, poses, hits_kt):
    """the counts of the result struct and the best candidate per threshold"""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    h = np.asarray(hits_kt)
    best_pose, best_hits = [], []
    for j in range(h.shape[1]):
        col = h[:, j]
        if len(col) and col.max() >= 0:
            best_hits.append(int(col.max()))
            best_pose.append(int(np.flatnonzero(col == col.max())[0]))
        else:
            best_hits.append(0)
            best_pose.append(-1)
    return dict(n_points=len(q), n_invalid_points=int((~np.isfinite(q).all(axis=1)).sum()), n_poses=len(h),
                n_invalid_poses=int((~pose_valid(poses)).sum()) if len(h) else 0, best_pose=tuple(best_pose), best_hits=tuple(best_hits))
