"""The painted map (include/ptudes_mi.h ptl_paint_*) restated in Python, sharing no code with the library.

The definition: a ray is a pixel with a return, its end w the posed world point ((R0 p0 + R1 p1) + R2 p2) + t of its column's pose.  Its voxel
is the truncating index (int)(coordinate / vs) per axis; a w outside the key range (2^20 voxels either side, or not finite) makes the ray
unmatched.  For every stored point p of that voxel with p.x == w.x and p.y == w.y and p.z == w.z (doubles): sum[p] += field[pixel],
count[p] += 1.  A ray with at least one such point is matched, every other ray unmatched; a pixel without a return is counted in n_no_return
and adds nothing; a skipped sweep (None) is counted and adds nothing.  Everything is an integer.

Three forms, checked against each other by tests/test_map_paint_cpu.py (paint_arrays, for sweeps of 10^5 rays, is further down):
  paint        a dict from voxel index to the stored points of that voxel, then the comparison of the three doubles
  paint_brute  every ray against every stored point in Python scalars: equal coordinates lie in one voxel, so no voxel is needed - only the key
               range of the ray's own end
Both take the map's STORED points as given (the device's `map_points()` / the returned xyz: which points a voxel kept is the map's business).
Sums and counts come back in the order of the stored points handed in."""
import math

import numpy as np

KEY_OFF = 1 << 20
COUNTS = ("n_points", "n_points_painted", "n_scans", "n_scans_skipped", "n_rays_matched", "n_rays_unmatched", "n_no_return", "sum_count")


def rays_of_sweep(p_sensor, has_return, col_poses, field):
    """p_sensor (H, W, 3) f64, has_return (H, W), col_poses (W, 4, 4), field (H, W): (w, ret, value) per pixel in row-major order"""
    p = np.asarray(p_sensor, dtype=np.float64)
    H, W = p.shape[:2]
    M = np.asarray(col_poses, dtype=np.float64)
    R, t = M[None, :, :3, :3], M[None, :, :3, 3]
    w = np.empty((H, W, 3))
    for k in range(3):
        w[..., k] = ((R[..., k, 0] * p[..., 0] + R[..., k, 1] * p[..., 1]) + R[..., k, 2] * p[..., 2]) + t[..., k]
    return w.reshape(-1, 3), np.asarray(has_return, dtype=bool).reshape(-1), np.asarray(field, dtype=np.uint32).reshape(-1)


def key_of(s, vs):
    """the map's truncating voxel index of one point, or None outside the key range / for a non-finite coordinate"""
    k = []
    for c in s:
        if not math.isfinite(c):
            return None
        q = c / vs
        if not abs(q) < 1.1e6:
            return None
        i = int(q)  # (truncates toward zero)
        if not -KEY_OFF <= i < KEY_OFF:
            return None
        k.append(i)
    return tuple(k)


def _close(n, stored, count):
    n["n_points"] = len(stored)
    n["n_points_painted"] = int((count > 0).sum())
    n["sum_count"] = int(count.astype(np.int64).sum())


def paint(stored, sweeps, vs):
    """sweeps: [(w, ret, value) or None for a skipped sweep].  Returns (sum uint64, count uint32, counts)"""
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    P = [tuple(float(x) for x in p) for p in stored]
    vox = {}
    for i, p in enumerate(P):
        vox.setdefault(key_of(p, vs), []).append(i)
    total, count = [0] * len(P), np.zeros(len(P), dtype=np.uint32)
    n = dict.fromkeys(COUNTS, 0)
    for sw in sweeps:
        if sw is None:
            n["n_scans_skipped"] += 1
            continue
        n["n_scans"] += 1
        for w, ret, value in zip(*sw):
            if not ret:
                n["n_no_return"] += 1
                continue
            w = tuple(float(x) for x in w)
            key = key_of(w, vs)
            hit = False
            if key is not None:
                for i in vox.get(key, ()):
                    if P[i][0] == w[0] and P[i][1] == w[1] and P[i][2] == w[2]:
                        total[i] += int(value)
                        count[i] += 1
                        hit = True
            n["n_rays_matched" if hit else "n_rays_unmatched"] += 1
    _close(n, stored, count)
    return np.array(total, dtype=np.uint64).reshape(-1), count, n


def paint_brute(stored, sweeps, vs):
    """the same function: every ray against every stored point"""
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    P = [[float(x) for x in p] for p in stored]
    total, count = [0] * len(P), [0] * len(P)
    n = dict.fromkeys(COUNTS, 0)
    for sw in sweeps:
        if sw is None:
            n["n_scans_skipped"] += 1
            continue
        n["n_scans"] += 1
        for w, ret, value in zip(*sw):
            if not ret:
                n["n_no_return"] += 1
                continue
            x, y, z = float(w[0]), float(w[1]), float(w[2])
            hit = False
            if key_of((x, y, z), vs) is not None:
                for i, p in enumerate(P):
                    if p[0] == x and p[1] == y and p[2] == z:
                        total[i] += int(value)
                        count[i] += 1
                        hit = True
            if hit:
                n["n_rays_matched"] += 1
            else:
                n["n_rays_unmatched"] += 1
    count = np.array(count, dtype=np.uint32).reshape(-1)
    _close(n, stored, count)
    return np.array(total, dtype=np.uint64).reshape(-1), count, n


def paint_arrays(stored, sweeps, vs):
    """the same function for sweeps of 10^5 rays: equal coordinates are found by sorting the points as rows (`paint` and `paint_brute` are
    what it is checked against).  Zeros are brought to one sign first: -0.0 == 0.0, and a sort of the rows' bytes would keep them apart"""
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3) + 0.0
    if len(stored):
        uniq, group = np.unique(stored, axis=0, return_inverse=True)
    else:
        uniq, group = stored, np.zeros(0, dtype=np.int64)
    group = np.asarray(group, dtype=np.int64).reshape(-1)  # the row of `uniq` each stored point equals
    total, count = np.zeros(len(uniq), dtype=np.uint64), np.zeros(len(uniq), dtype=np.int64)  # (u32 values: exact below 2^32 rays per point)
    n = dict.fromkeys(COUNTS, 0)
    for sw in sweeps:
        if sw is None:
            n["n_scans_skipped"] += 1
            continue
        n["n_scans"] += 1
        w, ret, value = (np.asarray(a) for a in sw)
        n["n_no_return"] += int((~ret).sum())
        w, value = w[ret] + 0.0, value[ret].astype(np.uint64)
        with np.errstate(invalid="ignore", over="ignore"):
            q = w / vs
            ok = np.isfinite(w).all(axis=1) & (np.abs(q) < 1.1e6).all(axis=1)
            k = np.trunc(np.where(ok[:, None], q, 0.0)).astype(np.int64)
        ok &= ((k >= -KEY_OFF) & (k < KEY_OFF)).all(axis=1)
        hit = np.zeros(len(w), dtype=bool)
        at = np.zeros(len(w), dtype=np.int64)
        if len(uniq):
            # the row of `uniq` each ray's end equals, -1 for none: the distinct rows of both sets, numbered once
            both =np.concatenate([uniq, w])
            _, inv = np.unique(both, axis=0, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
            where = np.full(inv.max() + 1, -1, dtype=np.int64)
            where[inv[:len(uniq)]] = np.arange(len(uniq))
            at = where[inv[len(uniq):]]
            hit = ok & (at >= 0)
        n["n_rays_matched"] += int(hit.sum())
        n["n_rays_unmatched"] += int((~hit).sum())
        np.add.at(count, at[hit], 1)
        np.add.at(total, at[hit], value[hit])
    per_sum = total[group]
    per_count = count[group].astype(np.uint32)
    _close(n, stored, per_count)
    return per_sum, per_count, n


def sorted_rows(xyz, total, count):
    """rows (x, y, z, sum, count) in lexicographic order of the point: the pool order of the device's arrays is unspecified.  The sum stays an
    exact integer (object rows would be slow; a u64 sum below 2^53 is exact in a double, larger ones are split into two 32-bit halves)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    total = np.asarray(total, dtype=np.uint64).reshape(-1)
    rows = np.column_stack([xyz, (total >> np.uint64(32)).astype(np.float64), (total & np.uint64(0xffffffff)).astype(np.float64),
                            np.asarray(count, dtype=np.float64).reshape(-1)])
    return rows[np.lexsort(rows.T[::-1])]


def first_points_per_voxel(points, vs, P):
    """the points a voxel map keeps of `points` handed in in this order: the first P of every voxel (points outside the key range: none)"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    seen, keep = {}, np.zeros(len(pts), dtype=bool)
    for i, p in enumerate(pts):
        k = key_of([float(x) for x in p], vs)
        if k is None:
            continue
        c = seen.get(k, 0)
        if c < P:
            seen[k] = c + 1
            keep[i] = True
    return pts[keep]
