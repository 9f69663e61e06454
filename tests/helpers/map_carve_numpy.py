"""The free-space carve (include/ptudes_mi.h ptl_carve_*) restated in numpy, sharing no code with the library.

Two forms of the one definition, checked against each other by tests/test_map_carve_cpu.py:
  carve_plain   ray by ray and sample by sample in Python floats (IEEE doubles, every operation rounded once), a dict for the voxels
  carve         the rays of a sweep in lockstep over the sample index (numpy arrays, the same operations element by element), a sorted key
                table for the voxels - for scenes of 10^5 rays
Both take the map's STORED points as given (the device's `map_points()`: which points a voxel kept is the map's business) and the rays as
(origin, end, has_return) per pixel; `rays_of_sweep` makes those from sensor-frame points and column poses with the posed-scan pass's product
((R0 p0 + R1 p1) + R2 p2) + t.  Votes come back in the order of the stored points handed in."""
import math

import numpy as np

KEY_OFF = 1 << 20
COUNTS = ("n_scans", "n_scans_skipped", "n_rays", "n_rays_out_of_range", "n_no_return", "n_voxel_visits", "n_points_through",
          "n_points_supported", "sum_through", "sum_support")


def defaults(vs):
    return dict(radius=vs / 10.0, margin=vs, step=vs / 2.0, min_range=0.0, max_range=120.0 * vs)


def dynamic(through, support, min_through=2, min_fraction=0.5):
    """the host policy, restated"""
    t, s = np.asarray(through, dtype=np.int64), np.asarray(support, dtype=np.int64)
    return (t >= min_through) & (t >= min_fraction * (t + s))


def rays_of_sweep(p_sensor, has_return, col_poses):
    """p_sensor (H, W, 3) f64, has_return (H, W), col_poses (W, 4, 4): (o, w, ret), each per pixel in row-major order"""
    p = np.asarray(p_sensor, dtype=np.float64)
    H, W = p.shape[:2]
    M = np.asarray(col_poses, dtype=np.float64)
    R, t = M[None, :, :3, :3], M[None, :, :3, 3]
    w = np.empty((H, W, 3))
    for k in range(3):
        w[..., k] = ((R[..., k, 0] * p[..., 0] + R[..., k, 1] * p[..., 1]) + R[..., k, 2] * p[..., 2]) + t[..., k]
    o = np.broadcast_to(t, (H, W, 3))
    return o.reshape(-1, 3).copy(), w.reshape(-1, 3), np.asarray(has_return, dtype=bool).reshape(-1)


# ---------------------------------------------------------------------------------------------- plain: Python floats, a dict
def key_of(s, vs):
    """the map's truncating voxel index of one point, or None outside the key range (2^20 voxels either side) / for a non-finite coordinate"""
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


def voxel_dict(stored, vs):
    vox = {}
    for i, p in enumerate(np.asarray(stored, dtype=np.float64)):
        vox.setdefault(key_of([float(x) for x in p], vs), []).append(i)
    return vox


def march_keys(o, w, vs, step, with_samples=False):
    """the voxels one used ray visits, in order (None entries are left out; consecutive equal keys once); with_samples: also every sample"""
    d = [w[c] - o[c] for c in range(3)]
    ln = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    keys, samples, prev, k = [], [], (False, None), 0
    while True:
        tk = (float(k) + 0.5) * step
        if tk < ln:
            ak = tk / ln
            s = [o[c] + ak * d[c] for c in range(3)]
        else:
            s = [w[0], w[1], w[2]]
        key = key_of(s, vs)
        samples.append(s)
        has = key is not None
        if has and not (prev[0] and prev[1] == key):
            keys.append(key)
        prev = (has, key)
        if not tk < ln:
            break
        k += 1
    return (keys, samples) if with_samples else keys


def vote(p, o, d, ln, rr, cfg):
    """0 nothing, 1 through, 2 support for one stored point against one ray"""
    ex, ey, ez = p[0] - o[0], p[1] - o[1], p[2] - o[2]
    cx, cy, cz = ey * d[2] - ez * d[1], ez * d[0] - ex * d[2], ex * d[1] - ey * d[0]
    if not (cx * cx + cy * cy) + cz * cz <= rr:
        return 0
    dot = (ex * d[0] + ey * d[1]) + ez * d[2]
    tp = dot / ln if ln != 0.0 else math.nan  # (0 / 0 on the device: NaN, every comparison false)
    if tp < cfg["min_range"]:
        return 0
    if tp <= ln - cfg["margin"]:
        return 1
    if tp <= ln + cfg["margin"]:
        return 2
    return 0


def carve_plain(stored, sweeps, vs, cfg):
    """sweeps: [(o, w, ret) or None for a skipped sweep].  Returns (through, support, counts)"""
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    vox = voxel_dict(stored, vs)
    P = [[float(x) for x in p] for p in stored]
    thr, sup = np.zeros(len(stored), dtype=np.uint32), np.zeros(len(stored), dtype=np.uint32)
    n = dict.fromkeys(COUNTS, 0)
    r2 = cfg["radius"] * cfg["radius"]
    for sw in sweeps:
        if sw is None:
            n["n_scans_skipped"] += 1
            continue
        n["n_scans"] += 1
        for o, w, ret in zip(*sw):
            if not ret:
                n["n_no_return"] += 1
                continue
            o, w = [float(x) for x in o], [float(x) for x in w]
            d = [w[c] - o[c] for c in range(3)]
            len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            ln = math.sqrt(len2) if len2 == len2 and len2 >= 0.0 else math.nan
            if not (ln >= cfg["min_range"] and ln <= cfg["max_range"]):
                n["n_rays_out_of_range"] += 1
                continue
            n["n_rays"] += 1
            rr = r2 * len2
            for key in march_keys(o, w, vs, cfg["step"]):
                ids = vox.get(key)
                if not ids:
                    continue
                n["n_voxel_visits"] += 1
                for i in ids:
                    v = vote(P[i], o, d, ln, rr, cfg)
                    if v == 1:
                        thr[i] += 1
                    elif v == 2:
                        sup[i] += 1
    _close(n, thr, sup)
    return thr, sup, n


def _close(n, thr, sup):
    n["n_points_through"], n["n_points_supported"] = int((thr > 0).sum()), int((sup > 0).sum())
    n["sum_through"], n["sum_support"] = int(thr.astype(np.int64).sum()), int(sup.astype(np.int64).sum())


# ---------------------------------------------------------------------------------------------- lockstep: arrays, a sorted key table
def _keys(s, vs):
    """packed keys (int64) of points (n, 3) and whether each has one"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = s / vs
        ok = np.isfinite(s).all(axis=1) & (np.abs(q) < 1.1e6).all(axis=1)
        k = np.trunc(np.where(ok[:, None], q, 0.0)).astype(np.int64)
    ok &= ((k >= -KEY_OFF) & (k < KEY_OFF)).all(axis=1)
    k = np.where(ok[:, None], k, 0) + KEY_OFF
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2], ok


def carve(stored, sweeps, vs, cfg):
    """the same function as carve_plain"""
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    thr, sup = np.zeros(len(stored), dtype=np.int64), np.zeros(len(stored), dtype=np.int64)
    n = dict.fromkeys(COUNTS, 0)
    skeys, sok = _keys(stored, vs)
    assert sok.all(), "a stored point outside the key range"
    order = np.argsort(skeys, kind="stable")
    ukeys, starts, counts = np.unique(skeys[order], return_index=True, return_counts=True)
    r2 = cfg["radius"] * cfg["radius"]
    step, margin, min_range = cfg["step"], cfg["margin"], cfg["min_range"]
    for sw in sweeps:
        if sw is None:
            n["n_scans_skipped"] += 1
            continue
        n["n_scans"] += 1
        o, w, ret = (np.asarray(a) for a in sw)
        with np.errstate(invalid="ignore", over="ignore"):
            d = w - o
            len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            ln = np.sqrt(len2)
            used = ret & (ln >= min_range) & (ln <= cfg["max_range"])
        n["n_no_return"] += int((~ret).sum())
        n["n_rays_out_of_range"] += int((ret & ~used).sum())
        n["n_rays"] += int(used.sum())
        o, w, d, ln, len2 = o[used], w[used], d[used], ln[used], len2[used]
        rr = r2 * len2
        t_thr, t_sup = ln - margin, ln + margin
        live = np.arange(len(o))
        prev_key, prev_has = np.zeros(len(o), dtype=np.int64), np.zeros(len(o), dtype=bool)
        k = 0
        while len(live):
            tk = (float(k) + 0.5) * step
            in_k = tk < ln[live]
            with np.errstate(invalid="ignore", divide="ignore"):
                ak = tk / ln[live]
                s = o[live] + ak[:, None] * d[live]
            s = np.where(in_k[:, None], s, w[live])
            key, has = _keys(s, vs)
            new = has & ~(prev_has[live] & (prev_key[live] == key))
            prev_key[live], prev_has[live] = key, has
            if len(ukeys) and new.any():
                rays, kk = live[new], key[new]
                at = np.minimum(np.searchsorted(ukeys, kk), len(ukeys) - 1)
                hit = ukeys[at] == kk
                rays, at = rays[hit], at[hit]
                n["n_voxel_visits"] += len(rays)
                if len(rays):
                    cnt = counts[at]
                    rr_ = np.repeat(rays, cnt)
                    within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                    pid = order[np.repeat(starts[at], cnt) + within]
                    e = stored[pid] - o[rr_]
                    dd = d[rr_]
                    cx = e[:, 1] * dd[:, 2] - e[:, 2] * dd[:, 1]
                    cy = e[:, 2] * dd[:, 0] - e[:, 0] * dd[:, 2]
                    cz = e[:, 0] * dd[:, 1] - e[:, 1] * dd[:, 0]
                    near = (cx * cx + cy * cy) + cz * cz <= rr[rr_]
                    with np.errstate(invalid="ignore", divide="ignore"):
                        tp = ((e[:, 0] * dd[:, 0] + e[:, 1] * dd[:, 1]) + e[:, 2] * dd[:, 2]) / ln[rr_]
                        far_enough = near & ~(tp < min_range)
                        through = far_enough & (tp <= t_thr[rr_])
                        support = far_enough & ~through & (tp <= t_sup[rr_])
                    np.add.at(thr, pid[through], 1)
                    np.add.at(sup, pid[support], 1)
            live = live[in_k]
            k += 1
    thr, sup = thr.astype(np.uint32), sup.astype(np.uint32)
    _close(n, thr, sup)
    return thr, sup, n


def sorted_rows(xyz, through, support):
    """rows (x, y, z, through, support) in lexicographic order: the pool order of the device's arrays is unspecified"""
    rows = np.column_stack([np.asarray(xyz, dtype=np.float64), np.asarray(through, dtype=np.float64), np.asarray(support, dtype=np.float64)])
    return rows[np.lexsort(rows.T[::-1])]


# ---------------------------------------------------------------------------------------------- the map's rule, for scenes without a device
def first_points_per_voxel(points, vs, P):
    """the points a voxel map keeps of `points` handed in in this order: the first P of every voxel"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    keys, ok = _keys(pts, vs)
    seen, keep = {}, np.zeros(len(pts), dtype=bool)
    for i, (k, good) in enumerate(zip(keys.tolist(), ok.tolist())):
        if not good:
            continue
        c = seen.get(k, 0)
        if c < P:
            seen[k] = c + 1
            keep[i] = True
    return pts[keep]


# ---------------------------------------------------------------------------------------------- the moving-box scene
ROOM = ((-10.0, -8.0, 0.0), (10.0, 8.0, 5.0))
BOX_SIZE = (0.6, 0.6, 1.8)
BOX_CFG = dict(radius=0.05, margin=0.5, step=0.25, min_range=0.0, max_range=60.0)
BOX_VS, BOX_P = 0.5, 20


def _slab(o, u, lo, hi):
    """entry and exit parameters of rays o + t u against the box [lo, hi]"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (np.asarray(lo) - o) / u, (np.asarray(hi) - o) / u
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    near, far = np.where(np.isnan(near), -np.inf, near), np.where(np.isnan(far), np.inf, far)
    return near.max(axis=-1), far.min(axis=-1)


def moving_box_scene(H=32, W=256, n_sweeps=10):
    """The room (-10, -8, 0) .. (10, 8, 5) seen from inside; sweep k from (0.3 k - 1.5, 0.2, 1.5) with identity rotation; elevations
    linspace(30, -30, H) degrees, azimuths 2 pi j / W; a box of 0.6 x 0.6 x 1.8 m on the floor, centred at (4, -5 + k, 0) in sweep k; ranges
    rounded to mm.  Returns [(xyz f32 (H, W, 3) in the sensor frame, pose 4x4, on_box (H, W))]"""
    el, az = np.radians(np.linspace(30.0, -30.0, H))[:, None], (2.0 * np.pi * np.arange(W) / W)[None, :]
    u = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=2)
    out = []
    for k in range(n_sweeps):
        pos = np.array([0.3 * k - 1.5, 0.2, 1.5])
        _, room_far = _slab(pos, u, ROOM[0], ROOM[1])
        c = np.array([4.0, -5.0 + k, 0.0])
        lo, hi = c - [BOX_SIZE[0] / 2, BOX_SIZE[1] / 2, 0.0], c + [BOX_SIZE[0] / 2, BOX_SIZE[1] / 2, BOX_SIZE[2]]
        b_near, b_far = _slab(pos, u, lo, hi)
        on_box = (b_near <= b_far) & (b_near > 0.0) & (b_near < room_far)
        rng = np.round(np.where(on_box, b_near, room_far) * 1000.0) / 1000.0
        pose = np.eye(4)
        pose[:3, 3] = pos
        out.append(((rng[..., None] * u).astype(np.float32), pose, on_box))
    return out


def moving_box_rays(scene, col_poses=None):
    """[(o, w, ret)] of the scene and the world points of the box's pixels as a set of byte strings (to label stored points); col_poses:
    per sweep (W, 4, 4) as the device evaluated them, else the scene's own pose for every column"""
    sweeps, box = [], set()
    for i, (xyz, pose, on_box) in enumerate(scene):
        H, W = xyz.shape[:2]
        M = np.tile(pose, (W, 1, 1)) if col_poses is None else col_poses[i]
        o, w, ret = rays_of_sweep(xyz.astype(np.float64), np.any(xyz != 0.0, axis=2), M)
        sweeps.append((o, w, ret))
        box.update(r.tobytes() for r in w[on_box.reshape(-1)])
    return sweeps, box


def on_box_mask(stored, box):
    return np.array([np.ascontiguousarray(p).tobytes() in box for p in np.asarray(stored, dtype=np.float64)], dtype=bool)
