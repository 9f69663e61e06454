"""The cast of a sweep's rays through a map (include/ptudes_mi.h ptl_cast_*) restated in numpy, sharing no code with the library.

Two forms of the one definition, checked against each other by tests/test_map_cast_cpu.py:
  cast_plain   ray by ray and sample by sample in Python floats (IEEE doubles, every operation rounded once), a dict for the voxels
  cast         the rays of a sweep in lockstep over the sample index (numpy arrays, the same operations element by element), a sorted key
               table for the voxels - for sweeps of 10^4 rays and more
Both take the map's STORED points as given, in POOL ORDER (the device's `Caster.points()`: which points a voxel kept and where they lie in the
pool is the map's business; the order only decides ties between equal coordinates) and the rays as (origin, end, has_return) per pixel, as
`map_carve_numpy.rays_of_sweep` makes them.  A sweep that is None was skipped as a whole.  `index` comes back as a row of the stored points
handed in.

The definition.  status 0: no return.  status 3: a return with len2 == 0 or a non-finite end.  Every other return is cast: samples
k = 0, 1, ... while t_k = (k + 0.5) step < max_range, s_k = o + (t_k / len) d, the voxel the map's truncating index; a sample outside the key
range is passed over; consecutive samples with one key visit the voxel once.  A stored point p of a visited voxel, e = p - o, qualifies iff
|e x d|^2 <= (radius radius) len2 and min_range <= t_p = (e . d) / len <= max_range.  The first visited voxel with a qualifying point decides:
its qualifying point with the smallest (t_p, x, y, z, index) is the hit (status 1); no such voxel up to max_range: status 2."""
import math

import numpy as np

from tests.helpers.map_carve_numpy import _keys, first_points_per_voxel, key_of, rays_of_sweep, voxel_dict  # noqa: F401

NONE, HIT, MISS, DEGENERATE = 0, 1, 2, 3
CH_NONE, CH_AGREE, CH_NEW, CH_GONE, CH_UNMAPPED = 0, 1, 2, 3, 4
COUNTS = ("n_pixels", "n_no_return", "n_degenerate", "n_hit", "n_miss", "n_voxel_visits", "skipped")


def defaults(vs):
    return dict(radius=vs / 5.0, step=vs / 2.0, min_range=0.0, max_range=120.0 * vs)


def changes(status, t_hit, length, margin):
    """the host policy, restated pixel by pixel"""
    st, t, ln = np.asarray(status).reshape(-1), np.asarray(t_hit).reshape(-1), np.asarray(length).reshape(-1)
    out = np.zeros(len(st), dtype=np.uint8)
    for i in range(len(st)):
        if st[i] == MISS:
            out[i] = CH_UNMAPPED
        elif st[i] == HIT:
            if abs(ln[i] - t[i]) <= margin:
                out[i] = CH_AGREE
            elif ln[i] < t[i] - margin:
                out[i] = CH_NEW
            elif ln[i] > t[i] + margin:
                out[i] = CH_GONE
    return out.reshape(np.asarray(status).shape)


def _empty(n):
    return (np.zeros(n, dtype=np.uint8), np.full(n, -1.0), np.full(n, -1.0), np.full(n, -1, dtype=np.int32), dict.fromkeys(COUNTS, 0))


# ---------------------------------------------------------------------------------------------- plain: Python floats, a dict
def n_samples(step, max_range):
    k = 0
    while (float(k) + 0.5) * step < max_range:
        k += 1
    return k


def qualifies(p, o, d, ln, rr, cfg):
    """t_p of one stored point against one ray when it qualifies, else None"""
    ex, ey, ez = p[0] - o[0], p[1] - o[1], p[2] - o[2]
    cx, cy, cz = ey * d[2] - ez * d[1], ez * d[0] - ex * d[2], ex * d[1] - ey * d[0]
    if not (cx * cx + cy * cy) + cz * cz <= rr:
        return None
    tp = ((ex * d[0] + ey * d[1]) + ez * d[2]) / ln
    return tp if cfg["min_range"] <= tp <= cfg["max_range"] else None


def cast_plain(stored, sweep, vs, cfg, n_pixels=None, trace=None):
    """Returns (status u8, t_hit, len, index i32, counts), each per pixel.  trace: a list that gets, per cast ray, the keys it visited"""
    if sweep is None:
        out = _empty(n_pixels)
        out[4].update(n_pixels=n_pixels, skipped=1)
        return out
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    vox = voxel_dict(stored, vs)
    P = [[float(x) for x in p] for p in stored]
    o_, w_, ret_ = sweep
    st, th, ln_, ix, n = _empty(len(ret_))
    n["n_pixels"] = len(ret_)
    r2 = cfg["radius"] * cfg["radius"]
    K = n_samples(cfg["step"], cfg["max_range"])
    for i, (o, w, ret) in enumerate(zip(o_, w_, ret_)):
        if not ret:
            n["n_no_return"] += 1
            continue
        o, w = [float(x) for x in o], [float(x) for x in w]
        d = [w[c] - o[c] for c in range(3)]
        len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        ln = math.sqrt(len2) if len2 == len2 else math.nan
        ln_[i] = ln
        if len2 == 0.0 or not all(math.isfinite(x) for x in w):
            st[i] = DEGENERATE
            n["n_degenerate"] += 1
            continue
        rr = r2 * len2
        prev, keys = (False, None), []
        for k in range(K):
            ak = ((float(k) + 0.5) * cfg["step"]) / ln
            key = key_of([o[c] + ak * d[c] for c in range(3)], vs)
            has = key is not None
            new = has and not (prev[0] and prev[1] == key)
            prev = (has, key)
            if not new:
                continue
            keys.append(key)
            ids = vox.get(key)
            if not ids:
                continue
            n["n_voxel_visits"] += 1
            best = None
            for j in ids:
                tp = qualifies(P[j], o, d, ln, rr, cfg)
                if tp is not None:
                    cand = (tp, P[j][0], P[j][1], P[j][2], j)
                    best = cand if best is None or cand < best else best
            if best is not None:
                st[i], th[i], ix[i] = HIT, best[0], best[4]
                break
        if trace is not None:
            trace.append(keys)
        if st[i] == HIT:
            n["n_hit"] += 1
        else:
            st[i] = MISS
            n["n_miss"] += 1
    return st, th, ln_, ix, n


# ---------------------------------------------------------------------------------------------- lockstep: arrays, a sorted key table
def cast(stored, sweep, vs, cfg, n_pixels=None):
    """the same function as cast_plain"""
    if sweep is None:
        out = _empty(n_pixels)
        out[4].update(n_pixels=n_pixels, skipped=1)
        return out
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    skeys, sok = _keys(stored, vs)
    assert sok.all(), "a stored point outside the key range"
    order = np.argsort(skeys, kind="stable")
    ukeys, starts, counts = np.unique(skeys[order], return_index=True, return_counts=True)
    o, w, ret = (np.asarray(a) for a in sweep)
    ret = ret.astype(bool)
    st, th, ln_out, ix, n = _empty(len(ret))
    n["n_pixels"] = len(ret)
    with np.errstate(invalid="ignore", over="ignore"):
        d = w - o
        len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ln = np.sqrt(len2)
    ln_out[ret] = ln[ret]
    degen = ret & ((len2 == 0.0) | ~np.isfinite(w).all(axis=1))
    st[degen] = DEGENERATE
    st[ret & ~degen] = MISS  # (until a hit is found)
    n["n_no_return"], n["n_degenerate"] = int((~ret).sum()), int(degen.sum())
    rr = (cfg["radius"] * cfg["radius"]) * len2
    live = np.flatnonzero(ret & ~degen)
    prev_key, prev_has = np.zeros(len(ret), dtype=np.int64), np.zeros(len(ret), dtype=bool)
    k = 0
    while len(live) and (float(k) + 0.5) * cfg["step"] < cfg["max_range"]:
        tk = (float(k) + 0.5) * cfg["step"]
        with np.errstate(invalid="ignore", over="ignore"):
            ak = tk / ln[live]
            s = o[live] + ak[:, None] * d[live]
        key, has = _keys(s, vs)
        new = has & ~(prev_has[live] & (prev_key[live] == key))
        prev_key[live], prev_has[live] = key, has
        k += 1
        if not (len(ukeys) and new.any()):
            continue
        rays, kk = live[new], key[new]
        at = np.minimum(np.searchsorted(ukeys, kk), len(ukeys) - 1)
        held = ukeys[at] == kk
        rays, at = rays[held], at[held]
        n["n_voxel_visits"] += len(rays)
        if not len(rays):
            continue
        cnt = counts[at]
        rr_ = np.repeat(rays, cnt)
        within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        pid = order[np.repeat(starts[at], cnt) + within]
        p = stored[pid]
        e, dd = p - o[rr_], d[rr_]
        cx = e[:, 1] * dd[:, 2] - e[:, 2] * dd[:, 1]
        cy = e[:, 2] * dd[:, 0] - e[:, 0] * dd[:, 2]
        cz = e[:, 0] * dd[:, 1] - e[:, 1] * dd[:, 0]
        with np.errstate(invalid="ignore", over="ignore"):
            near = (cx * cx + cy * cy) + cz * cz <= rr[rr_]
            tp = ((e[:, 0] * dd[:, 0] + e[:, 1] * dd[:, 1]) + e[:, 2] * dd[:, 2]) / ln[rr_]
            ok = near & (tp >= cfg["min_range"]) & (tp <= cfg["max_range"])
        if not ok.any():
            continue
        rr_, pid, tp, p = rr_[ok], pid[ok], tp[ok], p[ok]
        best = np.lexsort((pid, p[:, 2], p[:, 1], p[:, 0], tp, rr_))  # by ray, then (t_p, x, y, z, index)
        first = best[np.r_[True, rr_[best][1:] != rr_[best][:-1]]]
        st[rr_[first]], th[rr_[first]], ix[rr_[first]] = HIT, tp[first], pid[first]
        live = live[st[live] != HIT]
    n["n_hit"], n["n_miss"] = int((st == HIT).sum()), int((st == MISS).sum())
    return st, th, ln_out, ix, n


def same(a, b):
    """two results of the cast are the same: status, t_hit, len (NaN equals NaN), index, every count"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2], equal_nan=True)
            and np.array_equal(a[3], b[3]) and a[4] == b[4])


# ---------------------------------------------------------------------------------------------- the end-to-end scene: a box the map never saw
SCENE = dict(seed=1000, n_scans=24, H=32, W=256, room_size=(20.0, 16.0, 5.0), n_boxes=6, n_cyls=3)
SCENE_VS, SCENE_P = 0.5, 32  # (32, not 20, points per voxel: see tests/test_map_cast_cpu.py test_the_scene_on_the_restatement_alone)
SCENE_MAP_SWEEPS, SCENE_SWEEP = range(20), 22
SCENE_CFG = dict(radius=0.1, step=0.25, min_range=0.5, max_range=60.0)
SCENE_MARGIN = 0.5
SCENE_BOX_SIZE, SCENE_BOX_AHEAD = (1.0, 1.0, 2.0), 4.0


def scene_sequence():
    from ptudes_lab_amd import synth
    return synth.make_sequence(**SCENE)


def scene_col_ts(seq, k):
    """the firing time of every column of sweep k, seconds from the sequence's start"""
    return (k + np.arange(seq.W) / seq.W) * seq.scan_dt


def scene_with_box(seq):
    """the sequence with a box of SCENE_BOX_SIZE on the floor that no map sweep has seen, its centre SCENE_BOX_AHEAD metres along the
    sensor's own x axis (levelled) from where the sensor is in the middle of sweep SCENE_SWEEP"""
    import dataclasses
    T = seq.pose_at((SCENE_SWEEP + 0.5) * seq.scan_dt)[0]
    ahead = T[:2, 0] / np.linalg.norm(T[:2, 0])
    c = T[:2, 3] + SCENE_BOX_AHEAD * ahead
    hx, hy, hz = (0.5 * s for s in SCENE_BOX_SIZE)
    return dataclasses.replace(seq, boxes=np.vstack([seq.boxes, [c[0], c[1], hz, hx, hy, hz]]))


def scene_sweep(seq, k, col_poses=None):
    """(o, w, ret) of sweep k of a sequence, posed by `col_poses` (W, 4, 4) or else by the sequence's own ground truth at the column times"""
    xyz = seq.scan(k).reshape(seq.H, seq.W, 3)
    M = seq.pose_at(scene_col_ts(seq, k)) if col_poses is None else col_poses
    return rays_of_sweep(xyz.astype(np.float64), np.any(xyz != 0.0, axis=2), M)


def scene_figures(res_plain, res_box, margin=SCENE_MARGIN):
    """the four shares of the issue from the casts of the sweep without and with the box: (hit share of the cast rays, AGREE share of the
    hits, NEW share of the box's pixels, NEW share of all other pixels, number of box pixels).  The box's pixels are those whose measured
    length drops by more than 0.3 m against the same sweep without the box"""
    st, th, ln = res_plain[:3]
    cast_rays = (st == HIT) | (st == MISS)
    ch = changes(st, th, ln, margin)
    st_b, th_b, ln_b = res_box[:3]
    ch_b = changes(st_b, th_b, ln_b, margin)
    on_box = (ln > 0.0) & (ln_b > 0.0) & (ln - ln_b > 0.3)
    return (float((st == HIT).sum() / cast_rays.sum()), float((ch == CH_AGREE).sum() / (st == HIT).sum()),
            float((ch_b[on_box] == CH_NEW).sum() / on_box.sum()), float((ch_b[~on_box] == CH_NEW).sum() / (~on_box).sum()), int(on_box.sum()))
