"""The occupancy grid (include/ptudes_mi.h ptl_grid_*) restated in numpy, sharing no code with the library.

Two forms of the one definition, checked against each other by tests/test_occupancy_grid_cpu.py:
  grid_plain   ray by ray and sample by sample in Python floats (IEEE doubles, every operation rounded once), a dict for the cells
  grid         the rays of a sweep in lockstep over the sample index (numpy arrays, the same operations element by element) - for scenes of
               10^5 rays
Both take the rays as (origin, end, has_return) per pixel; `rays_of_sweep` (tests/helpers/map_carve_numpy.py: the ray is the carve's) makes
those from sensor-frame points and column poses.  cfg: dict(cell, x0, y0, nx, ny, z_lo, z_hi, margin, step, min_range, max_range).
Counts come back as (free, hit) uint32 arrays (ny, nx) - [iy, ix] - and a dict of the summary."""
import math

import numpy as np

from tests.helpers.map_carve_numpy import rays_of_sweep  # noqa: F401  (re-exported)

COUNTS = ("n_scans", "n_scans_skipped", "n_rays", "n_rays_out_of_range", "n_no_return", "n_runs_voted", "n_ends_outside", "n_cells_free",
          "n_cells_hit", "sum_free", "sum_hit")
BOX = ("box_ix0", "box_iy0", "box_ix1", "box_iy1")
FREE, OCCUPIED, UNKNOWN = 0, 1, 2


def defaults(cell):
    return dict(cell=cell, step=cell / 2.0, margin=cell, min_range=0.0, max_range=600.0 * cell, z_lo=-0.5, z_hi=0.5)


def classify(free, hit, min_hits=2, min_fraction=0.25, min_free=1):
    """the host policy, restated: occupied, else free, else unknown"""
    f, h = np.asarray(free, dtype=np.int64), np.asarray(hit, dtype=np.int64)
    out = np.full(f.shape, UNKNOWN, dtype=np.uint8)
    occupied = (h >= min_hits) & (h >= min_fraction * (h + f))
    out[(f >= min_free) & ~occupied] = FREE
    out[occupied] = OCCUPIED
    return out


def _close(n, free, hit):
    n["n_cells_free"], n["n_cells_hit"] = int((free > 0).sum()), int((hit > 0).sum())
    n["sum_free"], n["sum_hit"] = int(free.astype(np.int64).sum()), int(hit.astype(np.int64).sum())
    iy, ix = np.nonzero((free > 0) | (hit > 0))
    box = (int(ix.min()), int(iy.min()), int(ix.max()), int(iy.max())) if len(ix) else (0, 0, -1, -1)
    n.update(zip(BOX, box))


# ---------------------------------------------------------------------------------------------- plain: Python floats, a dict
def cell_of(px, py, cfg):
    """(ix, iy) of a point, or None outside the grid (a NaN fails the comparison)"""
    fx, fy = (px - cfg["x0"]) / cfg["cell"], (py - cfg["y0"]) / cfg["cell"]
    if not (fx >= 0.0 and fx < float(cfg["nx"]) and fy >= 0.0 and fy < float(cfg["ny"])):
        return None
    return int(fx), int(fy)


def ray_votes(o, w, cfg):
    """(free cells in run order, hit cell or None, end outside the grid) of one USED ray"""
    d = [w[c] - o[c] for c in range(3)]
    ln = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    free, started, cur, band, k = [], False, None, False, 0
    while True:
        tk = (float(k) + 0.5) * cfg["step"]
        if not tk < ln or not tk <= ln - cfg["margin"]:
            break
        ak = tk / ln
        s = [o[c] + ak * d[c] for c in range(3)]
        c = cell_of(s[0], s[1], cfg)
        dz = s[2] - o[2]
        if not started or c != cur:
            if started and cur is not None and band:
                free.append(cur)
            started, cur, band = True, c, False
        band = band or (cfg["z_lo"] <= dz and dz <= cfg["z_hi"])
        k += 1
    wc = cell_of(w[0], w[1], cfg)
    wz = w[2] - o[2]
    hit = wc if wc is not None and cfg["z_lo"] <= wz and wz <= cfg["z_hi"] else None
    if started and cur is not None and band and not (hit is not None and cur == hit):
        free.append(cur)
    return free, hit, wc is None


def grid_plain(sweeps, cfg):
    """sweeps: [(o, w, ret) or None for a skipped sweep].  Returns (free, hit, counts)"""
    free = np.zeros((cfg["ny"], cfg["nx"]), dtype=np.uint32)
    hit = np.zeros((cfg["ny"], cfg["nx"]), dtype=np.uint32)
    n = dict.fromkeys(COUNTS, 0)
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
            runs, h, outside = ray_votes(o, w, cfg)
            for ix, iy in runs:
                free[iy, ix] += 1
            n["n_runs_voted"] += len(runs)
            if h is not None:
                hit[h[1], h[0]] += 1
            n["n_ends_outside"] += int(outside)
    _close(n, free, hit)
    return free, hit, n


# ---------------------------------------------------------------------------------------------- lockstep: arrays
def _cells(px, py, cfg):
    """iy nx + ix per point, -1 outside the grid"""
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = (px - cfg["x0"]) / cfg["cell"], (py - cfg["y0"]) / cfg["cell"]
        inside = (fx >= 0.0) & (fx < float(cfg["nx"])) & (fy >= 0.0) & (fy < float(cfg["ny"]))
    ix, iy = np.where(inside, fx, 0.0).astype(np.int64), np.where(inside, fy, 0.0).astype(np.int64)
    return np.where(inside, iy * cfg["nx"] + ix, -1)


def grid(sweeps, cfg):
    """the same function as grid_plain"""
    free, hit = np.zeros(cfg["ny"] * cfg["nx"], dtype=np.int64), np.zeros(cfg["ny"] * cfg["nx"], dtype=np.int64)
    n = dict.fromkeys(COUNTS, 0)
    step, margin, z_lo, z_hi = cfg["step"], cfg["margin"], cfg["z_lo"], cfg["z_hi"]
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
            used = ret & (ln >= cfg["min_range"]) & (ln <= cfg["max_range"])
        n["n_no_return"] += int((~ret).sum())
        n["n_rays_out_of_range"] += int((ret & ~used).sum())
        n["n_rays"] += int(used.sum())
        o, w, d, ln = o[used], w[used], d[used], ln[used]
        t_free = ln - margin
        cur = np.full(len(o), -2, dtype=np.int64)  # -2: no run yet, -1: a run outside the grid
        band = np.zeros(len(o), dtype=bool)
        live = np.arange(len(o))
        k = 0
        while True:
            tk = (float(k) + 0.5) * step
            live = live[(tk < ln[live]) & (tk <= t_free[live])]
            if not len(live):
                break
            ak = tk / ln[live]
            s = o[live] + ak[:, None] * d[live]
            idx = _cells(s[:, 0], s[:, 1], cfg)
            dz = s[:, 2] - o[live, 2]
            change = cur[live] != idx
            flush = change & (cur[live] >= 0) & band[live]
            np.add.at(free, cur[live][flush], 1)
            n["n_runs_voted"] += int(flush.sum())
            cur[live[change]] = idx[change]
            band[live[change]] = False
            band[live] |= (z_lo <= dz) & (dz <= z_hi)
            k += 1
        widx = _cells(w[:, 0], w[:, 1], cfg)
        wz = w[:, 2] - o[:, 2]
        hits = (widx >= 0) & (z_lo <= wz) & (wz <= z_hi)
        last = (cur >= 0) & band & ~(hits & (cur == widx))
        np.add.at(free, cur[last], 1)
        np.add.at(hit, widx[hits], 1)
        n["n_runs_voted"] += int(last.sum())
        n["n_ends_outside"] += int((widx < 0).sum())
    free, hit = free.astype(np.uint32).reshape(cfg["ny"], cfg["nx"]), hit.astype(np.uint32).reshape(cfg["ny"], cfg["nx"])
    _close(n, free, hit)
    return free, hit, n


# ---------------------------------------------------------------------------------------------- the moving-box scene (map_carve_numpy's)
# cells of 0.5 m placed so that the room's walls (x = +-10, y = +-8) run through the MIDDLE of their cells: an end on a wall lands in the
# wall's cell whichever way its range was rounded.  The band is 1 .. 2 m above the floor for a sensor 1.5 m up: the box (1.8 m) stands in it
BOX_GRID = dict(cell=0.5, x0=-12.25, y0=-10.25, nx=49, ny=41, z_lo=-0.5, z_hi=0.5, margin=0.5, step=0.25, min_range=0.0, max_range=60.0)


def outline_cells(cfg, lo=(-10.0, -8.0), hi=(10.0, 8.0), spacing=0.05):
    """the cells (ix, iy) that hold a point of the room's outline"""
    xs, ys = np.arange(lo[0], hi[0] + spacing / 2, spacing), np.arange(lo[1], hi[1] + spacing / 2, spacing)
    pts = [(x, lo[1]) for x in xs] + [(x, hi[1]) for x in xs] + [(lo[0], y) for y in ys] + [(hi[0], y) for y in ys]
    return {cell_of(float(x), float(y), cfg) for x, y in pts}


def box_trail_cells(scene, sweeps, cfg):
    """the cells that hold an end on the box at band height, over all sweeps"""
    out = set()
    for (_, _, on_box), (o, w, _) in zip(scene, sweeps):
        m = on_box.reshape(-1)
        for p, q in zip(w[m], o[m]):
            if cfg["z_lo"] <= p[2] - q[2] <= cfg["z_hi"]:
                out.add(cell_of(float(p[0]), float(p[1]), cfg))
    return out
