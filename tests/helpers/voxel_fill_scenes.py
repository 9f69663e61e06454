"""A hand-built map whose voxels hold exactly 0 (absent), 1, 7, 8, 9, 16, 17 and 20 points - the chunk boundaries of the 8-lane voxel scan
(csrc/icp_kernels.h scan_voxelsL: lane l <-> stored points l, l + 8, l + 16; csrc/top2.h) - and one sweep of 1 024 source points, each in a
cell of its own.  Pure numpy + the CPU oracle; no GPU.  Built the way search_chain_scenes.py builds its map: the runners take the map as
scans.

Voxel size 0.5: pass 1 of the down-sampling keeps one point per 0.25 m voxel, so a scan brings at most 8 points to a voxel and a voxel of 20
needs three.  frames()[0 .. 2] are the map, frames()[3] is the sweep.  A voxel of n points gets min(n, 8) points from scan 0, each in a
0.25 m voxel of its own; up to 8 from scan 1 and the rest from scan 2: FIRST a copy of the voxel's point 0, then new points in the other
0.25 m voxels.  Only the 8 voxels of a cell on the low side of every axis (own voxel included) take points after scan 0: each of them lies
in a 0.75 m voxel of its own, so the copy is what pass 2 keeps as source point, every source point of scans 1 and 2 lies ON a map point,
their registration is the identity exactly and the map is the points as written here, in this order: stored point 8 (and 16) of a voxel
of more than 8 (16) is a copy of its point 0 - an exact tie inside one lane.

Cells are 3 m apart in the positive octant; the source point sits at U in the voxel [o, o + 0.5)^3 of its cell's origin o, near the low
faces: the boxes on the low side are the nearest.  Every coordinate is a multiple of 1 / 256 (exact in float32), the sweep starts from the
identity, so every distance of its first iteration is exact and a tie is a tie everywhere.

  kinds()    'random'      1 .. 6 of the low-side voxels and sometimes one of the others occupied, fills drawn from FILLS
             'tie_lane'    the own voxel holds 9, 16, 17 or 20 and its point 0 is the nearest: tied with its copies at 8 (and 16)
             'tie_lanes'   two points of the own voxel at exactly 0.25 m, both nearest, in different lanes
             'tie_vox_lo'  a point of the - x voxel (entry 4) and one of the own voxel (entry 13) at exactly 10/64 m: the lower id, scanned
                           in the same round, wins; the - x voxel's point sits at stored index 0, 5, 11 or 18 of up to 20
             'tie_vox_hi'  a point of the own voxel and one of the + x voxel (entry 22) at exactly 26/64 m: the own voxel wins
             'deep'        the nearest stored point in the second-, third- or fourth-nearest occupied box (a voxel of 16, 17 or 20): the boxes
                           before it, and the own voxel if there is one, hold a single far point
  first_iteration()   numpy alone: per source point where its nearest stored point sits (voxel entry, stored index, place of the voxel in the
                      search: 0 own, 1 / 2 the two nearest other occupied boxes, 3 the third-nearest (the idle slot), 4 a survivor round),
                      and what ties with it
tests/test_voxel_fill_scenes_cpu.py shows that the scene is what it claims; tests/test_gpu_voxel_fill.py holds the device against it.
"""
import functools

import numpy as np

from oracle import cpu as orc
from tests.helpers.search_chain_scenes import _offsets, box_gap2

H, W = 32, 1024
N = H * W
CELLS = 1024
VOXEL_SIZE, MAX_RANGE, MIN_RANGE = 0.5, 100.0, 0.5
THRESHOLD = 0.25
ICP = dict(voxel_size=VOXEL_SIZE, deskew=0, initial_threshold=THRESHOLD)
PITCH = 3.0
FILLS = (0, 1, 7, 8, 9, 16, 17, 20)
U = np.array([6.0, 9.0, 13.0]) / 64.0
MAP_SCANS = 3
COUNTS = dict(tie_lane=48, tie_lanes=32, tie_vox_lo=48, tie_vox_hi=32, deep=144)  # the rest: random
E = _offsets()
LOW = [int(i) for i in np.flatnonzero((E <= 0).all(axis=1))]   # own voxel and the 7 on the low side: may take points from every scan
HIGH = [i for i in range(27) if i not in LOW]
SUB = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)  # the 8 voxels of pass 1 inside a map voxel


def per_scan(n):
    """points a voxel of n takes from scans 0, 1, 2"""
    return min(n, 8), min(max(n - 8, 0), 8), max(n - 16, 0)


def _in_sub(rng, e, sub, lo=8, hi=56, far=None):
    """a point (relative to the cell's origin) in 0.25 m voxel `sub` of map voxel E[e]; far: offsets >= far / 256 on the axes where sub is 1"""
    off = rng.integers(lo, hi, 3)
    if far is not None:
        off = np.where(sub > 0, rng.integers(far, hi, 3), off)
    return 0.5 * E[e] + 0.25 * sub + off / 256.0


def _voxel(rng, e, n, fixed=None, subs=None, far=None):
    """the stored points of map voxel e holding n points, in storage order, as a list of three arrays (one per scan).  fixed: {stored
    index: point} (indices 8 and 16 are copies and cannot be fixed); subs: the 0.25 m voxels the other points may use"""
    fixed = dict(fixed or {})
    k = per_scan(n)
    assert e in LOW or n <= 8
    out, p0 = [], None
    for f in range(3):
        pts, used = [None] * k[f], set()
        base = 8 * f
        if f > 0 and k[f] > 0:
            pts[0] = p0
            used.add(tuple(np.floor((p0 - 0.5 * E[e]) / 0.25).astype(int)))
        for idx, p in fixed.items():
            if idx < base and idx >= 8:  # a point fixed in an earlier scan after scan 0 keeps its 0.25 m voxel to itself from then on
                used.add(tuple(np.floor((np.asarray(p) - 0.5 * E[e]) / 0.25).astype(int)))
            if base <= idx < base + k[f]:
                assert not (f > 0 and idx == base)
                pts[idx - base] = np.asarray(p, dtype=np.float64)
                used.add(tuple(np.floor((pts[idx - base] - 0.5 * E[e]) / 0.25).astype(int)))
        free = [s for s in (SUB if subs is None else subs) if tuple(s) not in used]
        free = [free[i] for i in rng.permutation(len(free))]
        for j in range(k[f]):
            if pts[j] is None:
                pts[j] = _in_sub(rng, e, free.pop(), far=far)
        if f == 0 and k[0] > 0:
            p0 = pts[0]
        out.append(np.array(pts).reshape(-1, 3))
    return out


@functools.lru_cache(maxsize=None)
def kinds():
    rng = np.random.default_rng(2511)
    k = np.array(sum(([name] * n for name, n in COUNTS.items()), []) + ["random"] * (CELLS - sum(COUNTS.values())))
    return k[rng.permutation(CELLS)]


@functools.lru_cache(maxsize=None)
def origins():
    g = np.stack(np.meshgrid(*[np.arange(1, 17)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return PITCH * g[np.random.default_rng(2512).permutation(len(g))[:CELLS]].astype(np.float64)


FAR_SUBS = [s for s in SUB if s.sum() >= 2]  # 0.25 m voxels of the own voxel whose points (offsets >= 32 / 256) are > 0.28 m from U
F1, F2 = np.array([56.0, 56.0, 124.0]) / 256.0, np.array([56.0, 120.0, 8.0]) / 256.0  # two more of the own voxel, 0.32 and 0.39 m from U
DEEP_ORDER = [4, 10, 1, 12]  # the low-side boxes nearest to U: - x (0.094 m), - y (0.141), - x - y (0.169), - z (0.203)


@functools.lru_cache(maxsize=None)
def cells():
    """per cell: {voxel entry: [points of scan 0, of scan 1, of scan 2]} relative to the cell's origin, the source point at U"""
    rng = np.random.default_rng(2513)
    out = []
    for n_cell, kind in enumerate(kinds()):
        vox = {}
        if kind in ("random", "tie_lane"):
            low = [e for e in LOW if e != 13]
            for e in rng.choice(low, int(rng.integers(0, 6)), replace=False):
                vox[int(e)] = _voxel(rng, int(e), int(rng.choice(FILLS[1:])))
            if rng.random() < 0.3:
                e = int(rng.choice(HIGH))
                vox[e] = _voxel(rng, e, int(rng.choice((1, 7, 8))))
        if kind == "random":
            n = int(rng.choice(FILLS))
            if n > 0:
                vox[13] = _voxel(rng, 13, n)
        if kind == "tie_lane":  # point 0 of the own voxel 0.058 m from U: nothing else of the cell is nearer than 0.078 m
            vox[13] = _voxel(rng, 13, (9, 16, 17, 20)[n_cell % 4], fixed={0: U + np.array([3.0, 2.0, 1.0]) / 64.0})
        if kind == "tie_lanes":  # the low side empty but for the far corner's voxel (box 0.264 m away)
            a, b = ((0, 1), (2, 5), (4, 3))[n_cell % 3]
            vox[13] = _voxel(rng, 13, 7, fixed={a: U + np.array([16.0, 0, 0]) / 64.0, b: U + np.array([0, 16.0, 0]) / 64.0, 6: F1}, subs=FAR_SUBS, far=32)
            vox[0] = _voxel(rng, 0, int(rng.choice(FILLS[1:])))
        if kind == "tie_vox_lo":  # - y empty (its box is nearer than the tie); every other box is farther than 10/64
            idx = (0, 5, 11, 18)[n_cell % 4]
            fixed = {idx: U - np.array([10.0, 0, 0]) / 64.0}
            if idx >= 8:  # the scans before the tied point's fill its 0.25 m voxel too: with a point at its far side, 0.3 m from U
                fixed[3] = 0.5 * E[4] + 0.25 * np.array([1.0, 0, 0]) + np.array([10.0, 30.0, 30.0]) / 256.0
            if idx >= 16:
                fixed[10] = 0.5 * E[4] + 0.25 * np.array([1.0, 0, 0]) + np.array([12.0, 28.0, 26.0]) / 256.0
            vox[4] = _voxel(rng, 4, (8, 9, 17, 20)[n_cell % 4] if idx < 8 else 20, fixed=fixed, far=24)
            j = int(rng.integers(0, 7))
            vox[13] = _voxel(rng, 13, 7, fixed={j: U + np.array([10.0, 0, 0]) / 64.0, (j + 1) % 7: F1, (j + 2) % 7: F2}, subs=FAR_SUBS, far=32)
            for e in rng.choice([1, 3, 9, 12, 0], int(rng.integers(0, 3)), replace=False):
                vox[int(e)] = _voxel(rng, int(e), int(rng.choice(FILLS[1:])))
        if kind == "tie_vox_hi":  # everything but the own voxel, + x and the + + + corner empty
            vox[13] = _voxel(rng, 13, 1, fixed={0: U + np.array([24.0, 10.0, 0]) / 64.0})
            n = (1, 7, 8)[n_cell % 3]
            vox[22] = _voxel(rng, 22, n, fixed={int(rng.integers(0, n)): U + np.array([26.0, 0, 0]) / 64.0})
            if rng.random() < 0.5:
                vox[26] = _voxel(rng, 26, int(rng.choice((1, 7, 8))))
        if kind == "deep":  # the own voxel and the boxes before the k-th hold one far point each, the k-th nearest box is full
            k = 2 + n_cell % 3
            if n_cell % 2:
                vox[13] = _voxel(rng, 13, 1, subs=[np.array([1, 1, 1])], far=40)
            for e in DEEP_ORDER[: k - 1]:
                vox[e] = _voxel(rng, e, 1, subs=[np.where(E[e] < 0, 0, 1)], far=32)
            vox[DEEP_ORDER[k - 1]] = _voxel(rng, DEEP_ORDER[k - 1], (16, 17, 20)[(n_cell // 3) % 3])
        out.append(vox)
    return out


def stored(vox):
    """{entry: (n, 3) stored points in storage order}"""
    return {e: np.concatenate(v) for e, v in vox.items()}


def _pad(p):
    out = np.zeros((N, 3))
    assert len(p) <= N, len(p)
    out[: len(p)] = p
    f = out.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), out)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def frames():
    """the four scans: three that build the map (cell after cell, voxel after voxel in entry order, points in storage order) and the sweep"""
    out = []
    for f in range(MAP_SCANS):
        out.append(_pad(np.concatenate([o + vox[e][f] for o, vox in zip(origins(), cells()) for e in sorted(vox)])))
    out.append(_pad(origins() + U))
    return out


def source():
    return frames()[MAP_SCANS][:CELLS].astype(np.float64)


@functools.lru_cache(maxsize=None)
def first_iteration():
    """per source point at the identity, numpy alone: fills = stored points of its 27 voxels, entry / index / chunk of the nearest stored point
    under (distance, entry * 32 + index), place (0 own voxel, 1 / 2 nearest and second-nearest other occupied box, 3 third-nearest, 4 a later
    one; -1 nothing stored), and what shares the nearest distance: copies (same position), lane (same voxel, indices l and l + 8 k), lanes
    (same voxel, other lanes), voxels (another voxel; tie_winner_entry < tie_loser_entry or >)"""
    keys = ("entry", "index", "chunk", "place", "copies", "lanes", "voxels", "other_entry")
    res = {k: [] for k in keys}
    fills = np.zeros((CELLS, 27), dtype=np.int64)
    g2 = box_gap2(U)
    for n, vox in enumerate(cells()):
        st = stored(vox)
        for e, p in st.items():
            fills[n, e] = len(p)
        if not st:
            for k in keys:
                res[k].append(-1 if k in ("entry", "index", "chunk", "place", "other_entry") else 0)
            continue
        ent = np.concatenate([np.full(len(p), e) for e, p in st.items()])
        idx = np.concatenate([np.arange(len(p)) for p in st.values()])
        pts = np.concatenate(list(st.values()))
        d2 = ((pts - U) ** 2).sum(axis=1)
        order = np.lexsort((ent * 32 + idx, d2))
        w = order[0]
        tied = order[1:][d2[order[1:]] == d2[w]]
        same_pos = np.array([np.array_equal(pts[t], pts[w]) for t in tied], dtype=bool)
        oth = np.array(sorted(e for e in st if e != 13), dtype=np.int64)
        oth = oth[np.lexsort((oth, g2[oth]))] if len(oth) else oth
        place = 0 if ent[w] == 13 else min(int(np.flatnonzero(oth == ent[w])[0]) + 1, 4)
        res["entry"].append(int(ent[w])); res["index"].append(int(idx[w])); res["chunk"].append(int(idx[w]) // 8); res["place"].append(place)
        res["copies"].append(int(same_pos.sum()))
        res["lanes"].append(int(((ent[tied] == ent[w]) & ~same_pos).sum()))
        res["voxels"].append(int((ent[tied] != ent[w]).sum()))
        res["other_entry"].append(int(ent[tied][ent[tied] != ent[w]][0]) if (ent[tied] != ent[w]).any() else -1)
    out = {k: np.array(v) for k, v in res.items()}
    out["fills"] = fills
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """the oracle's run of the four scans: statistics, poses, the sweep's source cloud, the map after the three map scans"""
    orc.set_threads(1)
    ref = orc.ICP(MAX_RANGE, MIN_RANGE, **ICP)
    map_points = None
    for k, f in enumerate(frames()):
        ref.register_frame(f.astype(np.float64), None)
        if k == MAP_SCANS - 1:
            map_points = ref.map.points()
    return dict(stats=ref.stats, poses=np.array(ref.poses()), source=ref.last_source(), map_points=map_points)


@functools.lru_cache(maxsize=None)
def iterations(max_iter=60):
    """the registration of the sweep against the map of the three map scans, restated with the oracle's pieces (Map.add_points,
    Map.linear_system, solve6, se3_exp): (iterations, final pose)"""
    orc.set_threads(1)
    m = orc.Map(VOXEL_SIZE, MAX_RANGE, 20)
    for f in frames()[:MAP_SCANS]:
        m.add_points(orc.voxel_downsample(orc.preprocess(f.astype(np.float64), MAX_RANGE, MIN_RANGE), 0.5 * VOXEL_SIZE))
    s = source().copy()
    T = np.eye(4)
    for it in range(1, max_iter + 1):
        sums, _, _ = m.linear_system(s, 3.0 * THRESHOLD, THRESHOLD / 3.0)
        dx = orc.solve6(sums)
        D = orc.se3_exp(dx)
        s = s @ D[:3, :3].T + D[:3, 3]
        T = D @ T
        if np.linalg.norm(dx) < 1e-4:
            break
    return it, T
