"""A hand-built map and one 4096-point sweep for the first round of the 8-lane search (csrc/icp_kernels.h gn8_search) - pure numpy + the
CPU oracle; no GPU.

The first round of a search scans four voxels at once: the point's own, the last winner's, and the nearest other occupied boxes.  Without
a last winner outside the own voxel the second slot takes the third-nearest box; and a search whose point changed voxel (phase A queues it
at the back) rebuilds its probe row without reading the old one.  The scene decides, point by point, what those rules meet.

Voxel size 0.5 (pass 1 of the down-sampling on 0.25 m voxels, pass 2 on 0.75 m).  Every source point has a CELL of its own: cells are 3 m
apart in the positive octant (no voxel at a coordinate of 0, where truncation makes voxels double width), the source point sits in the
voxel [o, o + 0.5)^3 of its cell's origin o and the cell's map points in that voxel and its 26 neighbours - nothing of another cell within
2 m.  Every coordinate is a multiple of 1 / 256, exact in float32; the registration of the sweep starts from the identity, so every
distance of its first iteration is exact and a tie is a tie everywhere.

  frame0()   the map: what the runners take as scan 0 (it enters the map as it is: every point has a 0.25 m voxel of its own)
  frame1()   the sweep: CELLS source points as the sensor sees them after moving by MOTION_T, padded with (0, 0, 0)
  kinds()    per source point, what its cell was built as:
             'anchor'   a map point exactly MOTION_T from the source in its own voxel (the registration's answer), random others around
             'random'   no anchor: an own-voxel point or none, 0 .. 6 other occupied boxes with 1 .. 3 points each, pushed towards the source
             'third'    exactly three other occupied boxes, the nearest map point in the third-nearest of them
             'fourth'   four other occupied boxes, the nearest map point in the fourth-nearest
             'tie_own' / 'tie_box'  exactly three others; a point of the third-nearest box and one of the own voxel at exactly the same distance,
                        both nearest: the own voxel comes first in visiting order / the box does
             'alone'    the own voxel holds the anchor, the 26 neighbours are empty
             'one_box'  the own voxel is empty, one neighbour holds points
             'crosser'  the source starts 1/128 .. 11/128 m below the +x face of its voxel: the Gauss-Newton iterations (MOTION_T[0] = 12/128)
                        carry it across, its anchor lies in the next voxel
  first_iteration() / iterations()   numpy + oracle: what the first search of every source point meets, and the positions of every iteration
tests/test_search_chain_scenes_cpu.py shows that the scene is what it claims; tests/test_gpu_search_chain.py holds the device against it.
"""
import functools

import numpy as np

from oracle import cpu as orc

H, W = 32, 1024
N = H * W                # points per scan the runners are created for (frame 0, the map, needs more than the sweep's 4096)
CELLS = 4096             # source points of the sweep
VOXEL_SIZE, MAX_RANGE, MIN_RANGE = 0.5, 100.0, 0.5
THRESHOLD = 0.25         # initial_threshold: gate 0.75 m, kernel 1/12 m
ICP = dict(voxel_size=VOXEL_SIZE, deskew=0, initial_threshold=THRESHOLD)
PITCH = 3.0
MOTION_T = np.array([12.0, -10.0, 8.0]) / 128.0
U0 = np.array([22.0, 18.0, 13.0]) / 64.0  # a source point inside its voxel: six different distances to the faces
COUNTS = dict(third=160, fourth=160, tie_own=48, tie_box=48, alone=120, one_box=120, crosser=640, random=1200)  # the rest: anchors


def _offsets():
    e = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)  # entry 9 (ex + 1) + 3 (ey + 1) + (ez + 1)
    return e


def box_gap2(u, vs=VOXEL_SIZE):
    """squared distance from a point at u inside its voxel [0, vs)^3 to each of the 27 boxes, as the search forms it ((gx + gy) + gz)"""
    e = _offsets()
    g = np.where(e < 0, np.maximum(u - 1e-9, 0.0), np.where(e > 0, np.maximum(vs - u - 1e-9, 0.0), 0.0))
    g2 = g * g
    return (g2[:, 0] + g2[:, 1]) + g2[:, 2]


@functools.lru_cache(maxsize=None)
def kinds():
    rng = np.random.default_rng(2201)
    k = np.array(sum(([name] * n for name, n in COUNTS.items()), []) + ["anchor"] * (CELLS - sum(COUNTS.values())))
    return k[rng.permutation(CELLS)]


@functools.lru_cache(maxsize=None)
def origins():
    g = np.stack(np.meshgrid(*[np.arange(1, 17)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return PITCH * g[np.random.default_rng(2202).permutation(len(g))[:CELLS]].astype(np.float64)


def _toward(rng, u, e, n, reach):
    """n points (multiples of 1/256, relative to the voxel's corner) inside box e, near the point of the box that is nearest to u, at most
    reach further on each axis"""
    lo, hi = 0.5 * e, 0.5 * e + 0.5
    near = np.clip(u, lo, hi - 1.0 / 256)
    step = rng.integers(0, int(reach * 256) + 1, (n, 3)) / 256.0
    p = np.where(e < 0, near - step, np.where(e > 0, near + step, near + (step - 0.5 * reach)))
    return np.clip(np.round(p * 256) / 256, lo, hi - 1.0 / 256)


def _others(rng, u, boxes, reach=0.125):
    out = []
    for b in boxes:
        out.append(_toward(rng, u, _offsets()[b], int(rng.integers(1, 4)), reach))
    return out


def _far_in_box(u, e, r):
    """one point of box e farther than r from u: the box's far corner region"""
    lo, hi = 0.5 * e, 0.5 * e + 0.5
    p = np.where(e < 0, lo + 1.0 / 64, np.where(e > 0, hi - 1.0 / 64, np.clip(u, lo, hi - 1.0 / 256)))
    assert np.linalg.norm(p - u) > r
    return p[None, :]


@functools.lru_cache(maxsize=None)
def cells():
    """per cell: (u, [map points]) relative to the cell's origin, the source at u"""
    rng = np.random.default_rng(2203)
    out = []
    E = _offsets()
    for kind in kinds():
        u = U0.copy()
        pts = []
        if kind in ("anchor", "alone", "random", "one_box"):
            u = rng.integers(40, 88, 3) / 256.0  # anywhere in the middle of the voxel: the anchor stays inside it
        if kind in ("anchor", "alone"):
            pts.append((u + MOTION_T)[None, :])
        if kind == "anchor":
            pts += _others(rng, u, rng.choice(np.delete(np.arange(27), 13), int(rng.integers(0, 3)), replace=False), reach=0.25)
        if kind == "random":
            if rng.random() < 0.7:
                pts.append(_toward(rng, u, E[13], int(rng.integers(1, 4)), 0.25))
            pts += _others(rng, u, rng.choice(np.delete(np.arange(27), 13), int(rng.integers(0, 7)), replace=False))
        if kind == "one_box":
            pts += _others(rng, u, rng.choice(np.delete(np.arange(27), 13), 1))
        if kind in ("third", "fourth"):
            # the other boxes in the order of their distance from U0: + x (10/64), - z (13/64), + y (14/64), - y (18/64), + z (19/64)
            order = [22, 12, 16, 10, 14]
            nb = 3 if kind == "third" else 4
            pts.append((u + np.array([-70.0, 40.0, 40.0]) / 256.0 + rng.integers(-2, 3, 3) / 256.0)[None, :])  # own voxel: about 0.35 m away
            for j, b in enumerate(order[:nb]):
                e = E[b]
                if j == nb - 1:  # the nearest map point of the cell: just inside the last box
                    pts.append(_toward(rng, u, e, 1, 1.0 / 128))
                else:
                    pts.append(_far_in_box(u, e, 0.4))
        if kind in ("tie_own", "tie_box"):
            r = 39.0 / 128.0
            if kind == "tie_box":
                u = np.array([22.0, 18.0, 19.0]) / 64.0  # mirrored in z: the third-nearest box is - z (entry 12 < 13)
            third, a, b = (14, 22, 12) if kind == "tie_own" else (12, 22, 14)
            pts.append((u - np.array([r, 0.0, 0.0]))[None, :])                               # own voxel, r away
            pts.append((u + np.array([0.0, 0.0, r if kind == "tie_own" else -r]))[None, :])  # the third-nearest box, r away
            pts.append(_far_in_box(u, E[a], 0.32))
            pts.append(_far_in_box(u, E[b], 0.32))
        if kind == "crosser":
            u = np.array([0.5 - int(rng.integers(1, 12)) / 128.0, int(rng.integers(48, 80)) / 256.0, int(rng.integers(48, 80)) / 256.0])
            pts.append((u + MOTION_T)[None, :])  # in the + x voxel
            pts.append(_toward(rng, u, E[13], 2, 0.25))
            pts += _others(rng, u, rng.choice(np.array([22, 4, 21, 25, 16]), int(rng.integers(0, 3)), replace=False), reach=0.25)
        p = np.concatenate(pts) if pts else np.zeros((0, 3))
        # one map point per 0.25 m voxel (pass 1 of the down-sampling keeps the first): later arrivals are dropped, what a kind is built on comes first
        _, first = np.unique(np.floor(p / 0.25).astype(np.int64), axis=0, return_index=True)
        out.append((u, p[np.sort(first)]))
    return out


def _pad(p):
    out = np.zeros((N, 3))
    out[: len(p)] = p
    f = out.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), out)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def frame0():
    p = np.concatenate([o + pts for o, (_, pts) in zip(origins(), cells())])
    assert len(p) <= N
    return _pad(p[np.random.default_rng(2204).permutation(len(p))])


@functools.lru_cache(maxsize=None)
def frame1():
    return _pad(np.stack([o + u for o, (u, _) in zip(origins(), cells())]))


def source():
    return frame1()[:CELLS].astype(np.float64)


@functools.lru_cache(maxsize=None)
def first_iteration():
    """per source point, at the identity: others = occupied boxes other than its own, own = the own voxel holds a point, rank = position of
    the nearest map point's box among the others in the order the search takes them (squared box distance, then entry; -1: the own
    voxel, -2: no map point), tie = the nearest distance is shared by the own voxel and the third-nearest box"""
    E = _offsets()
    res = dict(others=[], own=[], rank=[], tie=[], nearest_entry=[])
    for (u, pts), kind in zip(cells(), kinds()):
        ent = ((np.floor(pts / 0.5).astype(np.int64) + 1) @ np.array([9, 3, 1])) if len(pts) else np.zeros(0, dtype=np.int64)
        assert ((ent >= 0) & (ent < 27)).all()
        occ = np.unique(ent)
        oth = occ[occ != 13]
        g2 = box_gap2(u)
        order = oth[np.lexsort((oth, g2[oth]))]
        res["others"].append(len(oth))
        res["own"].append(13 in occ)
        if len(pts) == 0:
            res["rank"].append(-2); res["tie"].append(False); res["nearest_entry"].append(-1)
            continue
        d2 = ((pts - u) ** 2).sum(axis=1)
        best = np.flatnonzero(d2 == d2.min())
        e_best = ent[best].min()  # (distance, visiting order): the lower entry wins a tie between voxels
        res["nearest_entry"].append(int(e_best))
        res["rank"].append(-1 if e_best == 13 else int(np.flatnonzero(order == e_best)[0]))
        res["tie"].append(bool(len(order) >= 3 and {13, int(order[2])} <= set(ent[best].tolist())))
    return {k: np.array(v) for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def iterations(max_iter=40):
    """the registration of the sweep against the map, restated with the oracle's pieces (Map.linear_system, solve6, se3_exp), keeping every
    iteration: list of (source positions, targets) - the positions the device's phase A and its searches see"""
    orc.set_threads(1)
    m = orc.Map(VOXEL_SIZE, MAX_RANGE, 20)
    m.add_points(orc.voxel_downsample(orc.preprocess(frame0().astype(np.float64), MAX_RANGE, MIN_RANGE), 0.5 * VOXEL_SIZE))
    s = source().copy()
    out = []
    for _ in range(max_iter):
        sums, nc, cand, tgt = m.linear_system(s, 3.0 * THRESHOLD, THRESHOLD / 3.0, want_targets=True)
        out.append((s.copy(), tgt.copy()))
        dx = orc.solve6(sums)
        T = orc.se3_exp(dx)
        s = s @ T[:3, :3].T + T[:3, 3]
        if np.linalg.norm(dx) < 1e-4:
            break
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """the oracle's run of the two scans: statistics, poses, the second scan's source cloud"""
    orc.set_threads(1)
    ref = orc.ICP(MAX_RANGE, MIN_RANGE, **ICP)
    for f in (frame0(), frame1()):
        ref.register_frame(f.astype(np.float64), None)
    return dict(stats=ref.stats, poses=np.array(ref.poses()), source=ref.last_source())
