"""Scenes in which voxels fill at once, for the map update's "the voxel is full" path (pure numpy + the CPU oracle; no GPU).

AddPoints stores nothing for a point whose voxel already holds max_points_per_voxel points, and the device's insert a settles such a point
where it reads the voxel's table entry (csrc/icp_kernels.h d_map_insert_a).  With the default of 20 points per voxel a scene needs many
sweeps before that path carries weight; here the cap is 3 or 4, so it does from the second batch on.
tests/test_full_voxel_scenes_cpu.py shows with the oracle alone that the scenes are what they claim;
tests/test_gpu_map_full_voxels.py holds the device against them.

Coordinates of the stage scene are dyadic and well inside their voxels, as in hash_scenes.py.
"""
import functools

import numpy as np

from oracle import cpu as orc
from tests.helpers import hash_scenes as hs

# ------------------------------------------------------------------------------------------------ the map stage, teacher-forced
STAGE_P, STAGE_CAP, STAGE_N_MAX, STAGE_RANGE = 3, 1 << 12, 2048, 30.0
STAGE_LINE = STAGE_CAP // 16           # the colliding voxels home on this line of the table and the next (16 slots)
N_COLLIDING = 24                       # ... more voxels than slots: at least 8 sit at probe distance >= 1, whatever order they arrive in
WAVE = 64


def _distinct_voxels(rng, n, exclude):
    """n voxels of [-8, 8)^3 in a shuffled order, none of `exclude`"""
    flat = rng.permutation(16 ** 3)
    vox = np.stack([flat // 256, flat // 16 % 16, flat % 16], axis=1).astype(np.int64) - 8
    vox = vox[~np.isin(hs.pack_key(vox), hs.pack_key(exclude))]
    assert len(vox) >= n
    return vox[:n]


def _into(vox, rng):
    """one point in each of `vox` (repeats allowed), at fractions 1/8 .. 7/8 (positions no point of the first batch has)"""
    vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    return hs.points_in(vox, 0.125 + 0.25 * rng.integers(0, 4, (len(vox), 3)))


@functools.lru_cache(maxsize=None)
def stage_scene(seed=0):
    """Three calls of the stage-level map insert on a STAGE_CAP-slot table, max_points_per_voxel = 3, voxel size 1.0, as a dict:
      batches[0]   leaves `full` voxels at 3 points (the N_COLLIDING first of them home on 16 slots), `two` voxels at 2, `one` voxels at 1
      batches[1]   >= 1024 points, by wavefront of 64 consecutive points:
                     0, 1   full voxels only (a run of 128 points that store nothing)
                     2      a mix: full voxels, voxels at 1 and 2 points, new voxels - among them three candidates for ONE voxel at 2 (the first
                            in scan order enters), six points of one new voxel (the first three enter) and five of another
                     3 ..   the same kinds at random, every colliding full voxel among them
      batches[2]   points into every full voxel and some new ones, with `origin`: the prune that follows takes the full voxels whose first point
                   is farther than STAGE_RANGE from it - touched by this very batch - and leaves the others
    """
    rng = np.random.default_rng(seed)
    lines = STAGE_CAP // 8
    col = hs.homing_voxels(STAGE_CAP, [STAGE_LINE % lines, (STAGE_LINE + 1) % lines])[:N_COLLIDING]
    rest = _distinct_voxels(rng, 96 + 32 + 32 + 120, col)
    full, two, one, new = np.concatenate([col, rest[:96]]), rest[96:128], rest[128:160], rest[160:]
    own = np.concatenate([np.repeat(np.arange(len(full)), 3), len(full) + np.repeat(np.arange(len(two)), 2), len(full) + len(two) + np.arange(len(one))])
    vox1 = np.concatenate([full, two, one])
    b1 = hs.points_in(vox1[own], rng.integers(1, 4, (len(own), 3)) * 0.25)
    order = rng.permutation(len(b1))
    b1, own = b1[order], own[order]
    first = np.array([b1[own == v][0] for v in range(len(vox1))])  # a voxel's first point in scan order: what the prune looks at

    def pick(v, n):
        return v[rng.integers(0, len(v), n)]

    w01 = full[np.arange(2 * WAVE) % len(full)]
    w2 = np.concatenate([pick(full, 24), np.repeat(two[:1], 3, axis=0), np.repeat(new[:1], 6, axis=0), np.repeat(new[1:2], 5, axis=0),
                         pick(two[1:], 6), pick(one, 8), new[2:14]])
    assert len(w2) == WAVE
    w2 = w2[rng.permutation(WAVE)]
    n_tail = 1100 - 3 * WAVE
    tail = np.concatenate([col, pick(full, int(0.6 * n_tail) - len(col)), pick(np.concatenate([two, one]), int(0.2 * n_tail)), pick(new[14:100], n_tail - int(0.6 * n_tail) - int(0.2 * n_tail))])
    tail = tail[rng.permutation(len(tail))]
    b2 = _into(np.concatenate([w01, w2, tail]), rng)
    origin = np.array([24.0, 0.0, 0.0])
    b3v = np.concatenate([full, full[::2], new[100:], two[:8]])
    b3 = _into(b3v[rng.permutation(len(b3v))], rng)
    far = ((first[: len(full)] - origin) ** 2).sum(axis=1) > STAGE_RANGE ** 2
    return dict(batches=[b1, b2, b3], origin=origin, full=full, two=two, one=one, new=new, colliding=col, full_far=far)


def stage_oracle(sc):
    """the oracle's side of the three calls: per call (map size, sorted map points, points of the call that found their voxel full)"""
    m = orc.Map(1.0, STAGE_RANGE, STAGE_P)
    out = []
    for i, b in enumerate(sc["batches"]):
        dropped = count_dropped(m.points() if m.num_points else np.zeros((0, 3)), b, 1.0, STAGE_P)
        m.add_points(b)
        if i == 2:
            m.prune(sc["origin"])
        pts = m.points()
        out.append(((m.num_voxels, m.num_points), pts[np.lexsort(pts.T[::-1])], dropped))
    return out


def count_dropped(map_points, batch_world, voxel_size, P):
    """points of `batch_world` whose voxel holds P points in a map of `map_points`: what the device's insert a drops (its counter
    `dropped_full_voxel`)"""
    if len(map_points) == 0:
        return 0
    uk, cnt = np.unique(hs.pack_key(hs.voxel_of(map_points, voxel_size)), return_counts=True)
    assert cnt.max() <= P
    return int(np.isin(hs.pack_key(hs.voxel_of(batch_world, voxel_size)), uk[cnt >= P]).sum())


# ------------------------------------------------------------------------------------------------ a static sensor in a small box
BOX_N, BOX_H, BOX_W, BOX_P, BOX_RANGE, BOX_MIN = 9, 16, 256, 4, 12.0, 0.5
BOX_PTS = BOX_H * BOX_W
BOX_ICP = dict(voxel_size=1.0, deskew=0, max_points_per_voxel=BOX_P)
_BOX_LO, _BOX_HI = np.array([-5.0, -4.0, -1.5]), np.array([5.5, 4.5, 2.0])


def _box_ranges(d):
    """distance along unit directions d (n, 3) from the origin to the walls of the box"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, _BOX_HI / d, np.where(d < 0, _BOX_LO / d, np.inf))
    return t.min(axis=1)


@functools.lru_cache(maxsize=None)
def box_sweeps(seed=0):
    """BOX_N sweeps of BOX_H x BOX_W float32 points from a sensor that stands still in a box of 10.5 x 8.5 x 3.5 m: the same rays every sweep
    (beams at -24 .. +24 degrees), 1 cm of range noise of its own per sweep.  Every ray returns; one sweep brings about four points to every
    1 m voxel of the walls it sees, so with 4 points per voxel the map is nearly full after the first"""
    rng = np.random.default_rng(seed)
    el = np.deg2rad(np.linspace(-24.0, 24.0, BOX_H))[:, None]
    az = (2 * np.pi * (np.arange(BOX_W) + 0.5) / BOX_W)[None, :]
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1).reshape(-1, 3)
    r = _box_ranges(d)
    assert r.min() > 2 * BOX_MIN and r.max() < 0.9 * BOX_RANGE
    return [((r + rng.normal(0.0, 0.01, len(r)))[:, None] * d).astype(np.float32) for _ in range(BOX_N)]


BOX_P_TWO_CLASSES = 6  # two block classes need 5 points per voxel at least; with 6 a voxel outgrows its 5-point block before it is full


@functools.lru_cache(maxsize=None)
def box_reference(P=BOX_P):
    """the oracle's run of the box with P points per voxel: poses, statistics, the final map, and per sweep (frame_downsample points, of those
    dropped at a full voxel)"""
    orc.set_threads(1)
    ref = orc.ICP(BOX_RANGE, BOX_MIN, **dict(BOX_ICP, max_points_per_voxel=P))
    poses, per_sweep = [], []
    for f in box_sweeps():
        before = ref.map.points() if ref.map.num_points else np.zeros((0, 3))
        T = ref.register_frame(f.astype(np.float64), None)
        fd = ref.last_frame_down()
        per_sweep.append((len(fd), count_dropped(before, fd @ T[:3, :3].T + T[:3, 3], BOX_ICP["voxel_size"], P)))
        poses.append(T)
    pts = ref.map.points()
    return dict(poses=np.array(poses), stats=ref.stats, map=pts, per_sweep=per_sweep, size=(ref.map.num_voxels, ref.map.num_points))


# ------------------------------------------------------------------------------------------------ a flat wall close to the sensor
WALL_H, WALL_W = 16, 256


@functools.lru_cache(maxsize=None)
def wall_sweep():
    """one sweep of WALL_H x WALL_W float32 points on the wall x = 2 m, columns 1.6 cm apart: consecutive points of a beam share their
    0.5 m voxel of down-sampling pass 1 in runs of about thirty, so most points of a wavefront are no run head"""
    el = np.deg2rad(np.linspace(-30.0, 30.0, WALL_H))[:, None]
    az = np.deg2rad(np.linspace(-60.0, 60.0, WALL_W))[None, :]
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1).reshape(-1, 3)
    return (d * (2.0 / d[:, :1])).astype(np.float32)
