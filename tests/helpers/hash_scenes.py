"""Scenes on which collisions, long probe chains, the cyclic wrap and tombstones of the voxel hash tables are the rule (pure numpy; no GPU,
no oracle).

The hash of csrc/icp_kernels.h is deterministic: `pack_key`, `mix64`, `brick_slot` and the host's `vds_table_slots` are restated here, so a
test can choose voxels that all home on the same 128-byte lines of a small table.  `Table` mirrors the device's open-addressing rules (linear
probing from the home slot, a search walks past tombstones, an insert never reuses one, `used` grows by one per created entry and only a
rebuild resets it), `MapSim` the map on top of it (a voxel lives from its first point until a prune finds that point too far away).
tests/test_hash_scenes_cpu.py proves the scenes are what they claim; tests/test_gpu_hash_tables.py compares the device's tables, dumped with
ptl_icp_debug_table, with the simulator's - which pins this restatement - and its results with the CPU oracle's.

Coordinates are dyadic and well inside their voxels (voxel size 1.0: k + 0.25 / 0.5 / 0.75 as in lattice_scenes.py), so every
implementation sees exact keys.  A voxel index is (int)(x / size), truncation toward zero: voxel k >= 0 covers [k, k + 1) size, voxel
k < 0 covers (k - 1, k] size.
"""
import functools

import numpy as np

KEY_OFF = 1 << 20
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
TOMB_KEY = np.uint64(0xFFFFFFFFFFFFFFFE)
VDS1_SLOTS_PER_POINT, VDS2_SLOTS_PER_POINT = 64, 16
_LOW = np.uint64((1 << 42) | (1 << 21) | 1)


# ------------------------------------------------------------------------------------------------ the hash, restated
def pack_key(vox):
    """u64 key of voxel indices (..., 3): the three indices + 2^20 in 21 bits each, x highest"""
    o = (np.asarray(vox, dtype=np.int64) + KEY_OFF).astype(np.uint64)
    return (o[..., 0] << np.uint64(42)) | (o[..., 1] << np.uint64(21)) | o[..., 2]


def unpack_key(key):
    key = np.asarray(key, dtype=np.uint64)
    m = np.uint64((1 << 21) - 1)
    return np.stack([(key >> np.uint64(42)) & m, (key >> np.uint64(21)) & m, key & m], axis=-1).astype(np.int64) - KEY_OFF


def mix64(h):
    """the 64-bit finaliser of MurmurHash3 (fmix64)"""
    h = np.array(h, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    return h


def brick_slot(key, mask):
    """home slot of `key` in a table of mask + 1 slots: the 2 x 2 x 2 brick of voxels that agree in all but the lowest bit of each offset index
    shares the hash (of the key with those bits cleared, its low 32 bits shifted left by 3), the three low bits select the entry of the line"""
    key = np.asarray(key, dtype=np.uint64)
    fine = ((key >> np.uint64(42)) & np.uint64(1)) << np.uint64(2) | ((key >> np.uint64(21)) & np.uint64(1)) << np.uint64(1) | (key & np.uint64(1))
    h = (mix64(key & ~_LOW) & np.uint64(0xFFFFFFFF)) << np.uint64(3)
    return ((h | fine) & np.uint64(0xFFFFFFFF) & np.uint64(mask)).astype(np.int64)


def vds_table_slots(per_point, n):
    """slots of a per-scan voxel table of a handle for n points per scan: the power of two >= per_point * n, 1024 at least"""
    cap = 1024
    while cap < per_point * n:
        cap <<= 1
    return cap


def voxel_of(points, size):
    """(int)(x / size) per coordinate"""
    return np.trunc(np.asarray(points, dtype=np.float64) / size).astype(np.int64)


def points_in(vox, frac, size=1.0):
    """the points of voxels `vox` (n, 3) at the fractions `frac` (n, 3) in (0, 1) of the way through them, away from zero"""
    vox = np.asarray(vox, dtype=np.int64)
    return np.where(vox >= 0, vox + frac, vox - frac) * size


# ------------------------------------------------------------------------------------------------ the table, simulated
class Table:
    """open addressing as the device does it"""

    def __init__(self, cap):
        assert cap > 0 and cap & (cap - 1) == 0
        self.cap, self.mask = cap, cap - 1
        self.keys = np.full(cap, EMPTY_KEY, dtype=np.uint64)
        self.used = 0  # entries created since the last rebuild, tombstones included

    def home(self, key):
        return int(brick_slot(np.uint64(key), self.mask))

    def find(self, key):
        """slot of `key` or -1: walks past other voxels and tombstones, stops at an empty slot"""
        key = np.uint64(key)
        s = self.home(key)
        for _ in range(self.cap):
            k = self.keys[s]
            if k == key:
                return s
            if k == EMPTY_KEY:
                return -1
            s = (s + 1) & self.mask
        return -1

    def insert(self, key):
        """(slot, created): find-or-create; a new entry takes the first EMPTY slot of the walk, never a tombstone"""
        key = np.uint64(key)
        s = self.home(key)
        for _ in range(self.cap):
            k = self.keys[s]
            if k == key:
                return s, False
            if k == EMPTY_KEY:
                self.keys[s] = key
                self.used += 1
                return s, True
            s = (s + 1) & self.mask
        return -1, False

    def remove(self, key):
        s = self.find(key)
        assert s >= 0
        self.keys[s] = TOMB_KEY

    def rebuild(self, live_keys):
        self.keys[:] = EMPTY_KEY
        self.used = 0
        for k in live_keys:
            self.insert(k)

    # what a scene is judged by
    @property
    def exhausted(self):
        return self.used > self.cap // 4 * 3

    def occupied(self):
        return np.flatnonzero(self.keys != EMPTY_KEY)

    def tombstones(self):
        return int((self.keys == TOMB_KEY).sum())

    def live(self):
        """(slots, keys) of the live entries"""
        s = np.flatnonzero((self.keys != EMPTY_KEY) & (self.keys != TOMB_KEY))
        return s, self.keys[s]

    def chain_stats(self):
        """per live entry: displacement from its home slot (cyclic), whether its chain wrapped past slot 0, tombstones between home and slot"""
        s, k = self.live()
        home = brick_slot(k, self.mask)
        disp = (s - home) & self.mask
        tomb = np.concatenate([[0], np.cumsum(self.keys == TOMB_KEY)])
        between = np.where(s >= home, tomb[s] - tomb[home], tomb[self.cap] - tomb[home] + tomb[s])
        return disp, s < home, between


class MapSim:
    """the local map's table: which voxels exist, where they sit, what the counters say"""

    def __init__(self, cap, voxel_size=1.0, max_range=100.0):
        self.tab, self.vs, self.max_range = Table(cap), voxel_size, max_range
        self.first = {}  # key of a live voxel -> its first point

    def add(self, points):
        points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        keys = pack_key(voxel_of(points, self.vs))
        uk, ui = np.unique(keys, return_index=True)
        for k, i in zip(uk.tolist(), ui.tolist()):  # (return_index: the first occurrence = the first point in scan order)
            if k not in self.first:
                self.tab.insert(k)
                self.first[k] = points[i].copy()

    def prune(self, origin):
        """a voxel goes when its first point is farther than max_range from `origin` (strictly); its entry becomes a tombstone"""
        origin = np.asarray(origin, dtype=np.float64)
        for k, p in list(self.first.items()):
            d = p - origin
            if d[0] * d[0] + d[1] * d[1] + d[2] * d[2] > self.max_range * self.max_range:
                self.tab.remove(k)
                del self.first[k]

    def rebuild(self):
        self.tab.rebuild(list(self.first))

    @property
    def n_live(self):
        return len(self.first)


# ------------------------------------------------------------------------------------------------ voxels by home line
@functools.lru_cache(maxsize=8)
def _bricks(R):
    """brick indices [-R, R)^3 in scan order (x slowest) with the hash of each"""
    a = np.arange(-R, R, dtype=np.int64)
    g = np.meshgrid(a, a, a, indexing="ij")
    b = np.stack([x.reshape(-1) for x in g], axis=1)
    return b, mix64(pack_key(2 * b)) & np.uint64(0xFFFFFFFF)  # (2 b + 2^20 is even: the brick's key with the low bits cleared)


_FINE = np.array([[i >> 2 & 1, i >> 1 & 1, i & 1] for i in range(8)], dtype=np.int64)


def homing_voxels(cap, lines, R=32):
    """the voxels with brick index in [-R, R)^3 (voxel index in [-2 R, 2 R)^3) whose home slot lies on one of the 8-slot `lines` of a
    cap-slot table: brick by brick in scan order, the 8 voxels of a brick in the order of their entries of the line"""
    b, h = _bricks(R)
    line = ((h << np.uint64(3)) & np.uint64(cap - 1)) >> np.uint64(3)
    sel = b[np.isin(line.astype(np.int64), np.asarray(lines, dtype=np.int64))]
    return (2 * sel[:, None, :] + _FINE[None, :, :]).reshape(-1, 3)


def _fill(vox, rng, lo, hi, size=1.0):
    """lo..hi points in each voxel at fractions 0.25 / 0.5 / 0.75, voxel by voxel: (points, index of the voxel of each)"""
    n = rng.integers(lo, hi + 1, len(vox))
    own = np.repeat(np.arange(len(vox)), n)
    frac = rng.integers(1, 4, (len(own), 3)) * 0.25
    return points_in(vox[own], frac, size), own


def cluster_scene(cap, line, n_voxels=200, seed=0, lo=1, hi=3):
    """(voxels, points, owner): the first n_voxels voxels that home on lines `line` and `line` + 1 of a cap-slot table, 1..3 points in each
    (owner[i] = index of point i's voxel; the points come voxel by voxel)"""
    lines = cap // 8
    vox = homing_voxels(cap, [line % lines, (line + 1) % lines])[:n_voxels]
    assert len(vox) == n_voxels
    pts, own = _fill(vox, np.random.default_rng(seed), lo, hi)
    return vox, pts, own


def wrap_scene(cap, n_voxels=200, seed=0):
    """cluster_scene on the last two lines: the chain runs off the end of the table and goes on from slot 0"""
    return cluster_scene(cap, cap // 8 - 2, n_voxels, seed)


def absent_voxels(cap, line, skip, n):
    """n voxels that home on lines `line`, `line` + 1 like cluster_scene's, beyond its first `skip`: present in no scene"""
    lines = cap // 8
    return homing_voxels(cap, [line % lines, (line + 1) % lines])[skip:skip + n]


def dense_scene(cap, load, seed=0, R=32, exclude=None):
    """(voxels, points): int(load * cap) voxels drawn from [-2 R, 2 R)^3 without replacement (none of `exclude`), 1..25 points in each, all
    points in one shuffled order - a 20-point cap binds in some voxels, and a voxel's points arrive spread over the cloud"""
    rng = np.random.default_rng(seed)
    n = int(load * cap)
    flat = rng.choice((4 * R) ** 3, size=n + (0 if exclude is None else len(exclude)), replace=False)
    vox = np.stack([flat // (4 * R) ** 2, flat // (4 * R) % (4 * R), flat % (4 * R)], axis=1).astype(np.int64) - 2 * R
    if exclude is not None:
        vox = vox[~np.isin(pack_key(vox), pack_key(exclude))]
    vox = vox[:n]
    pts, _ = _fill(vox, rng, 1, 25)
    return vox, pts[rng.permutation(len(pts))]


def vds_scene(n_max, which, seed=0, n_bricks=32):
    """A sensor-frame cloud of at most n_max points (handle: voxel size 1.0, max_points_per_scan = n_max) whose voxels collide in the per-scan
    table of down-sampling pass `which`: 1 - voxels of 0.5 in the 64-slots-per-point table, 2 - voxels of 1.5 in the 16-slots-per-point table.
    n_bricks bricks (8 voxels each) that home on the last two lines: the chain wraps.  Every voxel of the pass holds four points in a shuffled
    order, so the first in scan order decides.  Pass 2: three of a voxel's four points lie in 0.5-voxels of their own (they survive pass
    1), the fourth shares the 0.5-voxel of one of them.
    Returns (points, voxels of the pass, voxel size of the pass, slots of its table)"""
    rng = np.random.default_rng(seed)
    size = 0.5 if which == 1 else 1.5
    cap = vds_table_slots(VDS1_SLOTS_PER_POINT if which == 1 else VDS2_SLOTS_PER_POINT, n_max)
    R = 64 if which == 1 else 32
    vox = homing_voxels(cap, [cap // 8 - 2, cap // 8 - 1], R)[:8 * n_bricks]
    assert len(vox) == 8 * n_bricks and 4 * len(vox) <= n_max
    own = np.repeat(np.arange(len(vox)), 4)
    off = np.empty((len(own), 3))  # distance from the voxel's face nearest to zero, per axis: dyadic
    for v in range(len(vox)):
        if which == 1:  # four distinct positions in the 0.5-voxel
            c = rng.choice(27, size=4, replace=False)
            off[4 * v:4 * v + 4] = (np.stack([c // 9, c // 3 % 3, c % 3], axis=1) + 1) * 0.125
        else:  # (j + f) * 0.5: j the 0.5-voxel along the axis, f = 0.25 / 0.5 / 0.75 of the way through it
            c = rng.choice(27, size=3, replace=False)
            j = np.stack([c // 9, c // 3 % 3, c % 3], axis=1)
            twin = int(rng.integers(0, 3))
            f = rng.integers(1, 4, (4, 3)) * 0.25
            while (f[3] == f[twin]).all():
                f[3] = rng.integers(1, 4, 3) * 0.25
            off[4 * v:4 * v + 4] = (np.concatenate([j, j[twin][None]]) + f) * 0.5
    pts = np.where(vox[own] >= 0, vox[own] * size + off, vox[own] * size - off)
    return pts[rng.permutation(len(pts))], vox, size, cap


# ------------------------------------------------------------------------------------------------ the teacher-forced map stage
def map_stage_scene(cap=1 << 12, seed=0, background=0.40):
    """The three steps of tests/test_gpu_hash_tables.py's map stage on a cap-slot table, as a dict:
      max_range, origin   the prune: a voxel goes when its first point is farther than max_range from origin
      batches             three ragged clouds, one call each.  Calls are ordered on the device, the points of one call are not: the colliding
                          voxels (a wrap scene and a cluster on an interior line) whose first point the prune will find too far away arrive
                          with the first call, those that stay with the second - so the tombstones stand in FRONT of the survivors wherever
                          the device puts the voxels of one call.  A dense background is spread over all three
      reinsert            new points into pruned voxels (they are created again behind their own tombstones), into survivors and into
                          background voxels
      colliding, absent   the colliding voxels; voxels that home on the same lines and never exist (the longest walk of a search)"""
    rng = np.random.default_rng(seed)
    line = cap // 16
    wv, wp, wo = wrap_scene(cap, 200, seed)
    cv, cp, co = cluster_scene(cap, line, 120, seed + 1)
    absent = np.concatenate([absent_voxels(cap, cap // 8 - 2, 200, 24), absent_voxels(cap, line, 120, 24)])
    vox = np.concatenate([wv, cv])
    pts, own = np.concatenate([wp, cp]), np.concatenate([wo, co + len(wv)])
    first = np.array([pts[own == v][0] for v in range(len(vox))])
    origin = np.array([8.0, -4.0, 2.0])
    dist = np.sqrt(((first - origin) ** 2).sum(axis=1))
    max_range = float(np.floor(np.median(dist)))
    far = dist > max_range
    bv, bp = dense_scene(cap, background, seed + 2, exclude=np.concatenate([vox, absent]))
    cut = [0, len(bp) // 3 + 1, 2 * len(bp) // 3 - 7, len(bp)]
    batches = [np.concatenate([pts[far[own]], bp[cut[0]:cut[1]]]), np.concatenate([bp[cut[1]:cut[2]], pts[~far[own]]]), bp[cut[2]:cut[3]]]
    again = np.concatenate([vox[far][::2], vox[~far][::2], bv[::7]])
    own2 = np.repeat(np.arange(len(again)), rng.integers(1, 5, len(again)))
    re_pts = points_in(again[own2], 0.125 + 0.25 * rng.integers(0, 4, (len(own2), 3)))  # fractions 1/8 .. 7/8: positions no earlier point has
    return dict(cap=cap, max_range=max_range, origin=origin, batches=batches, reinsert=re_pts[rng.permutation(len(re_pts))],
                colliding=vox, far=far, absent=absent, background=bv)


def exhaustion_steps(seed=0, per_step=96, n_steps=12):
    """Clouds of fresh voxels along +x, one per call, each pruned around its own centre so that most of what the earlier calls created goes:
    [(points, origin)], max_range.  Live voxels stay few, the tombstones pile up: without a rebuild `used` passes 3/4 of the table"""
    rng = np.random.default_rng(seed)
    steps = []
    for k in range(n_steps):
        centre = np.array([24 * k, 0, 0], dtype=np.int64)
        vox = centre + np.unique(rng.integers(-8, 8, (per_step, 3)), axis=0)
        pts, _ = _fill(vox, rng, 1, 3)
        steps.append((pts[rng.permutation(len(pts))], centre.astype(np.float64)))
    return steps, 30.0


# ------------------------------------------------------------------------------------------------ a drive that leaves its map behind
def drive_sequence(n_scans=24, H=16, W=512, max_range=12.0, seed=0, density=1.1):
    """(frames, positions): n_scans sensor-frame sweeps of H * W float32 points ((0, 0, 0) = no return) of a static cloud of random points
    in a corridor, seen from a sensor that accelerates along +x to 1 m per sweep over the first five sweeps and ends two ranges from where it
    began - most voxels ever created are pruned on the way.  A sweep holds the world points within 0.98 max_range of the sensor, in a shuffled
    order; coordinates are multiples of 1/256 m (exact in float32, and the sensor positions too, so a sweep is the world minus a position,
    exactly).  Random points have no ring pattern for the registration to lock on, and the constant-velocity prediction is never more
    than 0.25 m off"""
    rng = np.random.default_rng(seed)
    step = np.minimum(np.arange(n_scans), 4) * 0.25
    pos = np.stack([np.cumsum(step), np.zeros(n_scans), np.zeros(n_scans)], axis=1)
    lo, hi = np.array([-max_range - 1, -max_range, -4.0]), np.array([pos[-1, 0] + max_range + 1, max_range, 4.0])
    world = np.round(rng.uniform(lo, hi, (int(density * np.prod(hi - lo)), 3)) * 256.0) / 256.0
    frames = []
    for p in pos:
        x = world - p
        x = x[np.sqrt((x * x).sum(axis=1)) < 0.98 * max_range]
        assert 0 < len(x) <= H * W
        f = np.zeros((H * W, 3), dtype=np.float32)
        x = x[rng.permutation(len(x))]
        f[: len(x)] = x
        assert np.array_equal(f[: len(x)].astype(np.float64), x)
        frames.append(f)
    return frames, pos
