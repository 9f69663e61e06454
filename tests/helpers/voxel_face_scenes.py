"""Two sweeps whose points sit ON the faces of the voxels - for the exact-division fallback of the device's voxel index (pure numpy + the
CPU oracle; no GPU).

csrc/icp_kernels.h voxel_index truncates x * (1 / vs) and evaluates the real division x / vs only where that product lies within
1e-9 (|q| + 1) of an integer; the division sits behind a branch that a wavefront takes when ANY of its lanes is that near.  The sweeps
here decide, wavefront by wavefront (64 consecutive points), how many lanes are: none, a few, all 64.

Voxel size 1.0: pass 1 of the down-sampling works on 0.5 m voxels, pass 2 on 1.5 m, the map on 1.0 m - all three exact in float32, which
is what the sequence and batch runners take (a float32 coordinate that is NOT exactly k * vs is at least 6e-8 |x| away from it: far
outside the tolerance).  On such exact faces the fallback is REACHED and returns what the product gave: (k vs) (1 / vs) rounds to k whenever
k vs is exact.  It changes the index where k * vs is itself rounded, i.e. in float64 with sizes like 0.35: sweep0_f64().

  sweep0()     N = 4096 points = 64 wavefronts.  Every point starts in the middle of a 0.5 m cell of its own (quarter coordinates, a
               dyadic jitter: at least 1/16 m from every face of all three sizes).  A FACE lane gets one, two or three coordinates
               replaced by k * 0.5, k * 1.5 or k * 1.0 (within 12 m, k of both signs, +-0 included) - or by the float32 value 1, 2, 3 ulp either side
               of one: next to the face, outside the tolerance.  Wavefront 0: no face lane.  Wavefront 1: all 64.  Every other one:
               three to six, at varying lanes; a few lanes elsewhere hold "no return".
  sweep1()     the sweep that follows, from a sensor that has moved by MOTION: the quiet points of sweep 0 (none of its face points - their
               images would land within rounding of a face of the map, where device and oracle may differ), points that sit
               CROSS_MARGIN beyond a map face and start on its other side (the Gauss-Newton iterations carry them across: phase A's and
               the search's key change), and - in the SENSOR frame, where both down-samplings and the first search work - face lanes as in
               sweep 0 (their images in the map are generic).
  sweep0_f64() the lanes of sweep 0 with 0.7 m voxels in float64, for the per-call handle: the coordinates where the fallback changes the index.
tests/test_voxel_index_cpu.py shows with numpy and the oracle alone that the scenes are what they claim; tests/test_gpu_voxel_faces.py
holds the device against them.
"""
import functools

import numpy as np

from oracle import cpu as orc

H, W = 4, 1024
N = H * W
WAVE = 64
VOXEL_SIZE, MAX_RANGE, MIN_RANGE = 1.0, 40.0, 0.5
SIZES = (0.5 * VOXEL_SIZE, 1.5 * VOXEL_SIZE, VOXEL_SIZE)  # pass 1, pass 2, map
ICP = dict(voxel_size=VOXEL_SIZE, deskew=0)
REACH = 12.0  # the faces of a scene lie within this of the origin on every axis
CROSS_MARGIN = 0.03125  # a crosser ends this far beyond its face ...
MOTION_T = np.array([0.09375, -0.078125, 0.0625])  # ... and starts |MOTION_T| - CROSS_MARGIN before it (the rotation moves a point 0.011 m at most)
MOTION_R = np.array([2e-4, -3e-4, 4e-4])  # rotation vector, rad: nothing stays dyadic after it


def near(x, vs):
    """the device's test: does x * (1 / vs) lie within the tolerance of an integer?  (float64, elementwise)"""
    q = np.asarray(x, dtype=np.float64) * (1.0 / vs)
    return np.abs(q - np.rint(q)) <= 1e-9 * (np.abs(q) + 1.0)


def near_any(p):
    """per point: is any coordinate near a face of any of the three sizes?"""
    return np.any([near(p, vs).any(axis=1) for vs in SIZES], axis=0)


def _quiet(rng, n):
    """n points in cells of their own: (j + 1/2) / 2 on every axis, j in [-24, 24), plus a multiple of 1/64 in [-3/16, 3/16]; range > 1"""
    cells = np.stack(np.meshgrid(*[np.arange(-24, 24)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = cells[np.linalg.norm(0.5 * cells + 0.25, axis=1) > 1.5]
    c = cells[rng.choice(len(cells), n, replace=False)]
    return 0.5 * c + 0.25 + rng.integers(-12, 13, (n, 3)) / 64.0


def _face_values(rng, n, sizes, dtype):
    """n coordinates on a face of one of the three sizes (half of them), or 1 .. 3 ulp (of dtype) beside one"""
    size = np.array(sizes)[rng.integers(0, 3, n)]
    k = np.rint(rng.uniform(-1, 1, n) * np.floor(REACH / size))
    v = (k * size).astype(dtype)
    v[(k == 0) & (rng.random(n) < 0.5)] = dtype(-0.0)
    steps = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 4, n) * rng.choice((-1, 1), n))
    for s in range(1, 4):
        up, down = steps >= s, steps <= -s
        v[up] = np.nextafter(v[up], dtype(np.inf))
        v[down] = np.nextafter(v[down], dtype(-np.inf))
    return v.astype(np.float64)


def _put_faces(rng, p, lanes, sizes=SIZES, dtype=np.float32):
    """p[lanes]: one to three coordinates replaced by face values, the first of them EXACTLY on a face (as exactly as k * size is formed)"""
    for i in lanes:
        axes = rng.permutation(3)[: rng.integers(1, 4)]
        v = _face_values(rng, len(axes), sizes, dtype)
        size = sizes[rng.integers(0, 3)]
        v[0] = int(rng.integers(-int(REACH / size), int(REACH / size) + 1)) * size
        p[i, axes] = v
    return p


def face_lanes():
    """which points of a sweep are face lanes: wavefront 0 none, wavefront 1 all, every other one 3 .. 6 at varying lanes"""
    rng = np.random.default_rng(7)
    m = np.zeros(N, dtype=bool)
    m[WAVE:2 * WAVE] = True
    for w in range(2, N // WAVE):
        m[w * WAVE + rng.choice(WAVE, rng.integers(3, 7), replace=False)] = True
    return m


def no_return_lanes():
    """a few points without a return, none of them a face lane, none in wavefronts 0 and 1"""
    rng = np.random.default_rng(8)
    at = rng.choice(np.flatnonzero(~face_lanes())[WAVE:], 40, replace=False)
    m = np.zeros(N, dtype=bool)
    m[at] = True
    return m


@functools.lru_cache(maxsize=None)
def sweep0():
    rng = np.random.default_rng(70)
    p = _put_faces(rng, _quiet(rng, N), np.flatnonzero(face_lanes()))
    p[no_return_lanes()] = 0.0
    f = p.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), p)  # exact in float32
    f.setflags(write=False)
    return f


VOXEL_SIZE_F64 = 0.7
SIZES_F64 = (0.5 * VOXEL_SIZE_F64, 1.5 * VOXEL_SIZE_F64, VOXEL_SIZE_F64)


@functools.lru_cache(maxsize=None)
def sweep0_f64():
    """the same lanes with 0.7 m voxels, in float64 (the per-call handle takes it): k * 0.35, k * 1.05, k * 0.7 are rounded, their
    neighbours 1 .. 3 ulp either side lie inside the tolerance as well, and the product with the rounded reciprocal truncates to the
    wrong index for many of them - here the division DECIDES"""
    rng = np.random.default_rng(72)
    p = _put_faces(rng, VOXEL_SIZE_F64 * _quiet(rng, N), np.flatnonzero(face_lanes()), SIZES_F64, np.float64)
    p[no_return_lanes()] = 0.0
    p.setflags(write=False)
    return p


def motion():
    """sensor pose of sweep 1 in the frame of sweep 0 (= the map)"""
    T = np.eye(4)
    T[:3, :3] = _rodrigues(MOTION_R)
    T[:3, 3] = MOTION_T
    return T


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def crossers():
    """indices (into sweep 1) of the points built to cross a map face, and the axis each crosses on"""
    rng = np.random.default_rng(9)
    at = np.sort(rng.choice(np.flatnonzero(~face_lanes() & ~no_return_lanes()), 600, replace=False))
    return at, rng.integers(0, 3, len(at))


@functools.lru_cache(maxsize=None)
def sweep1():
    rng = np.random.default_rng(71)
    quiet0 = sweep0().astype(np.float64)
    world = np.where((face_lanes() | no_return_lanes())[:, None], _quiet(rng, N), quiet0)  # in the map's frame
    at, axis = crossers()
    # the registration starts from the identity, i.e. with the point at (nearly) world - MOTION_T, and ends with it at world: CROSS_MARGIN
    # above the lower face of its map voxel where the motion is positive, below the upper face where it is negative
    k = np.floor(world[at, axis])
    world[at, axis] = np.where(MOTION_T[axis] > 0, k + CROSS_MARGIN, k + 1.0 - CROSS_MARGIN)
    T = motion()
    p = (world - T[:3, 3]) @ T[:3, :3]  # sensor frame
    p = _put_faces(rng, p.astype(np.float32).astype(np.float64), np.flatnonzero(face_lanes()))
    p[no_return_lanes()] = 0.0
    f = p.astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference():
    """the oracle's run of the two sweeps: per scan (frame_downsample, source), the statistics, the poses"""
    orc.set_threads(1)
    ref = orc.ICP(MAX_RANGE, MIN_RANGE, **ICP)
    clouds = []
    for f in (sweep0(), sweep1()):
        ref.register_frame(f.astype(np.float64), None)
        clouds.append((ref.last_frame_down(), ref.last_source()))
    return dict(clouds=clouds, stats=ref.stats, poses=np.array(ref.poses()))


@functools.lru_cache(maxsize=None)
def reference_f64():
    """the oracle's run of sweep0_f64(): (frame_downsample, source), the statistics, the sorted map points"""
    orc.set_threads(1)
    ref = orc.ICP(MAX_RANGE, MIN_RANGE, voxel_size=VOXEL_SIZE_F64, deskew=0)
    ref.register_frame(sweep0_f64(), None)
    m = ref.map.points()
    return dict(clouds=[(ref.last_frame_down(), ref.last_source())], stats=ref.stats, map0=m[np.lexsort(m.T[::-1])])
