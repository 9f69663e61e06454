"""Single sweeps whose frame_downsample has a chosen length, for the block boundaries of the two voxel down-sampling passes (pure numpy +
the CPU oracle; no GPU).

The winners of a pass are counted per block and compacted behind the sum of the blocks before (csrc/icp_kernels.h d_count_winners,
d_compact_winners): pass 1 over the n_in points of the sweep, pass 2 over the n_down entries of frame_downsample.  The drivers with one launch
per stage walk blocks of STAGE_BLOCK points, the free-running kernel blocks of FREE_BLOCK.  A sweep here has exactly m returns, each at the
centre of a 0.5 m voxel of its own (voxel size 1.0), everything else is "no return": n_valid = n_down = m, so pass 2 walks m entries - one
block exactly full at m = block, one entry short of it, or a second block with a single entry.  Two arrangements:
  spread   the returns at m random places of the sweep, in the order of CELLS
  packed   the returns are the last m points of the sweep, behind blocks without a single return (an offset over empty blocks, a look-back
           over zero counts); all in the last block of pass 1 up to m = block, one in the block before at m = block + 1
The cells fill whole 1 m map voxels, eight to a voxel, more than MAX_POINTS_PER_VOXEL: the sweep that follows (follow_up) meets full voxels.
tests/test_downsample_scenes_cpu.py shows with the oracle alone that the scenes are what they claim;
tests/test_gpu_downsample_edges.py holds the device against them.
"""
import functools

import numpy as np

from oracle import cpu as orc

H, W = 16, 1024
N = H * W
VOXEL_SIZE, MAX_POINTS_PER_VOXEL, MAX_RANGE, MIN_RANGE = 1.0, 4, 40.0, 0.5
ICP = dict(voxel_size=VOXEL_SIZE, deskew=0, max_points_per_voxel=MAX_POINTS_PER_VOXEL)
STAGE_BLOCK = 256       # one launch per stage: 256 threads, one point each
FREE_BLOCK = 512 * 16   # free-running kernel: 512 threads, SEQ_U2 = 16 points each in K3 / K3b / K4 (csrc/seq_kernel.h)
COUNTS = tuple(b + d for b in (STAGE_BLOCK, FREE_BLOCK) for d in (-1, 0, 1))
ARRANGEMENTS = ("spread", "packed")
SCENES = tuple((m, a) for m in COUNTS for a in ARRANGEMENTS)


def _cells():
    """centres of the 0.5 m cells of the map voxels [2, 20) x [1, 9) x [1, 9), voxel by voxel; within a voxel the four cells of even parity
    first (the four points the map keeps of it lie on a tetrahedron, not on one face).  Dyadic, exact in float32."""
    vox = np.stack(np.meshgrid(np.arange(2, 20), np.arange(1, 9), np.arange(1, 9), indexing="ij"), axis=-1).reshape(-1, 3)
    sub = np.array([(a, b, c) for par in (0, 1) for a in (0, 1) for b in (0, 1) for c in (0, 1) if (a + b + c) % 2 == par])
    return (vox[:, None, :] + 0.25 + 0.5 * sub[None, :, :]).reshape(-1, 3)


CELLS = _cells()
assert len(CELLS) > max(COUNTS)


def places(m, arrangement):
    """indices of the m returns within the sweep, ascending"""
    if arrangement == "packed":
        return np.arange(N - m, N)
    return np.sort(np.random.default_rng(m).choice(N, m, replace=False))


def sweep(m, arrangement):
    """(N, 3) float32: CELLS[:m] at places(m, arrangement), zeros (no return) elsewhere"""
    f = np.zeros((N, 3), dtype=np.float32)
    f[places(m, arrangement)] = CELLS[:m]
    return f


def follow_up(m):
    """an ordinary sweep over the same m cells: every point a return, up to 0.2 m off its cell's centre on every axis"""
    rng = np.random.default_rng(1000 + m)
    return (CELLS[np.arange(N) % m] + rng.uniform(-0.2, 0.2, (N, 3))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(m, arrangement):
    """the oracle's run of sweep(m, arrangement) and follow_up(m): per scan (frame_downsample, source), the statistics, and the map points
    after the first scan"""
    orc.set_threads(1)
    ref = orc.ICP(MAX_RANGE, MIN_RANGE, **ICP)
    clouds, map0 = [], None
    for f in (sweep(m, arrangement), follow_up(m)):
        ref.register_frame(f.astype(np.float64), None)
        clouds.append((ref.last_frame_down(), ref.last_source()))
        if map0 is None:
            map0 = ref.map.points()
    return dict(clouds=clouds, stats=ref.stats, poses=np.array(ref.poses()), map0=map0)
