"""The scenes of tests/helpers/downsample_scenes.py are what they claim - shown with numpy and the CPU oracle alone, so that
tests/test_gpu_downsample_edges.py tests the block boundaries of the two down-sampling passes and not something else."""
import numpy as np
import pytest

from tests.helpers import downsample_scenes as ds
from tests.helpers import full_voxel_scenes as fv
from tests.helpers import hash_scenes as hs


def test_the_counts_sit_on_both_drivers_block_boundaries():
    assert ds.COUNTS == (255, 256, 257, 8191, 8192, 8193) and len(ds.SCENES) == 12
    half = hs.pack_key(hs.voxel_of(ds.CELLS, 0.5 * ds.VOXEL_SIZE))
    assert len(np.unique(half)) == len(ds.CELLS)                      # every cell a voxel of pass 1 of its own
    r = np.linalg.norm(ds.CELLS, axis=1)
    assert ds.MIN_RANGE < r.min() and r.max() < ds.MAX_RANGE          # inside the range gates
    assert np.array_equal(ds.CELLS.astype(np.float32).astype(np.float64), ds.CELLS)


@pytest.mark.parametrize("m,arrangement", ds.SCENES)
def test_scene_has_exactly_the_chosen_frame_downsample(m, arrangement):
    f = ds.sweep(m, arrangement)
    at = np.flatnonzero(f.any(axis=1))
    assert f.shape == (ds.N, 3) and len(at) == m
    if arrangement == "packed":
        # the last m points; every block before them, of either driver, is empty
        assert at[0] == ds.N - m and not f[: (ds.N - m) // ds.STAGE_BLOCK * ds.STAGE_BLOCK].any()
        assert (ds.N - m) // ds.STAGE_BLOCK >= 1
    else:
        # winners in the first and the last block of both drivers, and no block boundary of pass 1 that all of them sit behind
        assert at[0] < ds.STAGE_BLOCK and at[-1] >= ds.N - ds.STAGE_BLOCK
        assert (np.bincount(at // ds.FREE_BLOCK, minlength=ds.N // ds.FREE_BLOCK) > 0).all()
    ref = ds.reference(m, arrangement)
    st = ref["stats"][0]
    fd, src = ref["clouds"][0]
    assert st["n_valid"] == m and st["n_down"] == m == len(fd), (st, len(fd))
    assert 0 < st["n_src"] == len(src) < st["n_down"], st
    assert np.array_equal(fd, ds.CELLS[:m])                           # frame_downsample = the returns, in scan order
    # the map keeps MAX_POINTS_PER_VOXEL of the eight cells of a voxel, and the sweep that follows meets those full voxels
    _, per_voxel = np.unique(hs.pack_key(hs.voxel_of(ref["map0"], ds.VOXEL_SIZE)), return_counts=True)
    assert per_voxel.max() == ds.MAX_POINTS_PER_VOXEL and (per_voxel == ds.MAX_POINTS_PER_VOXEL).sum() >= m // 8
    fd1, src1 = ref["clouds"][1]
    T = ref["poses"][1]
    assert fv.count_dropped(ref["map0"], fd1 @ T[:3, :3].T + T[:3, 3], ds.VOXEL_SIZE, ds.MAX_POINTS_PER_VOXEL) > len(fd1) // 2
    assert ref["stats"][1]["n_valid"] == ds.N and 0 < len(src1) < len(fd1) <= m
    assert ref["stats"][1]["iterations"] >= 1 and ref["stats"][1]["n_corr_last"] > 0
