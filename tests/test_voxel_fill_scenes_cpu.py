"""tests/helpers/voxel_fill_scenes.py is what it claims (numpy + the CPU oracle, no GPU): the map's voxels hold exactly 0, 1, 7, 8, 9, 16,
17 and 20 points in the order written, the nearest stored point of the sweep's first iteration sits in every chunk and in every place of
the search, the exact ties are there - and the oracle alone passes the bars tests/test_gpu_voxel_fill.py asks of the device."""
import numpy as np

import ptudes_lab_amd  # noqa: F401  (import shim)
from oracle import cpu as orc
from tests.helpers import voxel_fill_scenes as vf


def test_the_scans_are_exact_and_the_map_is_the_points_as_written():
    fr = vf.frames()
    assert len(fr) == vf.MAP_SCANS + 1 and all(f.shape == (vf.N, 3) and f.dtype == np.float32 for f in fr)
    src = vf.source()
    assert len(np.unique(np.floor(src / (1.5 * vf.VOXEL_SIZE)), axis=0)) == vf.CELLS  # pass 2 of the down-sampling keeps every source point
    for f in fr[: vf.MAP_SCANS]:
        m = f[np.abs(f).sum(axis=1) > 0].astype(np.float64)
        assert len(np.unique(np.floor(m / (0.5 * vf.VOXEL_SIZE)), axis=0)) == len(m)  # ... and pass 1 every map point of every scan
        assert (m > 1.0).all() and np.linalg.norm(m, axis=1).max() < vf.MAX_RANGE
    ref = vf.reference()
    # the three map scans register at the identity EXACTLY (their source points lie on map points), so the map is what cells() wrote
    for k in range(vf.MAP_SCANS):
        assert np.array_equal(ref["poses"][k], np.eye(4)), k
    want = np.concatenate([o + p for o, vox in zip(vf.origins(), vf.cells()) for p in vf.stored(vox).values()])
    got = ref["map_points"]
    assert np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])])
    assert ref["stats"][vf.MAP_SCANS]["n_src"] == vf.CELLS and np.array_equal(ref["source"], src)
    # stored point 8 (16) of a voxel of more than 8 (16) is a copy of its point 0
    for vox in vf.cells()[:200]:
        for p in vf.stored(vox).values():
            for j in (8, 16):
                assert len(p) <= j or np.array_equal(p[j], p[0])


def test_the_fills_are_the_chunk_boundaries():
    fi = vf.first_iteration()
    assert set(np.unique(fi["fills"]).tolist()) == set(vf.FILLS)
    for n in vf.FILLS[1:]:
        assert (fi["fills"] == n).sum() >= 400, n
        assert (fi["fills"][:, 13] == n).sum() >= 50, n  # ... of the own voxel too
    assert (fi["fills"][:, 13] == 0).sum() >= 50  # and source points whose own voxel is absent


def test_where_the_nearest_stored_point_sits():
    fi, kind = vf.first_iteration(), vf.kinds()
    for name, n in vf.COUNTS.items():
        assert (kind == name).sum() == n
    # in chunk 0, 1 and 2 ...
    assert (np.bincount(fi["chunk"][fi["chunk"] >= 0], minlength=3) >= [500, 150, 20]).all()
    # ... in the own voxel, in each of the three other voxels of the first round (the third-nearest box is the idle slot's), in a survivor round
    place = np.bincount(fi["place"][fi["place"] >= 0], minlength=5)
    assert (place >= [500, 100, 50, 30, 30]).all(), place
    for c in (0, 1):
        assert (np.bincount(fi["place"][fi["chunk"] == c], minlength=5) >= 15).all(), c
    assert (np.bincount(fi["place"][fi["chunk"] == 2], minlength=5)[:2] >= 5).all() and (fi["place"][fi["chunk"] == 2] >= 2).sum() >= 3
    assert (fi["place"] == -1).sum() >= 5  # nothing stored in reach at all


def test_the_exact_ties():
    fi, kind = vf.first_iteration(), vf.kinds()
    k = lambda name: kind == name  # noqa: E731
    # inside one lane: point 0 of the own voxel and its copies at 8 (and 16)
    m = k("tie_lane")
    assert (fi["entry"][m] == 13).all() and (fi["index"][m] == 0).all() and (fi["copies"][m] >= 1).all() and (fi["copies"][m] == 2).sum() >= 20
    # across lanes of one voxel
    m = k("tie_lanes")
    assert (fi["entry"][m] == 13).all() and (fi["lanes"][m] == 1).all() and set(fi["index"][m].tolist()) == {0, 2, 3}
    # across voxels of one round, the id decides either way: - x (entry 4) beats the own voxel (13), the own voxel beats + x (22)
    m = k("tie_vox_lo")
    assert (fi["entry"][m] == 4).all() and (fi["other_entry"][m] == 13).all() and set(fi["index"][m].tolist()) == {0, 5, 11, 18}
    m = k("tie_vox_hi")
    assert (fi["entry"][m] == 13).all() and (fi["other_entry"][m] == 22).all()
    # the deep cells: second-, third- and fourth-nearest occupied box
    assert (np.bincount(fi["place"][k("deep")], minlength=5)[2:] >= 30).all()


def test_the_oracle_alone_passes_the_bars():
    """the oracle's pipeline against the registration restated with its pieces: the same iteration count, poses within 1e-9; and a second
    run of the pipeline bit for bit"""
    ref = vf.reference()
    it, T = vf.iterations()
    assert it == ref["stats"][vf.MAP_SCANS]["iterations"] >= 4
    D = np.linalg.inv(ref["poses"][vf.MAP_SCANS]) @ T
    assert np.linalg.norm(D[:3, 3]) <= 1e-9 and orc.rot_angle(D) <= 1e-9
    again = orc.ICP(vf.MAX_RANGE, vf.MIN_RANGE, **vf.ICP)
    for f in vf.frames():
        again.register_frame(f.astype(np.float64), None)
    assert np.array_equal(np.array(again.poses()), ref["poses"]) and again.stats == ref["stats"]
