"""The scenes of tests/helpers/full_voxel_scenes.py are what they claim - shown with numpy and the CPU oracle alone, so that
tests/test_gpu_map_full_voxels.py tests the full-voxel path of the map update and not something else."""
import numpy as np

from tests.helpers import full_voxel_scenes as fv
from tests.helpers import hash_scenes as hs


def _keys(x):
    return hs.pack_key(hs.voxel_of(x, 1.0))


def test_stage_scene_has_every_case():
    sc = fv.stage_scene()
    b1, b2, b3 = sc["batches"]
    full, two, one, new, col = (hs.pack_key(sc[k]) for k in ("full", "two", "one", "new", "colliding"))
    k1, cnt1 = np.unique(_keys(b1), return_counts=True)
    assert set(k1[cnt1 == 3]) == set(full) and set(k1[cnt1 == 2]) == set(two) and set(k1[cnt1 == 1]) == set(one)
    assert len(np.unique(np.concatenate([full, two, one, new]))) == len(full) + len(two) + len(one) + len(new)
    # more colliding voxels than the 16 slots they home on, all of them full
    home = hs.brick_slot(col, fv.STAGE_CAP - 1)
    assert len(col) == fv.N_COLLIDING and len(np.unique(home)) <= 16 and np.isin(col, full).all()
    k2 = _keys(b2)
    assert 1024 <= len(b2) <= fv.STAGE_N_MAX and len(b2) % 256 != 0
    assert np.isin(k2[:2 * fv.WAVE], full).all()                       # a run of 128 points that meet full voxels only
    w = k2[2 * fv.WAVE:3 * fv.WAVE]                                    # the mixed wavefront
    assert np.isin(w, full).sum() >= 16 and np.isin(w, one).any() and np.isin(w, new).sum() >= 16
    assert (w == two[0]).sum() == 3                                    # three candidates for a voxel one short of full
    assert (w == new[0]).sum() == 6 and (w == new[1]).sum() == 5       # several points of one new voxel inside one wavefront
    assert np.isin(col, k2).all()                                      # every full voxel behind a collision is asked for
    # the third call touches full voxels that its prune then takes, and full voxels that stay
    k3 = _keys(b3)
    far = sc["full_far"]
    assert far.sum() >= 10 and (~far).sum() >= 10 and np.isin(full, k3).all()
    ref = fv.stage_oracle(sc)
    assert ref[0][2] == 0 and ref[1][2] == np.isin(k2, full).sum() > len(b2) // 2
    assert ref[2][2] >= 2 * far.sum() and ref[2][0][0] < ref[1][0][0]  # points dropped at voxels the same call's prune removed
    # the voxel one short of full took exactly one of its three candidates - the first in scan order
    got = ref[1][1][_keys(ref[1][1]) == two[0]]
    first = b2[np.flatnonzero(k2 == two[0])[0]]
    assert len(got) == fv.STAGE_P and (got == first).all(axis=1).sum() == 1


def test_box_fills_at_once():
    """at least half of the frame_downsample points of the last three sweeps meet a full voxel (in fact nearly all, from the second sweep
    on); the second sweep still mixes full and filling voxels"""
    for P in (fv.BOX_P, fv.BOX_P_TWO_CLASSES):
        ref = fv.box_reference(P)
        per = ref["per_sweep"]
        assert len(per) == fv.BOX_N and per[0][1] == 0
        assert all(2 * d >= n for n, d in per[-3:]), per
        assert 0.5 * per[1][0] < per[1][1] < 0.9 * per[1][0], per[1]
        assert all(s["n_down"] == n for s, (n, _) in zip(ref["stats"], per))
        assert all(s["iterations"] >= 2 for s in ref["stats"][1:]) and np.abs(ref["poses"][:, :3, 3]).max() < 0.1
    # six points per voxel: voxels pass the five points of a small block on their way to full (the two-block-class run migrates them)
    assert fv.box_reference(fv.BOX_P_TWO_CLASSES)["size"][1] > 5 * fv.box_reference(fv.BOX_P_TWO_CLASSES)["size"][0]


def test_wall_has_long_runs():
    f = fv.wall_sweep().astype(np.float64)
    k = hs.pack_key(hs.voxel_of(f, 0.5))
    heads = 1 + int((k[1:] != k[:-1]).sum())
    assert len(f) == fv.WALL_H * fv.WALL_W and heads < len(f) // 12
