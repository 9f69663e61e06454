"""The device's voxel index (csrc/icp_kernels.h voxel_index) restated in numpy against (int)(x / vs) by C truncation, on the coordinates
where the two could part: k * vs and its neighbours up to 4 ulp either side.  The product x * (1 / vs) is truncated, and the real division
decides wherever the product lies within 1e-9 (|q| + 1) of an integer; the device evaluates that division behind a branch taken per
wavefront.  Shown here without a GPU: the restatement equals the truncated quotient everywhere, every such coordinate reaches the
fallback, and for the sizes whose reciprocal is not exact the fallback DECIDES indices (the plain truncation of the product is wrong there).

Then the scenes of tests/helpers/voxel_face_scenes.py, which tests/test_gpu_voxel_faces.py holds the device to: which lanes of which
wavefront reach the fallback, that it decides indices in the float64 scene, that the oracle alone gives the clouds an independent numpy
down-sampling expects, and that the second sweep's registration carries source points across faces of the map without ending near one."""
import numpy as np
import pytest

from oracle import icp_numpy as inp
from tests.helpers import voxel_face_scenes as vf

VOXEL_SIZES = (0.7, 0.35, 1.05, 0.5, 0.1, 1.5 * 0.7)  # a map voxel, its pass-1 voxel, pass 2 as a literal and as the device forms it; dyadic; small
K = np.arange(-2000, 2001)


def device_voxel_index(x, vs):
    """(index, reached the fallback, index without it)"""
    q = x * (1.0 / vs)
    plain = np.trunc(q).astype(np.int64)
    near = np.abs(q - np.rint(q)) <= 1e-9 * (np.abs(q) + 1.0)
    return np.where(near, np.trunc(x / vs).astype(np.int64), plain), near, plain


def boundary_coordinates(vs):
    """k * vs and the doubles 1 .. 4 ulp either side, k = -2000 .. 2000"""
    x0 = K * vs
    out = [x0]
    for direction in (np.inf, -np.inf):
        x = x0
        for _ in range(4):
            x = np.nextafter(x, direction)
            out.append(x)
    return np.concatenate(out)


@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_restatement_equals_the_truncated_quotient_on_the_boundaries(vs):
    x = boundary_coordinates(vs)
    got, near, plain = device_voxel_index(x, vs)
    want = (x / vs).astype(int)  # C truncation
    assert np.array_equal(got, want)
    assert near.all()  # every one of these coordinates takes the division
    decided = int((plain != want).sum())
    if vs == 0.5:
        assert decided == 0  # (an exact reciprocal: the product IS the quotient)
    else:
        assert decided > 100, decided  # the division, not the product, gives the index


@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_restatement_equals_the_truncated_quotient_away_from_the_boundaries(vs):
    rng = np.random.default_rng(3)
    x = rng.uniform(-2000 * vs, 2000 * vs, 200000)
    got, near, _ = device_voxel_index(x, vs)
    assert np.array_equal(got, (x / vs).astype(int))
    assert near.mean() < 1e-4  # practically no lane


# ------------------------------------------------------------------------------------------------ the scenes
def test_sweep0_wavefronts_take_the_branch_not_at_all_partly_and_fully():
    f = vf.sweep0()
    assert f.shape == (vf.N, 3) and f.dtype == np.float32 and vf.N <= 4096
    valid = f.any(axis=1)
    near = (vf.near_any(f.astype(np.float64)) & valid).reshape(-1, vf.WAVE).sum(axis=1)
    assert near[0] == 0 and near[1] == vf.WAVE
    assert ((near[2:] >= 3) & (near[2:] <= 6)).all(), near
    assert np.array_equal(near, vf.face_lanes().reshape(-1, vf.WAVE).sum(axis=1))  # the face lanes and nobody else
    assert (~valid).sum() == 40 and valid[:2 * vf.WAVE].all()
    r = np.linalg.norm(f[valid].astype(np.float64), axis=1)
    assert vf.MIN_RANGE < r.min() and r.max() < vf.MAX_RANGE
    p = f[vf.face_lanes()].astype(np.float64)
    assert (p < 0).any() and (p > 0).any() and (p == 0).any()
    for vs in vf.SIZES:  # faces of every size are met ...
        assert vf.near(p, vs).any(axis=1).sum() > 100, vs
    # ... and next to them sit float32 neighbours of a face, which do not reach the fallback
    beside = np.abs(p - np.rint(p * 2) / 2) < 1e-5
    assert (beside & ~vf.near(p, 0.5)).sum() > 50


@pytest.mark.parametrize("sweep", (vf.sweep0, vf.sweep1))
def test_the_float32_scenes_reach_the_fallback(sweep):
    x = sweep().astype(np.float64).ravel()
    for vs in vf.SIZES:
        got, near, plain = device_voxel_index(x, vs)
        assert np.array_equal(got, (x / vs).astype(int))
        assert near.sum() > 100
        assert np.array_equal(plain, got)  # (exact faces: reached, and the product was right)


def test_the_fallback_decides_indices_in_the_float64_scene():
    p = vf.sweep0_f64()
    valid = p.any(axis=1)
    reach = np.zeros(vf.N, dtype=bool)
    for vs in vf.SIZES_F64:
        got, near, plain = device_voxel_index(p.ravel(), vs)
        assert np.array_equal(got, (p.ravel() / vs).astype(int))
        assert near.sum() > 400
        if vs != vf.SIZES_F64[1]:  # (pass 2's 1.05 m: reached; within 12 m of the origin its product happens to truncate right)
            assert (plain != got).sum() >= 20, (vs, (plain != got).sum())  # pass 1 and the map: wrong without the division
        reach |= near.reshape(-1, 3).any(axis=1)
    assert np.array_equal((reach & valid).reshape(-1, vf.WAVE).sum(axis=1), vf.face_lanes().reshape(-1, vf.WAVE).sum(axis=1))
    ref = vf.reference_f64()
    r = np.linalg.norm(p, axis=1)
    fd = inp.voxel_downsample(p[(r < vf.MAX_RANGE) & (r > vf.MIN_RANGE)], vf.SIZES_F64[0])
    assert np.array_equal(ref["clouds"][0][0], fd) and np.array_equal(ref["clouds"][0][1], inp.voxel_downsample(fd, vf.SIZES_F64[1]))


def test_the_oracle_alone_gives_the_expected_clouds():
    ref = vf.reference()
    for k, sweep in enumerate((vf.sweep0, vf.sweep1)):
        p = sweep().astype(np.float64)
        r = np.linalg.norm(p, axis=1)
        valid = p[(r < vf.MAX_RANGE) & (r > vf.MIN_RANGE)]
        fd = inp.voxel_downsample(valid, vf.SIZES[0])
        src = inp.voxel_downsample(fd, vf.SIZES[1])
        st = ref["stats"][k]
        assert (st["n_valid"], st["n_down"], st["n_src"]) == (len(valid), len(fd), len(src)), st
        assert len(src) < len(fd) < len(valid) == vf.N - 40
        assert np.array_equal(ref["clouds"][k][0], fd) and np.array_equal(ref["clouds"][k][1], src)  # bit for bit


def test_sweep1_carries_source_points_across_map_faces_and_ends_away_from_them():
    ref = vf.reference()
    st, T = ref["stats"][1], ref["poses"][1]
    assert st["iterations"] >= 3 and st["n_corr_last"] > 2000, st
    D = np.linalg.inv(vf.motion()) @ T
    assert np.linalg.norm(D[:3, 3]) < 0.03  # the registration finds the motion (to what 4096 points, a fifth of them new, allow)
    src = ref["clouds"][1][1]
    end = src @ T[:3, :3].T + T[:3, 3]
    crossed = (inp.voxel_index(src, vf.VOXEL_SIZE) != inp.voxel_index(end, vf.VOXEL_SIZE)).any(axis=1)
    assert crossed.sum() > 300, crossed.sum()  # the Gauss-Newton iterations start in one map voxel and end in another
    # no point of the sweep ends within 1e-6 m of a face of the map or of a 27-voxel neighbourhood: device and oracle, whose poses
    # differ by rounding, decide alike
    fd = ref["clouds"][1][0]
    end = fd @ T[:3, :3].T + T[:3, 3]
    assert np.abs(end - np.rint(end)).min() > 1e-6
    # the sweep's face lanes: in the sensor frame, where the down-samplings and the first search's key are computed
    at, _ = vf.crossers()
    p = vf.sweep1().astype(np.float64)
    assert vf.near_any(p[vf.face_lanes()]).all() and not vf.near_any(p[at]).any()
