"""Carve cases whose answers are computed by hand: one sweep of 1 x 8 pixels from a sensor with identity rotation at
`origin`; a pixel is its end in the sensor frame, (0, 0, 0) = no return.  Voxel size 0.5 and dyadic numbers, so every product, sum and
comparison of the definition is exact.  `expect`: (through, support) per stored point, in the order of `stored`; `counts`: the summary
entries the case pins.  tests/test_map_carve_cpu.py holds the restatement to these answers, tests/test_gpu_map_carve.py the device."""
import numpy as np

VS = 0.5
W = 8


def _up(x):
    return float(np.nextafter(x, np.inf))


def _case(name, cfg, origin, ends, stored, expect, **counts):
    px = np.zeros((1, W, 3), dtype=np.float32)
    px[0, :len(ends)] = np.asarray(ends, dtype=np.float32)
    return dict(name=name, cfg=cfg, origin=np.asarray(origin, dtype=np.float64), xyz=px, stored=np.asarray(stored, dtype=np.float64),
                expect=np.asarray(expect, dtype=np.int64).reshape(-1, 2), counts=counts)


def hand_cases():
    out = []
    # 1. one ray along +x, (0, 0, 0) -> (4, 0, 0): len 4, len - margin 3.75, len + margin 4.25 (in the end's voxel 8 = [4, 4.5))
    cfg = dict(radius=0.25, margin=0.25, step=0.25, min_range=1.0, max_range=8.0)
    out.append(_case("+x", cfg, [0, 0, 0], [[4, 0, 0]],
                     [[2.0, 0.25, 0.0],          # at perpendicular distance exactly radius: through
                      [2.0, _up(0.25), 0.0],     # one ulp beyond: nothing
                      [3.75, 0.0, 0.125],        # t_p = len - margin exactly: through
                      [_up(3.75), 0.0, 0.125],   # just past it: support
                      [4.25, 0.125, 0.0],        # t_p = len + margin exactly: support
                      [_up(4.25), 0.125, 0.0],   # past it: nothing
                      [0.75, 0.0, 0.0],          # t_p < min_range: nothing
                      [2.0, 0.125, -0.5]],       # voxel (4, 0, -1) is not visited (and the point is beyond the radius anyway)
                     [[1, 0], [0, 0], [1, 0], [0, 1], [0, 1], [0, 0], [0, 0], [0, 0]],
                     n_rays=1, n_no_return=W - 1, n_rays_out_of_range=0, n_voxel_visits=4, n_scans=1))  # voxels 1, 4, 7, 8 on x
    # 2. a diagonal, (0, 0, 0) -> (3, 4, 0): len 5, radius 5 / 16, so a perpendicular offset of exactly the radius is (-1/4, 3/16, 0)
    cfg = dict(radius=0.3125, margin=0.5, step=0.25, min_range=0.0, max_range=8.0)
    out.append(_case("diagonal", cfg, [0, 0, 0], [[3, 4, 0]],
                     [[1.0625, 1.9375, 0.0],       # foot (1.3125, 1.75), exactly at the radius, in voxel (2, 3, 0) that the ray crosses: through
                      [1.0625, _up(1.9375), 0.0],  # one ulp beyond: nothing
                      [1.25, 2.1875, 0.0],         # foot (1.5, 2), exactly at the radius, but the ray misses voxel (2, 4, 0): NOT counted
                      [1.3125, 1.75, 0.3125],      # exactly at the radius along z, t_p = 2.1875: through
                      [3.0, 4.0, 0.0]],            # the end itself: support
                     [[1, 0], [0, 0], [0, 0], [1, 0], [0, 1]],
                     n_rays=1, n_no_return=W - 1))
    # 3. too long, no return, and shorter than step / 2 (one sample: w itself)
    cfg = dict(radius=0.25, margin=0.5, step=0.25, min_range=0.0, max_range=8.0)
    out.append(_case("out of range / short", cfg, [0, 0, 0], [[8.125, 0, 0], [0, 0, 0], [0.0625, 0, 0], [0, 8.0, 0]],
                     [[0.0625, 0.125, 0.0],   # the short ray's only voxel: t_p = 1/16 <= len + margin: support; the ray along y (len 8 = max_range:
                                              # used) starts in this voxel too: t_p = 1/8 <= 7.5: through
                      [4.0, 0.0, 0.0],        # only the ray that is too long comes here
                      [0.0, 7.75, 0.125]],    # the y ray: 7.5 < t_p <= 8.5: support
                     [[1, 1], [0, 0], [0, 1]],
                     n_rays=2, n_rays_out_of_range=1, n_no_return=W - 3))
    # 4. more than 64 samples (len 20: 81) and more than 1000 (len 300: 1201): rounds of the half-wave; points around the round edges
    cfg = dict(radius=0.25, margin=0.5, step=0.25, min_range=0.0, max_range=512.0)
    xs = [0.125, 7.625, 7.875, 8.125, 15.875, 16.125, 19.25, 19.75]
    ys = [0.125, 7.875, 8.125, 16.125, 100.0, 255.875, 256.125, 299.25, 300.25]
    out.append(_case("long", cfg, [0, 0, 0], [[20, 0, 0], [0, 300, 0]],
                     [[x, 0.0, 0.125] for x in xs] + [[0.125, y, 0.0] for y in ys],
                     # x ray: through up to 19.5, support up to 20.5; the y ray meets (0.125, 0, 0.125) too: t_p 0 -> through
                     [[2, 0]] + [[1, 0]] * 6 + [[0, 1]] + [[2, 0]] + [[1, 0]] * 6 + [[1, 0], [0, 1]],
                     n_rays=2, n_no_return=W - 2))
    out[-1]["expect"][8] = [2, 0]
    # 5. through voxel 0, which spans (-0.5, 0.5): both points are in it and it is visited once
    cfg = dict(radius=0.25, margin=0.5, step=0.25, min_range=0.0, max_range=8.0)
    out.append(_case("voxel 0", cfg, [-2.0, 0.125, 0.125], [[4, 0, 0]],
                     [[-0.25, 0.125, 0.125], [0.25, 0.125, 0.125], [-0.75, 0.125, 0.125]],
                     [[1, 0], [1, 0], [1, 0]], n_rays=1, n_voxel_visits=2))
    # 6. an end outside the key range (2^20 voxels of 0.5 m: 524288 m): the samples out there are passed over
    cfg = dict(radius=0.25, margin=0.5, step=0.25, min_range=0.0, max_range=32.0)
    out.append(_case("key range", cfg, [524280.0, 0.0, 0.0], [[20, 0, 0]],
                     [[524285.25, 0.0, 0.125], [524287.75, 0.125, 0.0]],
                     [[1, 0], [1, 0]], n_rays=1, n_voxel_visits=2))
    return out


def case_rays(case, col_poses=None):
    """(o, w, ret) of the case's sweep for the restatement; col_poses (W, 4, 4) as the device evaluated them, else the nominal pose"""
    from tests.helpers import map_carve_numpy as cv
    if col_poses is None:
        col_poses = np.tile(np.eye(4), (W, 1, 1))
        col_poses[:, :3, 3] = case["origin"]
    return cv.rays_of_sweep(case["xyz"].astype(np.float64), np.any(case["xyz"] != 0.0, axis=2), col_poses)
