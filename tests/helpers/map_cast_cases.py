"""Cast cases whose answers are computed by hand: one sweep of 1 x 8 pixels from a sensor with identity rotation at
`origin`; a pixel is its end in the sensor frame, (0, 0, 0) = no return.  Voxel size 0.5 and dyadic numbers, so every product, sum and
comparison of the definition is exact.  `expect`: per pixel (status, row of `stored` that is hit or -1, t_hit or None where the case does
not pin it, class of `changes(CHANGE_MARGIN)`); the pixels behind the listed ends have no return.  `counts`: the summary entries the case
pins.  tests/test_map_cast_cpu.py holds the restatement to these answers, tests/test_gpu_map_cast.py the device."""
import numpy as np

VS = 0.5
W = 8
CHANGE_MARGIN = 0.5
NONE, HIT, MISS, DEGEN = 0, 1, 2, 3
C_NONE, C_AGREE, C_NEW, C_GONE, C_UNMAPPED = 0, 1, 2, 3, 4
NO_RETURN = (NONE, -1, -1.0, C_NONE)


def _up(x):
    return float(np.nextafter(x, np.inf))


def _down(x):
    return float(np.nextafter(x, -np.inf))


def _case(name, cfg, origin, ends, stored, expect, **counts):
    px = np.zeros((1, W, 3), dtype=np.float32)
    px[0, :len(ends)] = np.asarray(ends, dtype=np.float32)
    expect = list(expect) + [NO_RETURN] * (W - len(expect))
    return dict(name=name, cfg=cfg, origin=np.asarray(origin, dtype=np.float64), xyz=px,
                stored=np.asarray(stored, dtype=np.float64).reshape(-1, 3), expect=expect, counts=counts)


def case_rays(case, col_poses=None):
    """(o, w, ret) of a case as the restatement takes them"""
    from tests.helpers.map_cast_numpy import rays_of_sweep
    pose = np.eye(4)
    pose[:3, 3] = case["origin"]
    M = np.tile(pose, (W, 1, 1)) if col_poses is None else col_poses
    x = case["xyz"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return rays_of_sweep(x, np.any(case["xyz"] != 0.0, axis=2), M)


def round_case(K):
    """a ray of exactly K samples (step 0.25, max_range = K / 4) whose only stored point sits at the LAST sample, in a voxel that no earlier
    sample touches: the hit is found by lane (K - 1) % 32 of round (K - 1) // 32"""
    ox = 0.25 if K % 2 == 0 else 0.5
    t = (K - 0.5) * 0.25
    cfg = dict(radius=0.125, step=0.25, min_range=0.0, max_range=K * 0.25)
    return _case(f"{K} samples", cfg, [ox, 0.25, 0.25], [[1, 0, 0]], [[ox + t, 0.25, 0.25]], [(HIT, 0, t, C_NEW)],
                 n_hit=1, n_voxel_visits=1, n_no_return=W - 1)


def hand_cases():
    out = []
    O = [0.25, 0.25, 0.25]
    # 1. rays along +x from (0.25, 0.25, 0.25), one stored point on the line at t = 2: hits before, at and beyond the measured length, and
    # the measured length never stops the march (the ray of length 1 still finds the point at 2)
    cfg = dict(radius=0.125, step=0.25, min_range=0.0, max_range=8.0)
    out.append(_case("+x: len against t_hit", cfg, O, [[4, 0, 0], [1, 0, 0], [2, 0, 0], [2.5, 0, 0], [1.5, 0, 0], [1.25, 0, 0], [-3, 0, 0]],
                     [[2.25, 0.25, 0.25]],
                     [(HIT, 0, 2.0, C_GONE), (HIT, 0, 2.0, C_NEW), (HIT, 0, 2.0, C_AGREE), (HIT, 0, 2.0, C_AGREE),   # len 2.5 = t + margin: agree
                      (HIT, 0, 2.0, C_AGREE), (HIT, 0, 2.0, C_NEW), (MISS, -1, -1.0, C_UNMAPPED)],                     # len 1.5 = t - margin: agree
                     n_hit=6, n_miss=1, n_no_return=1, n_degenerate=0, n_voxel_visits=6))
    # 2. the radius: a point at perpendicular distance exactly radius is near, one ulp inside is near, one ulp beyond is not; the voxel is
    # then left for good and the next voxel's point is the hit
    out.append(_case("radius: exactly, one ulp inside and one ulp beyond", cfg, O, [[4, 0, 0], [0, 4, 0], [0, 0, 4]],
                     [[2.25, 0.375, 0.25],         # +x ray: |e x d|^2 = (0.125 4)^2 = 0.25 = r^2 len2: hit at t = 2
                      [0.25, 2.25, _up(0.375)],    # +y ray: one ulp beyond the radius along z: passed over ...
                      [0.125, 3.25, 0.25],         # ... and this one, exactly at the radius along -x in a later voxel, is the hit at t = 3
                      # +z ray: one ulp inside the radius along y: ey = 2^-3 - 2^-54 exactly, 4 ey exact, its square rounds to 0.25 - 2^-52 <
                      # r^2 len2: the hit at t = 2 ...
                      [0.25, _down(0.375), 2.25],
                      [0.25, 0.25, 3.25]],         # ... and not this one on the line in a later voxel, t = 3, which a march that passed it over would give
                     [(HIT, 0, 2.0, C_GONE), (HIT, 2, 3.0, C_GONE), (HIT, 3, 2.0, C_GONE)], n_hit=3, n_voxel_visits=4))
    # 3. t_p exactly at min_range and max_range qualifies, one ulp outside does not
    cfg3 = dict(radius=0.125, step=0.25, min_range=1.0, max_range=3.0)
    out.append(_case("t_p at min_range and max_range", cfg3, O, [[4, 0, 0], [0, 4, 0], [0, 0, 4], [0, -4, 0]],
                     [[_down(1.25), 0.25, 0.25],   # +x: t_p one ulp below min_range: no; its voxel [1, 1.5) is left for good ...
                      [1.375, 0.25, 0.25],         # ... (this one, in the same voxel, t_p = 1.125, is taken: the voxel does hold a qualifying point)
                      [0.25, 1.25, 0.25],          # +y: t_p = min_range exactly: hit
                      [0.25, 0.25, 3.25],          # +z: t_p = max_range exactly (voxel [3, 3.5) is met by the last sample, t = 2.875): hit
                      [0.25, _down(-2.75), 0.25]], # -y: t_p one ulp above max_range: miss
                     [(HIT, 1, 1.125, C_GONE), (HIT, 2, 1.0, C_GONE), (HIT, 3, 3.0, C_GONE), (MISS, -1, -1.0, C_UNMAPPED)],
                     n_hit=3, n_miss=1, n_voxel_visits=4))
    # 4. ties: equal t_p in the deciding voxel go to the smaller (x, y, z); equal coordinates to the smaller index
    out.append(_case("ties", cfg, O, [[4, 0, 0], [0, 4, 0]],
                     [[2.25, 0.3125, 0.25], [2.25, 0.1875, 0.3125], [2.25, 0.1875, 0.25],   # +x: all t_p = 2; (2.25, 0.1875, 0.25) is the smallest
                      [0.25, 2.25, 0.25], [0.25, 2.25, 0.25]],                                # +y: twice the same point: the first row
                     [(HIT, 2, 2.0, C_GONE), (HIT, 3, 2.0, C_GONE)], n_hit=2, n_voxel_visits=2))
    # 5. the first voxel with a qualifying point decides, although a LATER voxel holds one with a smaller t_p; and an earlier voxel whose
    # points are all off the line is passed over.  Ray (8, 1, 0) s from (0.25, 0.25, 0.25): it crosses y = 0.5 at x = 2.25, so voxel
    # A = (4, 0, 0) (the sample at t = 1.875) comes before voxel B = (4, 1, 0).  Both points are 0.085 from the line.
    out.append(_case("the earlier voxel decides", cfg, O, [[8, 1, 0], [0, 0, 4]],
                     [[2.4375, 0.4375, 0.25],    # in A, t_p = 17.6875 / sqrt(65) = 2.19...: the hit
                      [2.0625, 0.5625, 0.25],    # in B, t_p = 14.8125 / sqrt(65) = 1.83...: smaller, later, not the answer
                      [0.25, 0.0, 1.25],         # +z ray: voxel (0, 0, 2) holds only a point 0.25 off the line: passed over
                      [0.25, 0.25, 2.25]],       # the next occupied voxel on the line: the hit
                     [(HIT, 0, None, C_GONE), (HIT, 3, 2.0, C_GONE)], n_hit=2))
    # 6. voxel 0 spans (-0.5, 0.5) per axis (the index truncates): a ray through it from either side meets BOTH points in one visit and
    # takes the one with the smaller t_p
    out.append(_case("voxel 0", cfg, [-1.25, 0.25, 0.25], [[4, 0, 0]], [[0.375, 0.25, 0.25], [-0.375, 0.25, 0.25]],
                     [(HIT, 1, 0.875, C_GONE)], n_hit=1, n_voxel_visits=1))
    out.append(_case("voxel 0 from the other side", cfg, [1.25, 0.25, 0.25], [[-4, 0, 0]], [[-0.375, 0.25, 0.25], [0.375, 0.25, 0.25]],
                     [(HIT, 1, 0.875, C_GONE)], n_hit=1, n_voxel_visits=1))
    # 7. no return, degenerate returns (a non-finite end; an end that the pose's translation swallows: len2 == 0), and they do not disturb
    # the pixel beside them
    out.append(_case("no return and degenerate", cfg, O, [[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1], [1e-30, 0, 0], [4, 0, 0]],
                     [[2.25, 0.25, 0.25]],
                     [NO_RETURN, (DEGEN, -1, -1.0, C_NONE), (DEGEN, -1, -1.0, C_NONE), (DEGEN, -1, -1.0, C_NONE), (DEGEN, -1, -1.0, C_NONE),
                      (HIT, 0, 2.0, C_GONE)],
                     n_no_return=3, n_degenerate=4, n_hit=1, n_miss=0, n_voxel_visits=1))
    # 8. a ray that leaves the key range (2^20 voxels = 524288 m either side): the samples beyond are passed over, the ray is a miss; the ray
    # back into the range meets the point
    far = 524287.25
    out.append(_case("leaving the key range", cfg, [far, 0.25, 0.25], [[4, 0, 0], [-4, 0, 0]], [[far - 2.0, 0.25, 0.25], [far + 0.5, 0.25, 0.375]],
                     [(HIT, 1, 0.5, C_GONE), (HIT, 0, 2.0, C_GONE)], n_hit=2))
    out.append(_case("leaving the key range: a miss", cfg, [far, 0.25, 0.25], [[4, 0, 0]], [[far - 2.0, 0.25, 0.25]],
                     [(MISS, -1, -1.0, C_UNMAPPED)], n_miss=1, n_voxel_visits=0))
    # 9. the empty map
    out.append(_case("empty map", cfg, O, [[4, 0, 0], [0, 0, 0], [np.nan, 1, 1]], np.zeros((0, 3)),
                     [(MISS, -1, -1.0, C_UNMAPPED), NO_RETURN, (DEGEN, -1, -1.0, C_NONE)], n_hit=0, n_miss=1, n_degenerate=1, n_voxel_visits=0))
    # 10. rays of exactly 31, 32, 33, 64 and 65 samples: the edges of the rounds of 32
    out += [round_case(K) for K in (31, 32, 33, 64, 65)]
    return out
