"""Map-distance cases with answers computed by hand, shared by the CPU test of the numpy restatement and the GPU test of the
kernels.  Voxel size 0.5, every coordinate dyadic, so every difference and square below is exact."""
import numpy as np

VS = 0.5
INF, NAN = np.inf, np.nan


def hand_cases():
    """(reference points (M, 3), max_dist, [(name, query, expected per-point value)])"""
    up = np.nextafter(1.25, np.inf)
    ref = np.array([
        [0.25, 0.125, 0.125],        # voxel (0, 0, 0)
        [0.5625, 0.125, 0.125],      # voxel (1, 0, 0): across a face from x = 0.4375
        [0.5625, 0.5625, 0.5625],    # voxel (1, 1, 1): across a corner from (0.4375, 0.4375, 0.4375)
        [1.25, 1.125, 1.125],        # voxel (2, 2, 2): exactly max_dist from (1.0, 1.125, 1.125)
        [up, 3.125, 3.125],          # voxel (2, 6, 6): one ulp beyond max_dist from (1.0, 3.125, 3.125)
    ])
    max_dist = 0.25
    cases = [
        # index 0 spans (-vs, vs): the query at x = -0.25 shares voxel 0 with the point at x = 0.25; but 0.5 apart is beyond max_dist = 0.25 ...
        ("voxel 0 at a negative coordinate, too far", [-0.25, 0.125, 0.125], INF),
        # ... while from x = -2^-60 dx = 0.25 + 2^-60 rounds to 0.25 (half an ulp of 0.25 is 2^-55): d2 = 0.0625 exactly, matched from below zero
        ("voxel 0 at a negative coordinate", [-(2.0 ** -60), 0.125, 0.125], 0.0625),
        ("across a face", [0.4375, 0.125, 0.125], 0.125 * 0.125),
        ("across a corner", [0.4375, 0.4375, 0.4375], 3 * 0.125 * 0.125),
        ("exactly max_dist", [1.0, 1.125, 1.125], 0.0625),
        ("one ulp beyond max_dist", [1.0, 3.125, 3.125], INF),
        ("empty neighbourhood", [10.0, 10.0, 10.0], INF),
        ("non-finite query", [NAN, 0.0, 0.0], NAN),
        ("infinite query", [0.0, INF, 0.0], NAN),
        ("beyond the key range", [0.5 * 2.0 ** 21, 0.0, 0.0], INF),
    ]
    return ref, max_dist, cases
