"""Scenes of the pose search, shared by the CPU test of the numpy restatement and the GPU tests of the kernels.  Voxel size
0.5; the lattice scenes have dyadic coordinates throughout, so a pose that is a multiple of 90 degrees with a dyadic translation transforms
them exactly."""
from functools import lru_cache

import numpy as np

from tests.helpers.map_compare_cases import hand_cases as _cmp_hand_cases

VS = 0.5
THRESHOLDS = (0.125, 0.25, 0.25, 0.5)  # (equal neighbours are allowed)


def pose(rotvec=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(np.asarray(rotvec, dtype=np.float64)).as_matrix()
    T[:3, 3] = t
    return T


def quarter_turn(perm, signs, t):
    """an exact pose: world axis r takes signs[r] * (sensor axis perm[r]), plus the dyadic translation t"""
    T = np.zeros((4, 4))
    for r in range(3):
        T[r, perm[r]] = signs[r]
    T[:3, 3] = t
    T[3, 3] = 1.0
    assert round(np.linalg.det(T[:3, :3])) == 1
    return T


def exact_poses():
    """multiples of 90 degrees with dyadic translations; the first is the identity"""
    return np.array([
        np.eye(4),
        quarter_turn((1, 0, 2), (-1.0, 1.0, 1.0), (0.25, -0.5, 0.125)),     # 90 degrees about z
        quarter_turn((0, 1, 2), (-1.0, -1.0, 1.0), (-0.375, 0.0625, 0.5)),  # 180 degrees about z
        quarter_turn((1, 0, 2), (1.0, -1.0, 1.0), (1.0, 0.75, -0.25)),      # 270 degrees about z
        quarter_turn((0, 2, 1), (1.0, -1.0, 1.0), (0.0, 0.5, 0.015625)),    # 90 degrees about x
        quarter_turn((2, 1, 0), (1.0, 1.0, -1.0), (-0.125, -0.125, 0.25)),  # 90 degrees about y
        quarter_turn((0, 1, 2), (1.0, 1.0, 1.0), (0.0078125, 0.0, 0.0)),    # a pure translation by 2^-7
    ])


def general_poses():
    """general rotations, attitudes past 120 degrees (2.094 rad) among them, with non-dyadic translations"""
    return np.array([
        pose((0.0, 0.0, 0.3), (0.1, -0.2, 0.05)),
        pose((0.2, -0.1, 1.0), (-0.3, 0.15, 0.0)),
        pose((1.3, 1.3, -1.2), (0.02, 0.03, -0.04)),     # |rotvec| = 2.19 rad = 126 degrees
        pose((0.0, 0.0, 2.9), (0.4, 0.1, 0.2)),          # 166 degrees about z
        pose((2.0, -2.2, 0.9), (-0.05, 0.0, 0.3)),       # 3.1 rad = 178 degrees
        pose((-1.9, 0.3, 1.7), (0.3, 0.3, -0.3)),        # 2.57 rad = 147 degrees
    ])


def hand_scene():
    """(stored points, max_dist, thresholds, query points, poses, expected hits (K, T)): the hand cases of the map distance (every answer
    computed by hand there) seen through the identity, through an exact pose with the query set moved into its sensor frame (the same world
    points, so the same counts), and through a pose with a NaN (no probe: -1)"""
    ref, max_dist, cases = _cmp_hand_cases()
    w = np.array([c[1] for c in cases])
    thr = (0.125, 0.25)
    # by hand (map_compare_cases): d2 = 0.0625, 0.015625, 0.046875, 0.0625 for the four matched cases: one within 0.125^2, four within 0.25^2
    want_world = (1, 4)
    T = exact_poses()[1]  # wx = -qy + 0.25, wy = qx - 0.5, wz = qz + 0.125
    with np.errstate(invalid="ignore"):
        q1 = np.stack([w[:, 1] + 0.5, -(w[:, 0] - 0.25), w[:, 2] - 0.125], axis=1)
    bad = np.eye(4)
    bad[1, 2] = np.nan
    return ref, max_dist, thr, (w, q1), (np.eye(4), T, bad), want_world


@lru_cache(maxsize=None)
def lattice_map():
    """(M, 3) dyadic points (multiples of 1/64): a dense core, where a voxel of 20 fills, a sparse shell with single points, and the isolated
    points of `lattice_queries`' boundary pairs"""
    rng = np.random.default_rng(23)
    core = rng.integers(-80, 81, (6000, 3)) / 64.0     # [-1.25, 1.25]^3: about 17 points a voxel on average
    shell = rng.integers(128, 257, (40, 3)) / 64.0 * rng.choice([-1.0, 1.0], (40, 3))  # 2 .. 4 m out, scattered
    out = np.concatenate([core, shell, BOUNDARY_POINTS])
    out.setflags(write=False)
    return out


# isolated stored points, 4 m apart along y at z = 8: on a voxel face, inside a voxel, and in voxel 0's double-width span (x in (-0.5, 0.5))
BOUNDARY_POINTS = np.array([[8.0, -8.0, 8.0], [7.75, -4.0, 8.0], [-0.125, 0.0, 8.0], [-0.375, 4.0, 8.0], [0.375, 8.0, 8.0]])
BOUNDARY_THR = 0.25


@lru_cache(maxsize=None)
def lattice_queries():
    """(n, 3) dyadic sensor-frame points: per boundary point three queries along x - at exactly BOUNDARY_THR, and the nearest coordinate either
    side at which the rounded difference p - q changes at all (one ulp of the coordinate, which is one ulp of the threshold or more; next to
    zero, where the coordinate is finer than the difference, the first of the few coordinate ulps that moves it) - under the identity
    d2 == thr^2, just below, just above; then random points over the core and the shell"""
    rows = []
    for p in BOUNDARY_POINTS:
        x = p[0] + BOUNDARY_THR
        rows.append([x, p[1], p[2]])
        for toward in (-np.inf, np.inf):
            xx = np.nextafter(x, toward)
            while p[0] - xx == p[0] - x:
                xx = np.nextafter(xx, toward)
            rows.append([xx, p[1], p[2]])
    rng = np.random.default_rng(29)
    out = np.concatenate([np.array(rows), rng.integers(-112, 113, (190, 3)) / 64.0, rng.integers(-256, 257, (52, 3)) / 64.0])
    out.setflags(write=False)
    return out  # 15 + 190 + 52 = 257 points


def first_per_voxel(points, voxel, cap=1):
    """the first `cap` rows of `points` (N, 3) in each voxel of side `voxel` (the map's truncating index), in array order"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    key = np.trunc(p / np.float64(voxel)).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    rank = np.empty(len(p), dtype=np.int64)
    starts = np.flatnonzero(np.r_[True, inv[order][1:] != inv[order][:-1]])
    rank[order] = np.arange(len(p)) - np.repeat(starts, np.diff(np.r_[starts, len(p)]))
    return p[rank < cap]


def returns(sweep):
    """the rows of a sweep (H W, 3) that carry a return, as float64"""
    x = np.asarray(sweep, dtype=np.float64).reshape(-1, 3)
    return x[(x != 0.0).any(axis=1)]


E2E = dict(seed=1000, other_seed=1001, n_scans=12, H=32, W=256, map_sweeps=range(10), keyframes=(0, 3, 6, 9), n_yaw=16, query_sweep=11,
           query_voxel=1.0, true_candidate=3 * 16 + 0)


@lru_cache(maxsize=None)
def end_to_end_scene():
    """dict(seq, gt (12, 4, 4), map_points, keyframes (4, 4, 4), query (n, 3), other_query): sweeps 0 - 9 of a synthetic sequence on their
    ground-truth (mid-sweep) poses, thinned to the first 20 points per 0.5 m voxel in sweep order - the stored set, so that a device map
    that is handed these points holds all of them; the keyframes are the ground-truth poses of sweeps 0, 3, 6, 9; the query is sweep 11
    thinned to the first point per 1 m voxel, and the same of sweep 11 of another scene"""
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import synth
    from tests.helpers import pose_search_numpy as psn
    e = E2E
    seq = synth.make_sequence(seed=e["seed"], n_scans=e["n_scans"], H=e["H"], W=e["W"])
    other = synth.make_sequence(seed=e["other_seed"], n_scans=e["n_scans"], H=e["H"], W=e["W"])
    gt = seq.gt_poses(0.5)
    world = np.concatenate([psn.transform(returns(seq.scan(k)), gt[k]) for k in e["map_sweeps"]])
    return dict(seq=seq, gt=gt, map_points=first_per_voxel(world, VS, cap=20), keyframes=gt[list(e["keyframes"])],
                query=first_per_voxel(returns(seq.scan(e["query_sweep"])), e["query_voxel"]),
                other_query=first_per_voxel(returns(other.scan(e["query_sweep"])), e["query_voxel"]),
                sweeps={k: seq.scan(k) for k in (10, 11)}, other_sweep=other.scan(e["query_sweep"]))
