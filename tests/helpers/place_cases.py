"""Scenes of the place descriptors, shared by the CPU tests of the numpy restatement and the GPU tests of the kernels."""
from functools import lru_cache

import numpy as np

CONFIGS = ((20, 60), (1, 4), (3, 8), (64, 64))  # (n_ring, n_sector): the default; the smallest; pad bytes; the largest
PARAMS = dict(min_radius=1.0, max_radius=80.0, z_min=-2.0, z_step=0.0625)
Z_LEVELS = (0, 1, 253, 254, 255)


def _near(v):
    return (np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf))


def ring_edge_points(edge2, z):
    """per ring edge x = sqrt(edge2[i]) and its two neighbours, on the +x axis: (3 (R + 1), 3)"""
    return np.array([[x, 0.0, z] for e in edge2 for x in _near(np.sqrt(e))])


def sector_edge_points(edge2, sdir, z):
    """per sector direction t dir_j (t in the middle of the first ring, or of the only one) and its neighbours one ulp away in x and in y;
    then the axis points, where a cross product is exactly 0: (5 S + 4, 3)"""
    t = 0.5 * (np.sqrt(edge2[0]) + np.sqrt(edge2[1]))
    rows = []
    for ex, ey in sdir:
        x, y = t * ex, t * ey
        rows.append([x, y, z])
        rows += [[xx, y, z] for xx in (_near(x)[0], _near(x)[2])] + [[x, yy, z] for yy in (_near(y)[0], _near(y)[2])]
    rows += [[t, 0.0, z], [-t, 0.0, z], [0.0, t, z], [0.0, -t, z]]
    return np.array(rows)


def special_points(edge2, z_min, z_step):
    """no return, non-finite rows, the level edges z_min + k z_step, one ulp below z_min, z = 1e300 - each level point in the first ring at
    its own heading (with 4 sectors several share a cell: the maximum decides)"""
    t = 0.5 * (np.sqrt(edge2[0]) + np.sqrt(edge2[1]))
    zs = [z_min + k * z_step for k in Z_LEVELS] + [np.nextafter(z_min, -np.inf), 1e300]
    rows = [[0.0, 0.0, 0.0], [np.nan, 1.0, 0.0], [2.0, np.inf, 0.0], [2.0, 1.0, -np.inf], [-0.0, 0.0, 0.0]]
    for a, z in enumerate(zs):
        ang = 0.1 + 0.8 * a
        rows.append([t * np.cos(ang), t * np.sin(ang), z])
    return np.array(rows)


def edge_points(edge2, sdir, z_min, z_step):
    """every binning edge of a configuration in one fp64 point set"""
    z = z_min + 10.5 * z_step
    return np.concatenate([ring_edge_points(edge2, z), sector_edge_points(edge2, sdir, z), special_points(edge2, z_min, z_step)])


def random_points(seed, n, max_radius, z_min, z_step):
    """a cloud around the sensor reaching past the outer ring and below z_min, with a few no-returns"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-1.1, 1.1, n) * max_radius, rng.uniform(-1.1, 1.1, n) * max_radius,
                  z_min + rng.uniform(-8.0, 300.0, n) * z_step], axis=1)
    p[rng.random(n) < 0.05] = 0.0
    return p


def quarter_turn_z():
    """an exact 90 degree turn about z as rot9"""
    return np.array([0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def random_descriptors(seed, n, n_ring, n_sector, fill=0.15):
    """(n, S, Rpad) uint8: random sparse descriptors with zero pad bytes"""
    rng = np.random.default_rng(seed)
    rp = (n_ring + 3) // 4 * 4
    d = np.zeros((n, n_sector, rp), dtype=np.uint8)
    d[:, :, :n_ring] = rng.integers(1, 256, (n, n_sector, n_ring)) * (rng.random((n, n_sector, n_ring)) < fill)
    return d


def distinct_descriptor(n_ring, n_sector):
    """(S, Rpad) uint8 whose columns all differ, so that no two shifts of it are equal"""
    d = np.zeros((n_sector, (n_ring + 3) // 4 * 4), dtype=np.uint8)
    j, r = np.meshgrid(np.arange(n_sector), np.arange(n_ring), indexing="ij")
    d[:, :n_ring] = 1 + (7 * j + 3 * r) % 250
    return d


MATCH_COUNTS =(0, 1, 2, 63, 64, 65, 130)
FUNCTIONAL = dict(seed=1000, n_scans=200, H=16, W=256, every=4, sweep=40, turns_deg=(97.0, 201.0, 354.0))


def rot_z(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


@lru_cache(maxsize=None)
def functional_sweeps():
    """(kept sweeps as float64 (n, H W, 3), the index of FUNCTIONAL's sweep among them)"""
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import synth
    f = FUNCTIONAL
    seq = synth.make_sequence(seed=f["seed"], n_scans=f["n_scans"], H=f["H"], W=f["W"])
    kept = list(range(0, f["n_scans"], f["every"]))
    return np.array([seq.scan(k).astype(np.float64) for k in kept]), kept.index(f["sweep"])


def turned(sweep, deg):
    """the sweep's returns turned by +deg about z (a no-return stays (0, 0, 0))"""
    return np.asarray(sweep, dtype=np.float64) @ rot_z(deg).T
