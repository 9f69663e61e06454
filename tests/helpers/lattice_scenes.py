"""Scenes on which the hard cases of the voxel search are the rule, not the exception (pure numpy; no GPU, no oracle).

Every coordinate is a dyadic rational.  With an identity rotation and a dyadic translation every position, difference and squared
distance of the first Gauss-Newton iteration is then exact in fp64 on every implementation that does not contract a * b + c: a tie
is a tie everywhere, a distance that equals the gate equals it everywhere, a coordinate on a voxel boundary is on it everywhere.
tests/test_lattice_scenes_cpu.py proves the scenes are what they claim; tests/test_gpu_search_edges.py runs the kernels on them.
"""
import numpy as np

VOXEL_SIZES = (0.7, 0.35, 1.05, 0.1, 0.3, 0.15, 0.45, 1.0, 0.5, 0.25)
DISPLACEMENTS = ((0.25, 0.25, 0.0), (0.25, 0.0, 0.0), (0.125, 0.25, 0.0), (0.25, 0.25, 0.25))
# the configuration the triplets were designed for
VOXEL_SIZE, MAX_RANGE, MIN_RANGE = 1.0, 100.0, 0.5
SWEEP_H, SWEEP_W = 16, 1024


def _grid(axis):
    g = np.meshgrid(axis, axis, axis, indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1)


def lattice_block(lo=-6.0, hi=6.0, seed=0):
    """points at arange(lo, hi, 0.5) + 0.25 on each axis in a seeded shuffled order (insertion order matters).  A 1.0 voxel holds
    8 of them; truncation toward zero makes the voxels around 0 double width, so they hold up to 64 and a 20-point cap binds there"""
    pts = _grid(np.arange(lo, hi, 0.5) + 0.25)
    return pts[np.random.default_rng(seed).permutation(len(pts))]


def tie_queries(seed=0):
    """(map points, queries): the block restricted to [-2, 2)^3 and the grid arange(-2, 2.01, 0.25)^3 - cell centres (8-way ties), face and
    edge midpoints (2- and 4-way), the stored points themselves (distance 0), coordinates on voxel boundaries and at +0; behind the grid, its
    queries with a zero coordinate once more with -0.0 in its place"""
    q = _grid(np.arange(-2.0, 2.01, 0.25))
    z = q[(q == 0.0).any(axis=1)].copy()
    z[z == 0.0] = -0.0
    return lattice_block(-2.0, 2.0, seed), np.concatenate([q, z])


def pick_queries(map_pts, queries, gate, per_kind=16, limit=240):
    """indices of a fixed subset of the tie queries with every kind in it: by the number of map points at the smallest distance (1, 2, 4, 8),
    a coordinate on a voxel boundary, a coordinate of +0 or -0, distance 0, distance exactly the gate - the first per_kind of each kind"""
    d2 = ((queries[:, None, :] - map_pts[None, :, :]) ** 2).sum(axis=2)
    best = d2.min(axis=1)
    kind = np.stack([(d2 == best[:, None]).sum(axis=1), (queries == np.round(queries)).any(axis=1), ((queries == 0) & ~np.signbit(queries)).any(axis=1),
                     ((queries == 0) & np.signbit(queries)).any(axis=1), best == 0.0, np.sqrt(best) == gate], axis=1).astype(np.int64)
    seen, out = {}, []
    for i, k in enumerate(map(tuple, kind)):
        if seen.setdefault(k, 0) < per_kind:
            seen[k] += 1
            out.append(i)
    return np.array(out[:limit])


def _ulps(x, n):
    """x moved |n| units in the last place of its own precision, up for n > 0 and down for n < 0"""
    x = np.asarray(x)
    to = np.asarray(np.inf if n > 0 else -np.inf, dtype=x.dtype)
    for _ in range(abs(n)):
        x = np.nextafter(x, to)
    return x


def gate_queries(M):
    """(map points, queries, exact): isolated map points (nothing else in their 27 voxels of size 1.0; 8 m apart) and, for each, queries
    whose offset from it is M long in exact arithmetic, and 1, 2 and 3 ulp either side: along both directions of every axis from points whose
    coordinate on that axis is 0 (the query's coordinate IS the distance), 0.25 and -37.25 (the difference is rounded), and from a point at
    the origin along (3, 4, 0) / 5, (1, 2, 2) / 3 and (2, 3, 6) / 7 in three rotations and both signs, the largest coordinate nudged.
    exact[i]: query i is the un-nudged one"""
    pts, qs, exact = [np.zeros(3)], [], []
    for axis in range(3):
        for j, (base, sign) in enumerate((b, s) for b in (0.0, 0.25, -37.25) for s in (1.0, -1.0)):
            p = np.empty(3)
            p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = base, 8.0 * (j + 1) + 0.25, 0.25
            pts.append(p)
            for u in (-3, -2, -1, 0, 1, 2, 3):
                q = p.copy()
                q[axis] = base + sign * float(_ulps(np.float64(M), u))
                qs.append(q)
                exact.append(u == 0)
    for tri, den in (((3.0, 4.0, 0.0), 5.0), ((1.0, 2.0, 2.0), 3.0), ((2.0, 3.0, 6.0), 7.0)):
        for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            for sign in (1.0, -1.0):
                off = sign * np.array(tri)[list(perm)] * M / den
                j = int(np.argmax(np.abs(off)))
                for u in (-3, -2, -1, 0, 1, 2, 3):
                    q = off.copy()
                    q[j] = float(_ulps(np.float64(off[j]), u))
                    qs.append(q)
                    exact.append(u == 0)
    return np.array(pts), np.array(qs), np.array(exact)


def boundary_coordinates(vs):
    """(probes, companions): k * vs for k in -300..300 and a few large |k| up to 1e6, each at the value itself and 1 and 2 ulp either side;
    and for every k the coordinates (k - 0.5) vs and (k + 0.5) vs, well inside the voxel on each side"""
    k = np.concatenate([np.arange(-300, 301), [-1000000, -65536, -4097, -1000, 1000, 4097, 65536, 1000000]]).astype(np.float64)
    x = k * vs
    probes = np.concatenate([x] + [_ulps(x, n) for n in (-2, -1, 1, 2)])
    comp = np.concatenate([(k - 0.5) * vs, (k + 0.5) * vs])
    return probes, comp


def boundary_cloud(vs, seed=0, dtype=np.float64):
    """boundary_coordinates(vs) and their companions as 3-D points: on each axis in turn, the other two coordinates at (+-1.25 vs, +-2.25 vs)
    in all four sign combinations (so every octant is met), in a seeded shuffled order.  dtype float32: the probes are k * vs rounded to f32
    and nudged by f32 ulps (dyadic vs: exact)"""
    probes, comp = boundary_coordinates(vs)
    if dtype == np.float32:
        k = probes[: len(probes) // 5].astype(np.float32)
        probes = np.concatenate([k] + [_ulps(k, n) for n in (-2, -1, 1, 2)]).astype(np.float64)
        comp = comp.astype(np.float32).astype(np.float64)
    line = np.concatenate([probes, comp])
    out = []
    for axis in range(3):
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                p = np.empty((len(line), 3))
                p[:, axis] = line
                p[:, (axis + 1) % 3] = sa * 1.25 * vs
                p[:, (axis + 2) % 3] = sb * 2.25 * vs
                out.append(p)
    out = np.concatenate(out)
    out = out[np.random.default_rng(seed).permutation(len(out))]
    return out.astype(dtype)


def range_edge_points(r, ulps=(-3, -2, -1, 0, 1, 2, 3)):
    """points whose norm is exactly r in exact arithmetic - (3, 4, 0) r / 5, (1, 2, 2) r / 3, (2, 3, 6) r / 7, (r, 0, 0), in every
    permutation and sign pattern - each as it is and with its largest coordinate 1, 2 and 3 ulp either side (ulps: the nudges wanted; one level at a time
    keeps the points in voxels of their own)"""
    out = []
    for tri, den in (((3.0, 4.0, 0.0), 5.0), ((1.0, 2.0, 2.0), 3.0), ((2.0, 3.0, 6.0), 7.0), ((1.0, 0.0, 0.0), 1.0)):
        for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
            for sx in (1.0, -1.0):
                for sy in (1.0, -1.0):
                    for sz in (1.0, -1.0):
                        p = np.array(tri)[list(perm)] * np.array([sx, sy, sz]) * r / den
                        j = int(np.argmax(np.abs(p)))
                        for u in ulps:
                            q = p.copy()
                            q[j] = float(_ulps(np.float64(q[j]), u))
                            out.append(q)
    return np.unique(np.array(out) + 0.0, axis=0)


def outlier_cluster():
    """a small lattice cluster about 20 m from the block"""
    return _grid(np.arange(0.0, 2.0, 0.5) + 0.25) + np.array([20.0, 4.0, -3.0])


def sweep_triplet(d, outliers=True, seed=0, H=SWEEP_H, W=SWEEP_W):
    """three frames of the block L seen from 0, d and 2 d (d a dyadic displacement), each padded with (0, 0, 0) to H * W points, float32
    (exact).  Frame 0 is L; frame 1 is L - d where L's x < -0.5; frame 2 is L - 2 d where L's x > 2.5.  Without a guess the
    constant-velocity prediction is the identity for frame 1: every one of its source points starts exactly between 2, 4 or 8 map points.
    Why frames 1 and 2 see different parts: Gauss-Newton brings frame 1 onto the lattice to 1e-13 m, so its points enter the map (8 + 8 per
    voxel fit under a cap of 20) as near-duplicates of L's, and a source point of frame 2 within reach of such a pair would have its nearest
    and second-nearest candidates 1e-13 m apart - a choice that rounding may make either way.  Frame 1's points end in voxels x <= 0, frame
    2's source points stay in voxels x >= 2 and search x >= 1.
    outliers: frames 1 and 2 carry outlier_cluster(), displaced like the block - in frame 1 all 27 voxels around its points are empty at
    every iteration, in frame 2 they hold frame 1's (one copy)"""
    d = np.asarray(d, dtype=np.float64)
    L = lattice_block(seed=seed)
    frames = []
    for k, part in enumerate((L, L[L[:, 0] < -0.5], L[L[:, 0] > 2.5])):
        f = part - k * d
        if outliers and k > 0:
            f = np.concatenate([f, outlier_cluster() - k * d])
        pad = np.zeros((H * W, 3))
        pad[: len(f)] = f
        f32 = pad.astype(np.float32)
        assert np.array_equal(f32.astype(np.float64), pad)
        frames.append(f32)
    return frames


def sweep_t01(H=SWEEP_H, W=SWEEP_W):
    """per-point normalised time of a padded frame: column / W, columns fastest"""
    return np.tile(np.linspace(0.0, 1.0, W, endpoint=False), (H, 1)).reshape(-1)


# ---- a tie that outlives the first iteration: the only way to the tie-break of the 8-lane kernel's answer row
PERSISTENT_TIE_THRESHOLD = 0.1875  # sigma: gate 3 sigma = 0.5625, kernel sigma / 3 = 0.0625


def persistent_tie_pair(H=SWEEP_H, W=SWEEP_W):
    """(frame 0, frame 1, first, last): padded float32 frames and two (64, 3) arrays of offsets candidate - source.
    Frame 1 holds 64 source points, one in every other voxel (x, z in +-1.5, +-3.5; y in +-2.25, +-4.25; shuffled); frame 0 holds, for
    each, four map points in that voxel at (+-0.25, +0.25, +-0.25) from it: a 4-way tie in x and z, and 0.25 m to go in y.  With
    initial_threshold = PERSISTENT_TIE_THRESHOLD every weight of the first iteration is kernel^2 / (kernel + 3/16)^2 = 1/16 exactly, the
    source points are symmetric under a sign flip of each axis, and the FIRST-inserted candidate of a source point lies at
    (sgn / 4, 1/4, sgn / 4), sgn = sign(x y z) of the point - so every sum is a sum of small dyadic numbers (exact in any order), J^T J is
    diagonal, J^T r is zero but for y, and the step is exactly 0.25 m in y without rotation on every implementation.  At the second
    iteration every source point is then still exactly equally far from its four candidates - at a position where the 8-lane kernel
    answers out of its cached row.  The first-inserted candidates balance (no further step: two iterations in all); the LAST-inserted ones
    lie at (1/4, 1/4, -sgn / 4): all on the +x side, so a rule that prefers them walks on.
    first / last: the offsets of the first- and last-inserted candidate of every source point, in frame 1's order"""
    g = np.meshgrid([-3.5, -1.5, 1.5, 3.5], [-4.25, -2.25, 2.25, 4.25], [-3.5, -1.5, 1.5, 3.5], indexing="ij")
    src = np.stack([a.reshape(-1) for a in g], axis=1)
    src = src[np.random.default_rng(5).permutation(len(src))]
    sgn = np.sign(src).prod(axis=1)
    q = np.full(len(src), 0.25)
    first = np.stack([q * sgn, q, q * sgn], axis=1)
    last = np.stack([q, q, -q * sgn], axis=1)
    mid0 = np.stack([-q * sgn, q, q * sgn], axis=1)
    mid1 = np.where((sgn > 0)[:, None], np.stack([-q, q, -q], axis=1), np.stack([-q, q, q], axis=1))
    corners = np.stack([first, mid0, mid1, last], axis=1)
    assert all(len({tuple(c) for c in four}) == 4 for four in corners)
    frames = []
    for f in (np.concatenate([src + corners[:, j] for j in range(4)]), src):  # a voxel's points enter in the order first, mid, mid, last
        pad = np.zeros((H * W, 3))
        pad[: len(f)] = f
        f32 = pad.astype(np.float32)
        assert np.array_equal(f32.astype(np.float64), pad)
        frames.append(f32)
    return frames[0], frames[1], first, last
