"""The lattice scenes of tests/helpers/lattice_scenes.py are what they claim, and the references are entitled to be the reference on them -
before any GPU is involved (tests/test_gpu_search_edges.py runs the kernels on the same scenes).

Everything asserted here is a condition on a scene, not a measurement of the code under test: the C oracle and its independent numpy
restatement agree on it (targets bit for bit, every integer statistic, poses to 1e-12), a third brute-force search picks the same targets,
the scene really contains the hard cases in numbers (ties, distances that equal the gate, coordinates on voxel boundaries, ranges that equal
the limits), and - for the free-running triplets - wherever the device may legitimately differ from the oracle by rounding (from the second
Gauss-Newton iteration on) no decision is closer than GUARD to flipping.
"""
import numpy as np
import pytest

from oracle import cpu as orc
from oracle import icp_numpy as inp
from tests.helpers import lattice_scenes as ls

GUARD = 1e-6  # metres; three orders above the 1e-9 m pose parity the GPU tests assert
# (max_points_per_voxel, initial_threshold) of the triplet runs the GPU tests make
TRIPLET_CONFIGS = ((20, 2.0), (5, 2.0), (20, 0.25))
_OFFS = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def brute_force(map_pts, queries, vs, cap, last=False):
    """third reference: all stored points of the 27 voxels in visiting order, argmin - the FIRST minimum wins (last=True: the last one).
    Returns (targets with NaN rows where the 27 voxels are empty, distances, tied: the minimum is met more than once)"""
    vox = {}
    for p in map_pts:
        lst = vox.setdefault(tuple(np.trunc(p / vs).astype(int)), [])
        if len(lst) < cap:
            lst.append(p)
    tgt, dist, tied = np.full(queries.shape, np.nan), np.full(len(queries), np.inf), np.zeros(len(queries), bool)
    for n, q in enumerate(queries):
        c = np.trunc(q / vs).astype(int)
        cand = [p for o in _OFFS for p in vox.get((c[0] + o[0], c[1] + o[1], c[2] + o[2]), ())]
        if cand:
            cand = np.array(cand)
            d2 = ((cand - q) ** 2).sum(axis=1)
            b = len(d2) - 1 - int(np.argmin(d2[::-1])) if last else int(np.argmin(d2))
            tgt[n], dist[n], tied[n] = cand[b], np.sqrt(d2[b]), (d2 == d2[b]).sum() > 1
    return tgt, dist, tied


def _static_scenes():
    """name -> (map points, queries, gate, points per voxel)"""
    out = {}
    m, q = ls.tie_queries()
    for cap in (20, 5, 32):
        out[f"tie_cap{cap}"] = (m, q, 0.5, cap)
    for name, M in (("gate_dyadic", 0.75), ("gate_3sigma", 3 * 0.35)):
        m, q, _ = ls.gate_queries(M)
        out[name] = (m, q, M, 20)
    return out


@pytest.fixture(scope="module")
def static_runs():
    """every static scene through the three references, once"""
    runs = {}
    for name, (m, q, M, cap) in _static_scenes().items():
        cmap = orc.Map(ls.VOXEL_SIZE, 1e9, cap)
        cmap.add_points(m)
        sums, nc, cand, tgt = cmap.linear_system(q, M, M / 9.0, want_targets=True)
        nmap = inp.VoxelMap(ls.VOXEL_SIZE, 1e9, cap)
        nmap.add(m)
        npts, nd2, found, ncand = inp.nearest(q, nmap.tables(), ls.VOXEL_SIZE)
        runs[name] = dict(q=q, M=M, cap=cap, c=(nc, cand, tgt), n=(npts, nd2, found, ncand), first=brute_force(m, q, ls.VOXEL_SIZE, cap),
                          last=brute_force(m, q, ls.VOXEL_SIZE, cap, last=True))
    return runs


def test_three_references_pick_the_same_targets_on_the_static_scenes(static_runs):
    for name, r in static_runs.items():
        (nc, cand, tgt), (npts, nd2, found, ncand), (btgt, bdist, _) = r["c"], r["n"], r["first"]
        paired = found & (np.sqrt(nd2) < r["M"])
        assert (nc, cand) == (int(paired.sum()), ncand), (name, nc, cand, int(paired.sum()), ncand)
        assert np.array_equal(np.isnan(tgt[:, 0]), ~paired), name
        assert np.array_equal(tgt[paired], npts[paired]), name                       # bit for bit
        assert np.array_equal(np.isfinite(bdist), found), name
        assert np.array_equal(btgt[found], npts[found]) and np.array_equal(bdist[found], np.sqrt(nd2[found])), name
        assert 0 < nc < len(r["q"]), (name, nc)                                       # the gate takes some and leaves some


def test_static_scenes_have_teeth(static_runs):
    r = static_runs["tie_cap20"]
    (_, dist, tied), (ltgt, _, _) = r["first"], r["last"]
    tgt = r["c"][2]
    paired = ~np.isnan(tgt[:, 0])
    n_tied, n_gate = int(tied.sum()), int((dist == r["M"]).sum())
    n_last = int((ltgt[paired] != tgt[paired]).any(axis=1).sum())
    zero = int((dist == 0.0).sum())
    print(f"tie queries: {len(r['q'])}, tied {n_tied}, nearest at exactly the gate {n_gate}, at distance 0 {zero}, last-minimum-wins differs on {n_last}")
    assert n_tied >= 1000 and n_last >= 1000, (n_tied, n_last)
    assert n_gate >= 50, n_gate
    assert zero >= 100, zero
    for cap in (5, 32):
        rc = static_runs[f"tie_cap{cap}"]
        n = int((rc["last"][0][~np.isnan(rc["c"][2][:, 0])] != rc["c"][2][~np.isnan(rc["c"][2][:, 0])]).any(axis=1).sum())
        assert n >= 500, (cap, n)  # (a cap of 5 leaves fewer candidates to tie; still hundreds of tie decisions)
    for name, M in (("gate_dyadic", 0.75), ("gate_3sigma", 3 * 0.35)):
        _, q, exact = ls.gate_queries(M)
        dist = static_runs[name]["first"][1]
        assert np.isfinite(dist).all(), name                                          # every query sees its map point
        at, below, above = int((dist == M).sum()), int((dist < M).sum()), int((dist > M).sum())
        print(f"{name}: {len(q)} queries, {at} at exactly the gate, {below} below, {above} above; un-nudged ones that round off the gate: {int((dist[exact] != M).sum())}")
        assert at >= 12 and below >= 50 and above >= 50, (name, at, below, above)
        paired = ~np.isnan(static_runs[name]["c"][2][:, 0])
        assert np.array_equal(paired, dist < M), name                                 # strictly smaller: a distance of exactly M is out


def test_boundary_coordinates_defeat_the_reciprocal_and_the_references_agree():
    wrong = 0
    for vs in ls.VOXEL_SIZES:
        probes, comp = ls.boundary_coordinates(vs)
        wrong += int((np.trunc(probes * (1.0 / vs)) != np.trunc(probes / vs)).sum())
        # a companion is well inside its voxel: the same voxel by either formula, and the neighbours of the probe's boundary
        assert np.array_equal(np.trunc(comp * (1.0 / vs)), np.trunc(comp / vs)), vs
        cloud = ls.boundary_cloud(vs)
        nmap = inp.VoxelMap(vs, 1e9, 20)
        nmap.add(cloud)
        for cap in (20, 1):
            cmap = orc.Map(vs, 1e9, cap)
            cmap.add_points(cloud)
            want = np.array([p for lst in nmap.vox.values() for p in lst[:cap]])
            assert (cmap.num_voxels, cmap.num_points) == (len(nmap.vox), len(want)), (vs, cap)
            assert np.array_equal(_sorted_rows(cmap.points()), _sorted_rows(want)), (vs, cap)
        fd = inp.voxel_downsample(cloud, 0.5 * vs)
        assert np.array_equal(orc.voxel_downsample(cloud, 0.5 * vs), fd), vs
        assert np.array_equal(orc.voxel_downsample(fd, 1.5 * vs), inp.voxel_downsample(fd, 1.5 * vs)), vs
    print(f"boundary coordinates: trunc(x * (1 / vs)) != trunc(x / vs) on {wrong} of {len(ls.VOXEL_SIZES) * len(probes)}")
    assert wrong >= 100, wrong
    for vs in (1.0, 0.5, 0.25):  # the f32 clouds hold the same values once widened
        c32 = ls.boundary_cloud(vs, dtype=np.float32)
        k = np.round(c32.astype(np.float64) / (0.5 * vs))
        assert (np.abs(c32.astype(np.float64) - k * 0.5 * vs) <= 4 * np.spacing(np.abs(c32)).astype(np.float64)).any(axis=1).all(), vs
        assert np.isfinite(c32).all()


def test_range_edge_points_sit_on_both_sides_of_the_limits():
    for r in (ls.MIN_RANGE, ls.MAX_RANGE):
        p = ls.range_edge_points(r)
        n = np.linalg.norm(p, axis=1)
        at, below, above = int((n == r).sum()), int((n < r).sum()), int((n > r).sum())
        print(f"range edge r = {r}: {len(p)} points, {at} at exactly r, {below} below, {above} above")
        assert at >= 50 and below >= 50 and above >= 50, (r, at, below, above)
        keep = (n > ls.MIN_RANGE) & (n < ls.MAX_RANGE)
        assert np.array_equal(orc.preprocess(p, ls.MAX_RANGE, ls.MIN_RANGE), p[keep]), r
        assert np.abs(n - r).max() <= 4 * np.spacing(r)


# ---------------------------------------------------------------------------------------------- triplets
def _top2(s, tables, vs):
    """distances to the nearest and the second-nearest candidate of the 27 voxels (inf where there is none)"""
    code, pts, _ = tables
    k0 = inp.voxel_index(s, vs)
    rows = np.empty((len(s), 27), dtype=np.int64)
    for o, off in enumerate(_OFFS):
        c = inp._code(k0 + np.array(off))
        pos = np.minimum(np.searchsorted(code, c), len(code) - 1)
        rows[:, o] = np.where(code[pos] == c, pos, len(code))
    d2 = np.sort(np.sum((pts[rows].reshape(len(s), -1, 3) - s[:, None, :]) ** 2, axis=2), axis=1)
    return np.sqrt(d2[:, 0]), np.sqrt(d2[:, 1])


def _boundary_margin(s, vs):
    """distance of every coordinate to the nearest voxel boundary k * vs, k != 0 (truncation toward zero: 0 is inside a voxel)"""
    k = np.maximum(np.round(np.abs(s) / vs), 1.0)
    return np.abs(np.abs(s) - k * vs).min()


def _run_triplet(d, cap, th, monkeypatch):
    """the triplet through both references; returns (oracle, numpy restatement, per-frame list of per-iteration (d1, d2, boundary margin,
    which source points belong to the outlier cluster))"""
    frames, t01 = ls.sweep_triplet(d), ls.sweep_t01()
    ref = orc.ICP(ls.MAX_RANGE, ls.MIN_RANGE, max_points_per_voxel=cap, initial_threshold=th)
    num = inp.KissICP(ls.MAX_RANGE, ls.MIN_RANGE)
    num.map.cap, num.initial_threshold = cap, th
    seen = []
    real = inp.nearest

    def spy(s, tables, vs):
        seen[-1].append(_top2(s, tables, vs) + (_boundary_margin(s, vs), s[:, 0] > 12.0))
        return real(s, tables, vs)

    monkeypatch.setattr(inp, "nearest", spy)
    for f in frames:
        seen.append([])
        ref.register_frame(f.astype(np.float64), t01)
        num.register_frame(f.astype(np.float64), t01)
    return ref, num, seen


@pytest.mark.parametrize("cap,th", TRIPLET_CONFIGS)
@pytest.mark.parametrize("d", ls.DISPLACEMENTS)
def test_triplet_references_agree_and_keep_the_guard(d, cap, th, monkeypatch):
    ref, num, seen = _run_triplet(d, cap, th, monkeypatch)
    assert ref.cfg.voxel_size == num.vs == ls.VOXEL_SIZE
    for k in range(3):
        a, b = ref.stats[k], num.stats[k]
        for key in ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points"):
            assert a[key] == b[key], (k, key, a[key], b[key])
        assert np.abs(ref.pose(k) - num.poses[k]).max() <= 1e-12, k
        assert len(seen[k]) == a["iterations"]
    assert ref.stats[0]["iterations"] == 0 and ref.stats[1]["iterations"] >= 2 and ref.stats[2]["iterations"] >= 1
    # frame 1 starts from the identity: its first iteration is exact everywhere, and full of ties
    d1, d2, _, _ = seen[1][0]
    tied, n1 = int((np.isfinite(d1) & (d1 == d2)).sum()), len(d1)
    empty = int(np.isinf(np.array([it[0] for it in seen[1]])).all(axis=0).sum())
    assert tied >= 100, tied
    assert empty >= 1, empty                                  # the outliers: all 27 voxels empty at every iteration of frame 1
    assert np.isfinite(seen[2][0][0][seen[2][0][3]]).any()    # ... and in frame 2 they have neighbours: frame 1's
    if th == 0.25:
        assert any(s["n_corr_last"] < s["n_src"] for s in ref.stats[1:]), [(s["n_corr_last"], s["n_src"]) for s in ref.stats]
    # the guard: where rounding may differ between implementations, no decision is within GUARD of flipping
    m_second = m_gate = m_bound = np.inf
    for k in (1, 2):
        gate = 3.0 * ref.stats[k]["sigma"]
        for it, (d1, d2, mb, _) in enumerate(seen[k]):
            if k == 1 and it == 0:
                continue
            has, two = np.isfinite(d1), np.isfinite(d2)
            m_second = min(m_second, (d2[two] - d1[two]).min())
            m_gate = min(m_gate, np.abs(d1[has] - gate).min())
            m_bound = min(m_bound, mb)
    print(f"d = {d}, cap {cap}, threshold {th}: tied at iteration 0 of frame 1 {tied} of {n1}, source points with 27 empty voxels {empty}, "
          f"iterations {[s['iterations'] for s in ref.stats]}, smallest margins: second nearest {m_second:.3g} m, gate {m_gate:.3g} m, "
          f"voxel boundary {m_bound:.3g} m")
    assert m_second >= GUARD and m_gate >= GUARD and m_bound >= GUARD, (m_second, m_gate, m_bound)


# ---------------------------------------------------------------------------------------------- the tie that outlives the first iteration
def _nearest_last(s, tables, vs):
    """icp_numpy.nearest with the LAST of the smallest distances winning"""
    code, pts, cnt = tables
    k0 = inp.voxel_index(s, vs)
    rows = np.empty((len(s), 27), dtype=np.int64)
    for o, off in enumerate(_OFFS):
        c = inp._code(k0 + np.array(off))
        pos = np.minimum(np.searchsorted(code, c), len(code) - 1)
        rows[:, o] = np.where(code[pos] == c, pos, len(code))
    cand = pts[rows].reshape(len(s), -1, 3)
    d2 = np.sum((cand - s[:, None, :]) ** 2, axis=2)
    best = d2.shape[1] - 1 - np.argmin(d2[:, ::-1], axis=1)
    ar = np.arange(len(s))
    return cand[ar, best], d2[ar, best], np.isfinite(d2[ar, best]), int(cnt[rows].sum())


def test_persistent_tie_pair_is_exact_and_only_the_first_minimum_stops_after_two_iterations(monkeypatch):
    f0, f1, first, last = ls.persistent_tie_pair()
    t01 = ls.sweep_t01()
    src = f1[:64].astype(np.float64)
    # the scene: four candidates per source point, 4-way tied at the start and after the exact step of 0.25 m in y
    for pos in (src, src + np.array([0.0, 0.25, 0.0])):
        d2 = ((f0[:256].astype(np.float64)[None, :, :] - pos[:, None, :]) ** 2).sum(axis=2)
        near = np.sort(d2, axis=1)
        assert (near[:, 0] == near[:, 3]).all() and (near[:, 4] > 2.0).all()
    assert not first[:, [0, 2]].sum(axis=0).any() and last[:, 0].sum() == 16.0  # the first-inserted balance, the last-inserted do not
    for a in range(3):  # ... also about every axis: sum of s x r over the first-inserted is zero
        assert not np.cross(src + np.array([0.0, 0.25, 0.0]), first - np.array([0.0, 0.25, 0.0])).sum(axis=0)[a]
    runs = {}
    for rule in ("first", "last"):
        if rule == "last":  # ... from the second iteration on: what a wrong tie-break in the answer row alone would do
            real, calls = inp.nearest, []
            monkeypatch.setattr(inp, "nearest", lambda *a: (calls.append(0), real(*a) if len(calls) == 1 else _nearest_last(*a))[1])
        num = inp.KissICP(ls.MAX_RANGE, ls.MIN_RANGE)
        num.initial_threshold = ls.PERSISTENT_TIE_THRESHOLD
        for f in (f0, f1):
            num.register_frame(f.astype(np.float64), t01)
        runs[rule] = num
    ref = orc.ICP(ls.MAX_RANGE, ls.MIN_RANGE, initial_threshold=ls.PERSISTENT_TIE_THRESHOLD)
    for f in (f0, f1):
        ref.register_frame(f.astype(np.float64), t01)
    num = runs["first"]
    for k in range(2):
        for key in ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points"):
            assert ref.stats[k][key] == num.stats[k][key], (k, key)
        assert np.abs(ref.pose(k) - num.poses[k]).max() <= 1e-12
    st = ref.stats[1]
    assert (st["n_src"], st["iterations"], st["n_corr_last"], st["sum_cand"]) == (64, 2, 64, 2 * 64 * 4), st
    for T in (ref.pose(1), num.poses[1]):  # the first step is exact; the second one is rounding of a balanced sum
        assert T[1, 3] == 0.25 and np.abs(T - np.eye(4))[[0, 2], 3].max() < 1e-15 and np.abs(T[:3, :3] - np.eye(3)).max() < 1e-15, T
    wrong = runs["last"]
    print(f"persistent tie: first minimum wins {st['iterations']} iterations; last minimum wins {wrong.stats[1]['iterations']} iterations, "
          f"{np.linalg.norm(wrong.poses[1][:3, 3] - ref.pose(1)[:3, 3]):.3g} m away")
    assert wrong.stats[1]["iterations"] > 2 and np.linalg.norm(wrong.poses[1][:3, 3] - ref.pose(1)[:3, 3]) > 1e-3
