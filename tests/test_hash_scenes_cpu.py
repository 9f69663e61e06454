"""tests/helpers/hash_scenes.py without a GPU: the restated hash against known answers and against the key packing of tools/layout_sim.py, the
table simulator's rules, and - with the simulator alone - that the scenes of tests/test_gpu_hash_tables.py contain the hard cases in numbers:
long chains, chains that wrap past slot 0, live voxels behind tombstones, a table that really fills.  These are conditions on the inputs,
not tolerances."""
import ast
import os

import numpy as np
import pytest

from tests.helpers import hash_scenes as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 12


def _fmix64(h):
    """the finaliser on Python integers: shares nothing with the numpy restatement"""
    m = (1 << 64) - 1
    h ^= h >> 33
    h = h * 0xFF51AFD7ED558CCD & m
    h ^= h >> 33
    h = h * 0xC4CEB9FE1A85EC53 & m
    return h ^ h >> 33


def _table_of(vox, cap):
    t = hs.Table(cap)
    for k in hs.pack_key(vox).tolist():
        t.insert(k)
    return t


# ------------------------------------------------------------------------------------------------ the restatement
def test_mix64_known_answers():
    """0 is the finaliser's fixed point; 1 -> 0xB456BCFC34C2CB2C is the value every MurmurHash3 port quotes; 2, 2^33 (the first input the
    opening shift changes) and all ones worked out step by step on Python integers and written down; then that arithmetic against the numpy one"""
    known = {0: 0, 1: 0xB456BCFC34C2CB2C, 2: 0x3ABF2A20650683E7, 1 << 33: 0x6B80F8591E1145C3, 0xFFFFFFFFFFFFFFFF: 0x64B5720B4B825F21}
    for x, want in known.items():
        assert int(hs.mix64(np.uint64(x))) == want == _fmix64(x), hex(x)
    for x in (1 << 33, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF, int(hs.pack_key(np.array([0, 0, 0])))):
        assert int(hs.mix64(np.uint64(x))) == _fmix64(x), hex(x)
    x = np.random.default_rng(0).integers(0, 1 << 63, 1000).astype(np.uint64)
    assert [int(v) for v in hs.mix64(x)] == [_fmix64(int(v)) for v in x]


def test_pack_key_is_the_packing_of_layout_sim():
    """tools/layout_sim.py packs its voxel keys like the kernels; its two functions are taken out of its source (the tool runs on import)"""
    tree = ast.parse(open(os.path.join(ROOT, "tools", "layout_sim.py")).read())
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("keys", "pack"):
            exec(compile(ast.Module([node], []), "layout_sim", "exec"), ns)
    rng = np.random.default_rng(1)
    p = rng.uniform(-300.0, 300.0, (4000, 3))
    for vs in (1.0, 0.5, 0.7):
        k = ns["keys"](p, vs)
        assert np.array_equal(k, hs.voxel_of(p, vs))
        assert np.array_equal(ns["pack"](k).astype(np.uint64), hs.pack_key(k))
    k = np.array([[-(1 << 20), 0, (1 << 20) - 1], [5, -7, 9]])
    assert np.array_equal(hs.unpack_key(hs.pack_key(k)), k)
    assert int(hs.pack_key(k)[0]) == ((1 << 21) - 1) | (1 << 20) << 21


def test_brick_slot_and_table_sizes():
    """the 8 voxels of a brick take the 8 entries of one line in (x, y, z) bit order; another brick another hash; the per-scan table sizes"""
    for b in ([0, 0, 0], [-3, 7, 100], [-1, -1, -1]):
        vox = 2 * np.array(b) + hs._FINE
        s = hs.brick_slot(hs.pack_key(vox), CAP - 1)
        assert np.array_equal(s, s[0] + np.arange(8)) and s[0] % 8 == 0
        h = _fmix64(int(hs.pack_key(2 * np.array(b))))
        assert s[0] == ((h & 0xFFFFFFFF) << 3) & 0xFFFFFFFF & (CAP - 1)
    assert hs.vds_table_slots(64, 2048) == 1 << 17 and hs.vds_table_slots(16, 2048) == 1 << 15
    assert hs.vds_table_slots(64, 1) == 1024 and hs.vds_table_slots(16, 131072) == 1 << 21 and hs.vds_table_slots(64, 3000) == 1 << 18
    p = hs.points_in(np.array([[0, -1, 5], [-64, 63, 0]]), np.array([[0.25, 0.5, 0.75], [0.75, 0.25, 0.5]]))
    assert np.array_equal(p, [[0.25, -1.5, 5.75], [-64.75, 63.25, 0.5]]) and np.array_equal(hs.voxel_of(p, 1.0), [[0, -1, 5], [-64, 63, 0]])


def test_simulator_rules():
    """a search walks past a tombstone, an insert does not reuse it, `used` counts tombstones, a rebuild drops them"""
    vox = hs.homing_voxels(64, [7])  # the last line of a 64-slot table
    a, b, c = (int(k) for k in hs.pack_key(vox[[0, 8, 16]]))  # three bricks' first voxels: one home slot
    t = hs.Table(64)
    assert [t.insert(k) for k in (a, b, c)] == [(56, True), (57, True), (58, True)] and t.used == 3
    t.remove(b)
    assert t.find(c) == 58 and t.find(b) == -1 and t.tombstones() == 1
    assert t.insert(b) == (59, True) and t.used == 4 and t.insert(c) == (58, False)
    disp, wrapped, behind = t.chain_stats()
    assert disp.tolist() == [0, 2, 3] and not wrapped.any() and behind.tolist() == [0, 1, 1]
    for k in hs.pack_key(vox[24:24 + 8 * 4:8]).tolist():
        t.insert(k)
    assert t.find(int(hs.pack_key(vox[48]))) == (56 + 7) % 64  # 56 57T 58 59 60 61 62 63 -> the next one wraps
    assert t.insert(int(hs.pack_key(vox[56]))) == (0, True)
    assert t.chain_stats()[1].sum() == 1
    t.rebuild([a, c])
    assert t.used == 2 and t.tombstones() == 0 and (t.find(a), t.find(c)) == (56, 57)
    assert not t.exhausted
    t.used = 49
    assert t.exhausted


# ------------------------------------------------------------------------------------------------ the scenes
def test_wrap_and_cluster_scenes():
    vox, pts, own = hs.wrap_scene(CAP, 200)
    assert np.array_equal(hs.voxel_of(pts, 1.0), vox[own]) and len(np.unique(hs.pack_key(vox))) == 200
    assert set(np.unique(own)) == set(range(200)) and (np.bincount(own) > 1).any()
    assert set(hs.brick_slot(hs.pack_key(vox), CAP - 1) >> 3) == {CAP // 8 - 2, CAP // 8 - 1}
    disp, wrapped, _ = _table_of(vox, CAP).chain_stats()
    assert wrapped.sum() >= 100 and disp.max() >= 128, (wrapped.sum(), disp.max())
    assert (wrapped.sum(), disp.max()) == (184, 184)  # the figures DESIGN.md 3.15.1 quotes
    vox, pts, own = hs.cluster_scene(CAP, 100, 120)
    assert set(hs.brick_slot(hs.pack_key(vox), CAP - 1) >> 3) == {100, 101}
    disp, wrapped, _ = _table_of(vox, CAP).chain_stats()
    assert not wrapped.any() and disp.max() >= 100
    assert not np.isin(hs.pack_key(hs.absent_voxels(CAP, 100, 120, 24)), hs.pack_key(vox)).any()


@pytest.mark.parametrize("load", (0.65, 0.70, 0.74))
def test_dense_scene(load):
    vox, pts = hs.dense_scene(CAP, load)
    assert len(np.unique(hs.pack_key(vox))) == len(vox) == int(load * CAP)
    keys, counts = np.unique(hs.pack_key(hs.voxel_of(pts, 1.0)), return_counts=True)
    assert np.array_equal(keys, np.unique(hs.pack_key(vox))) and counts.min() >= 1 and counts.max() > 20  # the 20-point cap binds
    disp, _, _ = _table_of(vox, CAP).chain_stats()
    assert (disp > 0).mean() >= 0.30 and disp.max() >= 16, ((disp > 0).mean(), disp.max())
    if load == 0.70:  # the figures DESIGN.md 3.15.1 quotes
        assert round(100 * (disp > 0).mean()) == 36 and disp.max() == 38


@pytest.mark.parametrize("which", (1, 2))
def test_vds_scenes(which):
    pts, vox, size, cap = hs.vds_scene(2048, which)
    assert len(pts) <= 2048 and cap == (1 << 17 if which == 1 else 1 << 15)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)  # exact as f32 input
    keys, counts = np.unique(hs.pack_key(hs.voxel_of(pts, size)), return_counts=True)
    assert np.array_equal(keys, np.unique(hs.pack_key(vox))) and (counts == 4).all()
    for shift in (0.0625, -0.0625):  # the second scan of the GPU test is moved by these: the same voxels
        assert np.array_equal(hs.voxel_of(pts + shift, size), hs.voxel_of(pts, size))
        assert np.array_equal(hs.voxel_of(pts + shift, 0.5), hs.voxel_of(pts, 0.5))
    disp, wrapped, _ = _table_of(vox, cap).chain_stats()
    assert (disp > 0).sum() >= 100 and wrapped.any(), ((disp > 0).sum(), wrapped.sum())
    if which == 2:  # pass 1 keeps three of a voxel's four points, and which one pass 2 keeps is decided among those
        k1, first = np.unique(hs.pack_key(hs.voxel_of(pts, 0.5)), return_index=True)
        assert len(k1) == 3 * len(vox)
        kept = pts[np.sort(first)]
        assert (np.unique(hs.pack_key(hs.voxel_of(kept, 1.5)), return_counts=True)[1] == 3).all()


def test_map_stage_scene():
    sc = hs.map_stage_scene(CAP)
    m = hs.MapSim(CAP, 1.0, sc["max_range"])
    for b in sc["batches"]:
        assert 0 < len(b) and len(b) % 256 != 0
        m.add(b)
    disp, wrapped, _ = m.tab.chain_stats()
    assert wrapped.sum() >= 100 and disp.max() >= 128 and m.tab.used == m.n_live == len(sc["colliding"]) + len(sc["background"])
    assert m.tab.find(int(hs.pack_key(sc["absent"][0]))) == -1
    n_before = m.n_live
    m.prune(sc["origin"])
    gone = n_before - m.n_live
    _, _, behind = m.tab.chain_stats()
    assert (behind > 0).sum() >= 50, (behind > 0).sum()
    assert (behind > 0).sum() == 253  # the figure DESIGN.md 3.15.1 quotes
    assert m.tab.tombstones() == gone >= sc["far"].sum() >= 100 and m.tab.used == n_before
    live_before = set(m.first)
    m.add(sc["reinsert"])
    recreated = sc["colliding"][sc["far"]][::2]
    again = set(hs.pack_key(hs.voxel_of(sc["reinsert"], 1.0)).tolist())
    assert len(recreated) >= 50 and set(hs.pack_key(recreated).tolist()) <= again - live_before and len(again & live_before) >= 100
    assert m.tab.used == n_before + len(again - live_before) and m.tab.tombstones() == gone and not m.tab.exhausted
    slots = [m.tab.find(int(k)) for k in hs.pack_key(recreated)]
    _, _, behind = m.tab.chain_stats()
    live_slots = m.tab.live()[0]
    assert all((behind[live_slots == s] > 0).all() for s in slots)  # each sits behind its own tombstone at least


def test_exhaustion_steps():
    steps, max_range = hs.exhaustion_steps()
    m = hs.MapSim(1 << 10, 1.0, max_range)
    first = None
    for i, (p, o) in enumerate(steps):
        m.add(p)
        m.prune(o)
        if m.tab.exhausted and first is None:
            first = i
            assert m.n_live < 1 << 8 and m.tab.used < 1 << 10  # the tombstones fill it, not the voxels; and the table is not full yet
    assert first is not None and first >= 4
    assert first == 8  # the ninth call - DESIGN.md 3.15.1 quotes it, with 856 entries used and 169 voxels live then
    m = hs.MapSim(1 << 10, 1.0, max_range)
    for p, o in steps[:9]:
        m.add(p)
        m.prune(o)
    assert (m.tab.used, m.n_live) == (856, 169)


def test_drive_reference():
    """the drive of the rebuild tests through the oracle and the simulator (tests/helpers/hash_drive.py asserts the conditions - the table is the
    smallest that never passes 3/4, its peak load is at least 1/2, the registration follows the drive - while it builds the reference): the
    answers the GPU drivers are held against, as DESIGN.md 3.15.1 quotes them"""
    from tests.helpers import hash_drive as hd
    ref = hd.drive_reference()
    assert ref["cap"] == 1 << 12 and max(ref["used"]) >= ref["cap"] // 2 and max(ref["used"]) <= ref["cap"] // 4 * 3
    assert max(ref["used"]) == 2344 and ref["sim"].tab.tombstones() == 207 and ref["refused"] == 12
    assert hd.DRIVE_N % hd.REBUILD_EVERY == 2  # two scans of tombstones since the last rebuild
    assert len(ref["frames"]) == len(ref["stats"]) == hd.DRIVE_N and all(f.shape == (hd.DRIVE_PTS, 3) for f in ref["frames"])
