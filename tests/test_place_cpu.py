"""The place descriptors without a device: the numpy restatement's own properties, the header against the binding, the
refusals that come before any HIP call, the host policy of `fly.LoopFinder` / `fly.PlaceLocalizer` on hand-made integer results, the places
file's round trip and refusals, the commands' refusals, and the functional scene's precondition on the restatement alone."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib, core, fly
from ptudes_lab_amd import utils as pu
from tests.helpers import abi_surface
from tests.helpers import place_cases as pc
from tests.helpers import place_numpy as pn

PTL_ERR_ARG = -1
NEW = {"ptl_place_sizeof_cfg", "ptl_place_default_cfg", "ptl_place_create", "ptl_place_destroy", "ptl_place_clear", "ptl_place_size",
       "ptl_place_tables", "ptl_place_profile", "ptl_place_describe_range", "ptl_place_describe_xyz", "ptl_place_match", "ptl_place_match_all",
       "ptl_place_read", "ptl_place_load"}
CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


# ---------------------------------------------------------------------------------------------- 1. the restatement's own properties
@pytest.mark.parametrize("R,S", pc.CONFIGS)
def test_a_permutation_of_the_points_gives_the_same_descriptor(R, S):
    e, d = pn.tables(R, S, pc.PARAMS["min_radius"], pc.PARAMS["max_radius"])
    z_min, z_step = pc.PARAMS["z_min"], pc.PARAMS["z_step"]
    pts = np.concatenate([pc.edge_points(e, d, z_min, z_step), pc.random_points(3, 5000, pc.PARAMS["max_radius"], z_min, z_step)])
    want, winfo = pn.describe(pts, e, d, z_min, z_step)
    rng = np.random.default_rng(1)
    for _ in range(3):
        got, info = pn.describe(pts[rng.permutation(len(pts))], e, d, z_min, z_step)
        assert np.array_equal(got, want) and info == winfo
    assert (want[:, R:] == 0).all() and winfo["n_cells"] == int((want != 0).sum())
    assert sum(winfo[k] for k in pn.INFO_FIELDS[1:7]) == winfo["n_points"] == len(pts)
    # the identity levels nothing; the binning edges are all there
    same, sinfo = pn.describe(pts, e, d, z_min, z_step, rot=np.eye(3))
    assert np.array_equal(same, want) and sinfo == winfo
    ring, sector, level, why = pn.bins(pts, e, d, z_min, z_step)
    assert {0, 1, 2, 3, 5} <= set(why.tolist()) and {1, 2, 254, 255} <= set(level[why == 0].tolist())
    re = pn.bins(pc.ring_edge_points(e, 0.0), e, d, z_min, z_step)
    for i in range(R + 1):
        assert len({(re[3][3 * i + k], re[0][3 * i + k]) for k in range(3)}) >= 2, f"both sides of ring edge {i}"


@pytest.mark.parametrize("R,S", pc.CONFIGS)
def test_every_roll_matches_at_its_shift_and_the_tie_rules(R, S):
    q = pc.distinct_descriptor(R, S)
    for k in range(S):
        assert pn.best_shift(q, np.roll(q, -k, axis=0)) == (0, k)
    # all-equal columns: every shift ties, the smallest wins
    flat = np.zeros_like(q)
    flat[:, :R] = 9
    assert pn.best_shift(flat, flat) == (0, 0) and len(set(pn.dists(q, flat).tolist())) == 1 and pn.best_shift(q, flat)[1] == 0
    # equal entries: the smaller index wins, in match and in match_all
    entries = np.array([flat, q, q, flat])
    assert pn.match(q, entries)[2] == 1 and pn.match(flat, entries)[2] == 0
    e, dist, shift = pn.match_all(entries, 1)
    assert list(e) == [-1, 0, 1, 0] and dist[2] == 0 and dist[3] == 0
    e0 = pn.match_all(entries, 0)[0]
    assert list(e0) == [0, 1, 1, 0], "with min_gap 0 an entry meets itself, unless an equal one came first"
    assert list(pn.match_all(entries, 4)[0]) == [-1] * 4
    # the table form is the pairwise form
    descs = pc.random_descriptors(2, 9, R, S)
    td, ts = pn.pair_table(descs, full_rows={0, 8})
    for i in range(9):
        for j in range(9 if i in (0, 8) else i + 1):
            assert (td[i, j], ts[i, j]) == pn.best_shift(descs[i], descs[j])
    assert (td[3, 4:] == -1).all()
    # dist is bounded by 64 64 255 and symmetric in the sense dist(q, c, s) == dist(c, q, -s)
    a, b = descs[0], descs[1]
    assert np.array_equal(pn.dists(a, b), np.roll(pn.dists(b, a)[::-1], 1))


def test_a_turn_about_z_is_a_shift_of_the_sectors():
    """the convention: points turned by +k sectors about z give a descriptor whose best shift against the original is k, dist 0 - exact here
    because the points sit in the middle of their sectors"""
    R, S = 20, 60
    e, d = pn.tables(R, S, 1.0, 80.0)
    rng = np.random.default_rng(4)
    ang = (rng.integers(0, S, 400) + 0.5) * 2.0 * np.pi / S
    rad = rng.uniform(2.0, 70.0, 400)
    pts = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1.0, 9.0, 400)], axis=1)
    base, _ = pn.describe(pts, e, d, -2.0, 0.0625)
    for k in (1, 16, 59):
        turned, _ = pn.describe(pts @ pc.rot_z(360.0 * k / S).T, e, d, -2.0, 0.0625)
        assert pn.best_shift(turned, base) == (0, k)
        assert np.allclose(core.place_shift_pose(k, S)[:3, :3], pc.rot_z(-360.0 * k / S), atol=1e-15)


def test_the_functional_scene_on_the_restatement():
    """tests/test_gpu_place.py's functional test expects every turned sweep to find its own entry; that the definition gives this is checked
    here.  Measured: own entry 4 762 / 15 494 / 0 at shifts 16 / 34 / 59 for 97 / 201 / 354 degrees, the next best entry about 40 570"""
    sweeps, own = pc.functional_sweeps()
    e, d = pn.tables(20, 60, 1.0, 40.0)
    D = np.array([pn.describe(s.astype(np.float32), e, d, -2.0, 1.0 / 16.0)[0] for s in sweeps])
    for deg, want in zip(pc.FUNCTIONAL["turns_deg"], ((4762, 16), (15494, 34), (0, 59))):
        q, _ = pn.describe(pc.turned(sweeps[own], deg), e, d, -2.0, 1.0 / 16.0)
        dist, shift, best = pn.match(q, D)
        assert best == own and (int(dist[own]), int(shift[own])) == want and np.delete(dist, own).min() > 2 * int(dist[own])


# ---------------------------------------------------------------------------------------------- 2. header, binding, refusals
def test_header_against_binding_field_by_field():
    for name, struct in (("ptl_place_cfg", _lib.PlaceCfg), ("ptl_place_info", _lib.PlaceInfo), ("ptl_place_result", _lib.PlaceResult)):
        want = [(f, CTYPES[t]) for f, t, n in abi_surface.struct_fields(name) if n is None]
        assert want == [(f, t) for f, t in struct._fields_], name
    assert C.sizeof(_lib.PlaceCfg) == 64 and C.sizeof(_lib.PlaceInfo) == 72 and C.sizeof(_lib.PlaceResult) == 40
    assert NEW <= abi_surface.declared() and NEW <= set(_lib.PROTOTYPES)
    assert _lib.ABI_VERSION == 6 and _lib.PLACE_INFO_FIELDS == pn.INFO_FIELDS


def test_surface_and_refusals_before_any_hip_call():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    L = _lib.lib()
    assert NEW <= abi_surface.exported(_lib.LIB_PATH)
    assert L.ptl_abi_version() == 6 and L.ptl_place_sizeof_cfg() == C.sizeof(_lib.PlaceCfg)
    assert L.ptl_sizeof_cfg(6) == -1, "ptl_sizeof_cfg keeps its ids"
    cfg = core.place_cfg()
    assert {k: getattr(cfg, k) for k in pu.PLACE_CFG_KEYS} == pn.DEFAULTS and (cfg.capacity, cfg.max_points_per_scan) == (4096, 1 << 20)

    class Guarded(C.Structure):  # a canary behind the cfg: a library that believed another size would write into it
        _fields_ = [("cfg", _lib.PlaceCfg), ("canary", C.c_uint64 * 4)]

    g = Guarded()
    for size, abi in ((C.sizeof(_lib.PlaceCfg) - 8, _lib.ABI_VERSION), (C.sizeof(_lib.PlaceCfg) + 8, _lib.ABI_VERSION),
                      (C.sizeof(_lib.PlaceCfg), _lib.ABI_VERSION + 1)):
        g.cfg.struct_size, g.cfg.abi_version, g.cfg.max_radius = size, abi, 123.0
        for i in range(4):
            g.canary[i] = 0xA5A5A5A5A5A5A5A5
        assert L.ptl_place_default_cfg(C.byref(g.cfg)) == PTL_ERR_ARG
        msg = L.ptl_last_error().decode()
        assert str(size) in msg and "64" in msg and g.cfg.max_radius == 123.0 and list(g.canary) == [0xA5A5A5A5A5A5A5A5] * 4
        h = C.c_void_p()
        assert L.ptl_place_create(0, C.byref(g.cfg), C.byref(h)) == PTL_ERR_ARG and not h.value
    # every parameter bound, with its numbers, before a device is looked for
    for over, words in ((dict(n_ring=0), ["n_ring = 0", "1 .. 64"]), (dict(n_ring=65), ["n_ring = 65"]), (dict(n_sector=3), ["n_sector = 3", "4 .. 64"]),
                        (dict(n_sector=65), ["n_sector = 65"]), (dict(min_radius=0.0), ["min_radius = 0"]),
                        (dict(min_radius=4.0), ["min_radius = 4", "max_radius / n_ring = 4"]), (dict(max_radius=float("inf")), ["max_radius = inf"]),
                        (dict(z_step=0.0), ["z_step = 0"]), (dict(z_min=float("nan")), ["z_min = nan"]), (dict(capacity=0), ["capacity = 0"]),
                        (dict(capacity=(1 << 20) + 1), [str((1 << 20) + 1), str(1 << 20)]), (dict(max_points_per_scan=0), ["max_points_per_scan = 0"]),
                        (dict(max_points_per_scan=(1 << 24) + 1), [str((1 << 24) + 1), str(1 << 24)])):
        h = C.c_void_p()
        assert L.ptl_place_create(0, C.byref(core.place_cfg(**over)), C.byref(h)) == PTL_ERR_ARG, over
        assert all(w in L.ptl_last_error().decode() for w in words), (over, L.ptl_last_error().decode())
    assert L.ptl_place_create(-1, C.byref(core.place_cfg()), C.byref(h)) == PTL_ERR_ARG and "device_id = -1" in L.ptl_last_error().decode()
    with pytest.raises(ValueError, match="no field"):
        core.place_cfg(rings=3)
    for fn, args in ((L.ptl_place_clear, (None,)), (L.ptl_place_size, (None, None)), (L.ptl_place_tables, (None, None, None)),
                     (L.ptl_place_match, (None, 0, 0, 0, None, None, None)), (L.ptl_place_match_all, (None, 0, 0, 0, None, None, None, None)),
                     (L.ptl_place_read, (None, 0, 0, None, None)), (L.ptl_place_load, (None, 0, None, None)),
                     (L.ptl_place_describe_xyz, (None, None, 0, 0, None, 0, None, None)),
                     (L.ptl_place_describe_range, (None, None, None, None, 0, None, None))):
        assert fn(*args) == PTL_ERR_ARG and "null argument" in L.ptl_last_error().decode()
    assert L.ptl_place_destroy(None) == 0


# ---------------------------------------------------------------------------------------------- 3. host policy on hand-made integers
def test_loop_candidates_policy():
    entry = np.array([-1, -1, 0, 1, 0, 2], dtype=np.int32)
    dist = np.array([0, 0, 300, 100, 100, 50], dtype=np.uint32)
    shift = np.array([0, 0, 3, 59, 0, 7], dtype=np.int32)
    n_cells = [10, 10, 20, 0, 40, 0]
    # cell_dist: pair (2, 0) 300 / 30 = 10; (3, 1) 100 / 10 = 10; (4, 0) 100 / 50 = 2; (5, 2) 50 / 20 = 2.5
    got = fly.loop_candidates(entry, dist, shift, n_cells, 10.0, 8)
    assert got == [(4, 0, 0, 100, 2.0), (5, 2, 7, 50, 2.5), (2, 0, 3, 300, 10.0), (3, 1, 59, 100, 10.0)]
    assert fly.loop_candidates(entry, dist, shift, n_cells, 9.99, 8) == got[:2] and fly.loop_candidates(entry, dist, shift, n_cells, 10.0, 1) == got[:1]
    assert fly.loop_candidates(entry, dist, shift, n_cells, 10.0, 0) == []
    # a pair without any non-zero cell never qualifies; `first` offsets the queries
    assert fly.loop_candidates([0], [0], [0], [0, 0], 100.0, 4, first=1) == []
    assert fly.loop_candidates([0], [8], [2], [1, 3], 100.0, 4, first=1) == [(1, 0, 2, 8, 2.0)]


def test_loop_from_measures_the_odometry_against_the_registration():
    pose_j, pose_i = np.eye(4), np.eye(4)
    pose_j[:3, 3], pose_i[:3, 3] = [1.0, 2.0, 0.0], [1.5, 2.0, 0.0]           # the odometry: i is 0.5 m ahead of j
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = pc.rot_z(2.0), [0.25, 0.0, 0.0]                       # the registration: 0.25 m ahead, turned by 2 degrees
    l = fly.loop_from(7, 2, 5, 120, 1.5, 0.75, T, pose_i, pose_j, 0.5)
    assert (l.i, l.j, l.shift, l.dist, l.cell_dist, l.fraction, l.accepted) == (7, 2, 5, 120, 1.5, 0.75, True)
    assert np.allclose(l.T_ji_odometry[:3, 3], [0.5, 0.0, 0.0]) and abs(l.dt_m - 0.25) < 1e-12 and abs(l.drot_deg - 2.0) < 1e-9
    assert not fly.loop_from(7, 2, 5, 120, 1.5, 0.49, T, pose_i, pose_j, 0.5).accepted
    lines = fly.loop_lines([l, fly.loop_from(8, 3, 0, 9, 0.1, 0.2, T, pose_i, pose_j, 0.5)])
    assert lines[0].startswith("loops: 1 accepted of 2 verified") and "untuned" in lines[0] and "keyframe 7 revisits 2" in lines[1] and len(lines) == 2


def test_place_candidates_policy():
    poses = np.tile(np.eye(4), (5, 1, 1))
    poses[:, 0, 3] = np.arange(5.0)
    dist, shift = np.array([30, 10, 10, 40, 5]), np.array([0, 15, 30, 45, 59])
    got, entries = fly.place_candidates(dist, shift, poses, 60, 3)
    assert list(entries) == [4, 1, 2], "smallest distance first, ties to the smaller index"
    for p, c in zip(got, entries):
        assert np.allclose(p, poses[c] @ core.place_shift_pose(int(shift[c]), 60), atol=0.0)
    assert np.allclose(got[1][:3, :3], pc.rot_z(-90.0), atol=1e-15) and got[1][0, 3] == 1.0
    assert len(fly.place_candidates(dist, shift, poses, 60, 9)[0]) == 5
    with pytest.raises(ValueError, match="place_top = 0"):
        fly.place_candidates(dist, shift, poses, 60, 0)
    with pytest.raises(ValueError, match="5 matched entries from 1 on, 5 poses"):
        fly.place_candidates(dist, shift, poses, 60, 2, first=1)


def test_loop_finder_refusals_need_no_device():
    for kw, word in ((dict(spacing=-1.0), "spacing = -1"), (dict(query_voxel=0.0), "query_voxel = 0"), (dict(map_voxel=-2.0), "map_voxel = -2")):
        with pytest.raises(ValueError, match=word):
            fly.LoopFinder(index=object(), **kw)


# ---------------------------------------------------------------------------------------------- 4. the places file
class _FakeIndex:
    """what save_places / load_places ask of an index: .cfg, .tables(), .descriptors(), .load()"""

    def __init__(self, R=3, S=8, n=4, **over):
        self.cfg = SimpleNamespace(**dict(pn.DEFAULTS, n_ring=R, n_sector=S, **over))
        self.e, self.d = pn.tables(R, S, self.cfg.min_radius, self.cfg.max_radius)
        self.desc = pc.random_descriptors(6, n, R, S)
        self.infos = pn.infos_of(self.desc)

    def tables(self):
        return self.e, self.d

    def descriptors(self):
        return self.desc, self.infos

    def load(self, desc, infos):
        self.desc, self.infos = np.concatenate([self.desc, desc]), np.concatenate([self.infos, infos])


def test_places_file_round_trip_and_refusals(tmp_path):
    src = _FakeIndex()
    poses = np.tile(np.eye(4), (4, 1, 1))
    poses[:, :3, 3] = np.random.default_rng(0).normal(size=(4, 3))
    stamps = [1626432000.0 + 0.1 * k for k in range(4)]
    path = str(tmp_path / "places.npz")
    pu.save_places(path, src, poses, stamps)
    assert os.path.isfile(path)
    back = pu.load_places(path)
    assert back["cfg"] == dict(pn.DEFAULTS, n_ring=3, n_sector=8) and isinstance(back["cfg"]["n_ring"], int)
    assert np.array_equal(back["desc"], src.desc) and back["desc"].dtype == np.uint8 and np.array_equal(back["infos"], src.infos)
    assert np.array_equal(back["poses"], poses) and np.array_equal(back["stamps"], np.array(stamps))
    assert np.array_equal(back["ring_edge2"], src.e) and np.array_equal(back["sector_dir"], src.d)
    dst = _FakeIndex(n=0)
    pu.load_places(path, dst)
    assert np.array_equal(dst.desc, src.desc) and np.array_equal(dst.infos, src.infos)
    # refusals: counts, another cfg, another table, another kind of file
    with pytest.raises(ValueError, match="4 entries with 3 poses and 4 stamps"):
        pu.save_places(path + ".x", src, poses[:3], stamps)
    other = _FakeIndex(n=0, z_step=0.125)
    with pytest.raises(ValueError, match="z_step = 0.0625 in the file, 0.125 in the handle"):
        pu.load_places(path, other)
    assert len(other.desc) == 0
    bent = _FakeIndex(n=0)
    bent.d = bent.d.copy()
    bent.d[3, 1] = np.nextafter(bent.d[3, 1], 1.0)
    with pytest.raises(ValueError, match="the table sector_dir differs"):
        pu.load_places(path, bent)
    assert len(bent.desc) == 0
    np.savez(str(tmp_path / "other.npz"), free=np.zeros(3))
    with pytest.raises(ValueError, match="not a places file"):
        pu.load_places(str(tmp_path / "other.npz"))


# ---------------------------------------------------------------------------------------------- 5. the commands' refusals
def test_commands_refuse_options_before_any_device_is_touched(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    r = run(ptudes_cli, ["ekf-bench", "ouster", "--help"])
    assert r.exit_code == 0
    for opt in ("--find-loops", "--loop-spacing", "--loop-min-gap", "--loop-max-cell-dist", "--loop-min-fraction", "--save-loops", "--save-places"):
        assert opt in r.output, opt
    assert "untuned" in r.output
    base = ["ekf-bench", "ouster", "--synthetic", "1000", "--find-loops"]
    for args, words in ((["ekf-bench", "ouster", "--synthetic", "1", "--loop-min-gap", "3"], ["--loop-min-gap belongs to --find-loops"]),
                        (["ekf-bench", "ouster", "--synthetic", "1", "--save-loops", "a.csv"], ["--save-loops belongs to --find-loops"]),
                        (["ekf-bench", "ouster", "--synthetic", "1", "--loop-spacing", "3"], ["--loop-spacing belongs to"]),
                        (base + ["--loop-spacing", "-1"], ["--loop-spacing -1"]), (base + ["--loop-min-gap", "-2"], ["--loop-min-gap -2"]),
                        (base + ["--loop-max-cell-dist", "-0.5"], ["--loop-max-cell-dist -0.5"]),
                        (base + ["--loop-min-fraction", "1.5"], ["--loop-min-fraction 1.5", "[0, 1]"]),
                        (base + ["--save-loops", "loops.txt"], ["--save-loops loops.txt", ".csv"]),
                        (base + ["--save-places", "places.bin"], ["--save-places places.bin", ".npz"])):
        r = run(ptudes_cli, args)
        assert r.exit_code != 0 and all(w in r.output for w in words), (args, r.output)
    r = run(ptudes_cli, ["localize", "--help"])
    assert r.exit_code == 0 and "--places" in r.output and "--place-top" in r.output
    m, k, p = tmp_path / "map.npy", tmp_path / "kf.csv", tmp_path / "places.npz"
    np.save(str(m), np.zeros((3, 3)))
    k.write_text("")
    np.savez(str(p), free=np.zeros(3))
    loc = ["localize", "--synthetic", "1000", "--map", str(m)]
    for args, words in ((loc + ["--places", str(p), "--keyframes", str(k)], ["--keyframes does not go with --places"]),
                        (loc + ["--places", str(p), "--yaws", "8"], ["--yaws does not go with --places"]),
                        (loc + ["--places", str(tmp_path / "no.npz")], ["--places", "no such file"]),
                        (loc + ["--places", str(k)], [".npz"]), (loc + ["--places", str(p), "--place-top", "0"], ["--place-top 0"]),
                        (loc + ["--keyframes", str(k), "--place-top", "2"], ["--place-top belongs to --places"]),
                        (loc + ["--places", str(p)], ["not a places file"])):
        r = run(ptudes_cli, args)
        assert r.exit_code != 0 and all(w in r.output for w in words), (args, r.output)
