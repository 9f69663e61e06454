"""The voxel hash tables under collisions, the cyclic wrap, tombstones, real exhaustion and rebuilds: every open-addressing
loop that consumes brick_slot() - the claims of both per-scan down-sampling tables, map_find behind the 32-lane search and the map score, the
8-lane search's probe rounds, the map insert, the prune's tombstones, the rebuild - on tables of 2^10 / 2^12 slots filled with the scenes of
tests/helpers/hash_scenes.py, where probing past the home slot is the rule.  tests/test_hash_scenes_cpu.py shows without a GPU that the
scenes collide, wrap and hide voxels behind tombstones in numbers.

References: the CPU oracle for every result (map content bit for bit, correspondences, poses, statistics), and the table simulator of
hash_scenes.py for the table itself, read back with ptl_icp_debug_table: the set of occupied slots of a linear-probing table without reuse
does not depend on the order of insertion, so it must equal the simulator's exactly - which pins the Python restatement of the hash (a wrong
one would only make the scenes collide less) and proves that the collisions happened on the device.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from oracle import cpu as orc
from ptudes_lab_amd import _lib as L
from ptudes_lab_amd import core
from tests.helpers import hash_drive as hd
from tests.helpers import hash_scenes as hs
from tests.helpers import lattice_scenes as ls

pytestmark = pytest.mark.gpu

CAP = 1 << 12
CAPS = dict(voxel_size=1.0, map_table_capacity=CAP, map_block_capacity=1 << 12)
ICP_T_TOL, ICP_R_TOL = 2e-4, 2e-5  # tests/test_gpu_parity.py
POSE_TOL = 1e-9                     # tests/test_gpu_search_edges.py
FORMS = {  # tests/test_gpu_search_edges.py PER_CALL_FORMS
    "sparse32": dict(),
    "lanes8_gc32": dict(gn_lanes_per_point=8, gn_threads=512, gn_workgroups=32),
}
ENTRY = np.dtype([("key", "<u8"), ("blk", "<i4"), ("head", "<i4")])
ERR_TABLE = 4


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def _pose_diff(A, B):
    D = np.linalg.inv(A) @ B
    return np.linalg.norm(D[:3, 3]), orc.rot_angle(D)


# ------------------------------------------------------------------------------------------------ the dump and its invariants
def _dump(h):
    """ptl_icp_debug_table of an ICP handle (a core.Icp or a raw pointer) as a dict"""
    h = getattr(h, "_h", h)
    info = (C.c_int64 * 8)()
    L.check(L.lib().ptl_icp_debug_table(h, None, 0, None, None, 0, info))
    slots, blocks = info[3] + 1, info[6]
    ent, bhdr, bfirst = np.empty(slots, dtype=ENTRY), np.empty((blocks, 4), dtype=np.int32), np.empty((blocks, 3))
    L.check(L.lib().ptl_icp_debug_table(h, ent.ctypes.data_as(C.c_void_p), slots, bhdr.ctypes.data_as(C.POINTER(C.c_int32)), L.dptr(bfirst),
                                        blocks, info))
    return dict(ent=ent, bhdr=bhdr, bfirst=bfirst, tab_used=info[0], n_live=info[1], err_flags=info[2], tmask=info[3], vmask=info[4],
                vmask2=info[5], n_small=info[7])


def _check_table(d, what, vs=1.0):
    """live table entries and live directory blocks are in bijection, and every key can be found: returns the live keys"""
    key = d["ent"]["key"]
    live = np.flatnonzero((key != hs.EMPTY_KEY) & (key != hs.TOMB_KEY))
    blocks = np.flatnonzero(d["bhdr"][:, 0] > 0)
    assert len(live) == len(blocks) == d["n_live"], (what, len(live), len(blocks), d["n_live"])
    slot, count = d["bhdr"][blocks, 1], d["bhdr"][blocks, 0]
    assert np.array_equal(np.sort(slot), live), what
    assert np.array_equal(key[slot], hs.pack_key(hs.voxel_of(d["bfirst"][blocks], vs))), what  # the entry's key is the key of the block's first point
    assert np.array_equal(d["ent"]["blk"][slot], blocks | count << 24), what
    assert (d["ent"]["blk"][key == hs.TOMB_KEY] == -1).all() and (d["ent"]["head"][live] == -1).all(), what
    assert len(np.unique(key[live])) == len(live), what
    # no EMPTY slot lies cyclically between a key's home and its slot
    home = hs.brick_slot(key[live], d["tmask"])
    empty = np.concatenate([[0], np.cumsum(key == hs.EMPTY_KEY)])
    between = np.where(live >= home, empty[live] - empty[home], empty[-1] - empty[home] + empty[live])
    assert (between == 0).all(), (what, int((between != 0).sum()))
    return key[live]


def _check_against_sim(d, sim, what, n_max):
    live = _check_table(d, what, sim.vs)
    key = d["ent"]["key"]
    assert np.array_equal(np.flatnonzero(key != hs.EMPTY_KEY), sim.tab.occupied()), what
    assert int((key == hs.TOMB_KEY).sum()) == sim.tab.tombstones(), what
    assert (d["tab_used"], d["n_live"]) == (sim.tab.used, sim.n_live), (what, d["tab_used"], d["n_live"], sim.tab.used, sim.n_live)
    assert set(live.tolist()) == set(sim.first), what
    assert (d["tmask"], d["vmask"], d["vmask2"]) == (sim.tab.cap - 1, hs.vds_table_slots(hs.VDS1_SLOTS_PER_POINT, n_max) - 1,
                                                     hs.vds_table_slots(hs.VDS2_SLOTS_PER_POINT, n_max) - 1), what


def _same_map(icp, size, points, what):
    assert icp.map_size() == size, (what, icp.map_size(), size)
    assert np.array_equal(_sorted_rows(icp.map_points()), points), what  # bit for bit


def _check_score(icp):
    """map_score(per_point=True) against tests/helpers/map_score_numpy.py, by the check and the bounds of tests/test_gpu_map_score.py"""
    from tests.helpers import map_score_check
    map_score_check.check(icp, 20)


# ------------------------------------------------------------------------------------------------ A. the map stage, teacher-forced
N_MAX = 4096


def _query_clouds(sc):
    """the tie grid of lattice_scenes (its part within one voxel size of the centre) around colliding voxels - pruned ones, survivors, wrapped
    ones - and the centres of voxels that never exist and home on the full lines: an unsuccessful probe is the longest walk"""
    grid = ls.tie_queries()[1]
    grid = grid[(np.abs(grid) <= 1.0).all(axis=1)]
    col, far = sc["colliding"], sc["far"]
    a = np.concatenate([grid + v for v in np.concatenate([col[far][[1, -1]], col[~far][[0, -1]]])])
    b = np.concatenate([grid + v for v in col[~far][[60, 90]]] + [hs.points_in(sc["absent"], 0.5), grid[::3] + sc["absent"][5]])
    assert len(a) <= N_MAX and len(b) <= N_MAX
    return a, b


@functools.lru_cache(maxsize=None)
def _oracle_map_stage():
    """the oracle's and the simulator's side of the steps, once: per step what the device must show"""
    sc = hs.map_stage_scene(CAP)
    ref = orc.ICP(sc["max_range"], 0.0, voxel_size=1.0)
    m, sim = ref.map, hs.MapSim(CAP, 1.0, sc["max_range"])
    queries, M = _query_clouds(sc), 0.5
    small = orc.se3_exp(np.array([0.03, -0.02, 0.01, 0.002, -0.001, 0.003]))
    out = []

    def record(what):
        pts = _sorted_rows(m.points())
        src = pts[::7][:N_MAX]
        src = (src - small[:3, 3]) @ small[:3, :3]  # the map's own points seen from a pose a little off: align brings them back
        lin = [m.linear_system(q, M, M / 9.0) for q in queries]
        assert what != "insert" or all(r[1] > 100 for r in lin)
        out.append(dict(what=what, size=(m.num_voxels, m.num_points), points=pts, lin=lin, src=src, reg=m.register(src, np.eye(4), 6.0, 2 / 3)[:2],
                        table=(sim.tab.keys.copy(), sim.tab.used, dict(sim.first))))

    for b in sc["batches"]:
        m.add_points(b)
        sim.add(b)
    record("insert")
    m.prune(sc["origin"])
    sim.prune(sc["origin"])
    record("prune")
    m.add_points(sc["reinsert"])
    sim.add(sc["reinsert"])
    record("reinsert")
    # a registered scan on the collided table (the search of the handle's own Gauss-Newton kernel), its map update and - rebuild_every = 1 - a
    # rebuild; then one more prune from elsewhere: it goes by the table slots the rebuild left in the directory
    # (its points: stored ones moved by 1/64 m, none within two voxels of a query - there the registered copies, 1e-13 m from the originals on
    # either side, would turn the exact ties of the queries into choices that rounding makes)
    qv = np.unique(hs.voxel_of(np.concatenate(queries), 1.0), axis=0)
    scan = out[-1]["points"][::4]
    near = np.zeros(len(scan), dtype=bool)
    for v in qv:
        near |= (np.abs(hs.voxel_of(scan, 1.0) - v) <= 2).all(axis=1)
    scan = (scan[~near][:N_MAX] + np.array([0.015625, 0.0, -0.015625])).astype(np.float32)
    pose = ref.register_frame(scan.astype(np.float64), np.zeros(len(scan)))
    sim.add(ref.last_frame_down() @ pose[:3, :3].T + pose[:3, 3])
    sim.prune(pose[:3, 3])
    sim.rebuild()
    reg = dict(scan=scan, pose=pose, stats=ref.stats[-1], fd=ref.last_frame_down(), src=ref.last_source())
    record("register + rebuild")
    origin2 = sc["origin"] + np.array([-48.0, 32.0, 16.0])
    m.prune(origin2)
    sim.prune(origin2)
    record("prune after rebuild")
    return sc, queries, M, out, reg, origin2, ref  # (ref owns the map the records were made of)


def _restore(rec, sc):
    sim = hs.MapSim(CAP, 1.0, sc["max_range"])
    sim.tab.keys, sim.tab.used, sim.first = rec["table"][0].copy(), rec["table"][1], dict(rec["table"][2])
    return sim


def _check_step(icp, rec, sc, queries, M, exact=True):
    what = rec["what"]
    if exact:
        _same_map(icp, rec["size"], rec["points"], what)
    else:  # points that entered under a registered pose: the same number, each within POSE_TOL of the oracle's (test_gpu_search_edges._check_maps)
        assert icp.map_size() == rec["size"], (what, icp.map_size(), rec["size"])
        a, b = icp.map_points(), rec["points"]
        a, b = a[np.lexsort(np.round(a, 6).T[::-1])], b[np.lexsort(np.round(b, 6).T[::-1])]
        assert np.abs(a - b).max() <= POSE_TOL, (what, np.abs(a - b).max())
    for q, (s_ref, nc_ref, cand_ref) in zip(queries, rec["lin"]):
        s_gpu, nc, cand = icp.linear_system(q, M, M / 9.0)
        assert (nc, cand) == (nc_ref, cand_ref), (what, nc, cand, nc_ref, cand_ref)
        assert np.abs(s_gpu - s_ref).max() <= 1e-9 * np.abs(s_ref).max(), what
    out, it = icp.align(rec["src"], np.eye(4), 6.0, 2 / 3)
    dt, dr = _pose_diff(rec["reg"][0], out)
    assert dt <= ICP_T_TOL and dr <= ICP_R_TOL and abs(it - rec["reg"][1]) <= 1, (what, dt, dr, it, rec["reg"][1])
    _check_score(icp)
    _check_against_sim(_dump(icp), _restore(rec, sc), what, N_MAX)


@pytest.mark.parametrize("form", list(FORMS))
def test_map_stage_on_a_collided_table(form):
    """insert in three ragged calls (long chains, a chain that wraps, a 55 % full table), prune (tombstones in front of survivors), insert into
    pruned voxels and survivors, register a scan and rebuild, prune again: after every step the oracle's map, correspondences, alignment and
    map score, and the simulator's table"""
    sc, queries, M, recs, reg, origin2, _ = _oracle_map_stage()
    icp = core.Icp(sc["max_range"], 0.0, max_points_per_scan=N_MAX, rebuild_every=1, **CAPS, **FORMS[form])
    for b in sc["batches"]:
        icp.map_add(b)
    _check_step(icp, recs[0], sc, queries, M)
    icp.map_add(np.zeros((0, 3)), origin=sc["origin"])
    _check_step(icp, recs[1], sc, queries, M)
    icp.map_add(sc["reinsert"])
    _check_step(icp, recs[2], sc, queries, M)
    pose = icp.register_frame(reg["scan"], np.zeros(len(reg["scan"])))
    st = icp.stats[-1]
    for key in ("n_in", "n_valid", "n_down", "n_src", "map_voxels", "map_points"):
        assert st[key] == reg["stats"][key], (key, st[key], reg["stats"][key])
    # the scan is the map moved by 1/64 m: a first step of 0.022 m, a second of rounding size - the iteration count hangs on no rounding, and
    # with it the pairs of the last iteration and the candidates every search of the run met are the oracle's numbers
    assert reg["stats"]["iterations"] == 2 and reg["stats"]["n_src"] > 500
    for key in ("iterations", "n_corr_last", "sum_cand"):
        assert st[key] == reg["stats"][key], (key, st[key], reg["stats"][key])
    assert np.array_equal(icp.last_frame_down(), reg["fd"]) and np.array_equal(icp.last_source(), reg["src"])
    dt, dr = _pose_diff(reg["pose"], pose)
    print(f"{form}: registered pose off the oracle's by {dt:.3e} m, {dr:.3e} rad")
    assert dt <= ICP_T_TOL and dr <= ICP_R_TOL, (dt, dr)
    _check_step(icp, recs[3], sc, queries, M, exact=False)
    icp.map_add(np.zeros((0, 3)), origin=origin2)
    _check_step(icp, recs[4], sc, queries, M, exact=False)
    assert recs[4]["size"][0] < recs[3]["size"][0] - 100
    icp.close()


# ------------------------------------------------------------------------------------------------ B. exhaustion for real
def test_a_table_that_fills_with_tombstones_is_refused_at_three_quarters():
    """rebuild_every = 0, fresh voxels in and old ones out call after call: every call before the one at which the simulator's `used` passes
    3/4 of the table gives the oracle's map, that call returns PTL_ERR_CAPACITY with the table flag, and `used` - tombstones included - is
    the simulator's"""
    cap = 1 << 10
    steps, max_range = hs.exhaustion_steps()
    icp = core.Icp(max_range, 0.0, voxel_size=1.0, map_table_capacity=cap, map_block_capacity=1 << 12, max_points_per_scan=N_MAX, rebuild_every=0)
    m, sim = orc.Map(1.0, max_range, 20), hs.MapSim(cap, 1.0, max_range)
    refused = None
    for i, (p, o) in enumerate(steps):
        m.add_points(p)
        m.prune(o)
        sim.add(p)
        sim.prune(o)
        if sim.tab.exhausted:
            with pytest.raises(RuntimeError, match=r"error -3: .*flags 0x4 "):
                icp.map_add(p, origin=o)
            refused = i
            break
        icp.map_add(p, origin=o)
        _same_map(icp, (m.num_voxels, m.num_points), _sorted_rows(m.points()), i)
        _check_against_sim(_dump(icp), sim, i, N_MAX)
    assert refused is not None and refused >= 4
    d = _dump(icp)
    assert d["err_flags"] == ERR_TABLE and d["tab_used"] == sim.tab.used > cap // 4 * 3 > 3 * d["n_live"]
    assert np.array_equal(np.flatnonzero(d["ent"]["key"] != hs.EMPTY_KEY), sim.tab.occupied())  # (the call itself went through: the table is not full)
    icp.close()


# ------------------------------------------------------------------------------------------------ D. the per-scan tables
VDS_N = 2048
VDS_SHIFT = np.array([0.0625, 0.0, -0.0625])  # every point stays in its voxel of either pass (tests/test_hash_scenes_cpu.py)


@functools.lru_cache(maxsize=None)
def _vds_reference(which):
    """the two scans and the oracle's run of them"""
    pts = hs.vds_scene(VDS_N, which)[0]
    scans = [pts, pts + VDS_SHIFT]
    ref = orc.ICP(1000.0, 0.0, voxel_size=1.0)
    rows = []
    for x in scans:
        pose = ref.register_frame(x, np.zeros(len(x)))
        fd = orc.voxel_downsample(x, 0.5)
        src = orc.voxel_downsample(fd, 1.5)
        assert np.array_equal(fd, ref.last_frame_down()) and np.array_equal(src, ref.last_source())
        rows.append(dict(pose=pose, stats=ref.stats[-1], fd=fd, src=src))
    assert rows[0]["stats"]["n_src"] < rows[0]["stats"]["n_down"] < len(pts) and not np.array_equal(rows[0]["fd"], rows[1]["fd"])
    return scans, rows


def _padded(x, n=VDS_N):
    out = np.zeros((n, 3), dtype=np.float32)
    out[: len(x)] = x
    assert np.array_equal(out[: len(x)].astype(np.float64), x)
    return out


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("which", (1, 2))
def test_downsample_tables_with_chains_that_wrap(which, dtype):
    """scans whose voxels of pass `which` home on the last two lines of its table: both selections bit-equal to the oracle's, twice - the second
    scan finds the table as the first one's compaction left it, so a claimed slot of a long chain that was not released would show"""
    scans, rows = _vds_reference(which)
    icp = core.Icp(1000.0, 0.0, max_points_per_scan=VDS_N, **CAPS)
    for k, (x, row) in enumerate(zip(scans, rows)):
        pose = icp.register_frame(x.astype(dtype), None if dtype == np.float32 else np.zeros(len(x)))
        for key in ("n_in", "n_valid", "n_down", "n_src", "map_voxels", "map_points"):
            assert icp.stats[-1][key] == row["stats"][key], (k, key, icp.stats[-1][key], row["stats"][key])
        assert np.array_equal(icp.last_frame_down(), row["fd"]), k
        assert np.array_equal(icp.last_source(), row["src"]), k
        dt, dr = _pose_diff(row["pose"], pose)
        assert dt <= ICP_T_TOL and dr <= ICP_R_TOL and abs(icp.stats[-1]["iterations"] - row["stats"]["iterations"]) <= 1, (k, dt, dr)
    d = _dump(icp)
    _check_table(d, which)
    assert d["vmask"] + 1 == hs.vds_scene(VDS_N, 1)[3] and d["vmask2"] + 1 == hs.vds_scene(VDS_N, 2)[3]
    icp.close()


@pytest.mark.parametrize("which", (1, 2))
def test_downsample_tables_in_the_resident_drivers(which):
    """the same two scans as scans 0 and 1 of a SeqRunner and of one member of a free-running batch (its down-sampling stages are another
    instance): the counts and poses of the per-call run with the same Gauss-Newton geometry, and the oracle's counts"""
    scans, rows = _vds_reference(which)
    frames = [_padded(x) for x in scans]
    geom = dict(gn_lanes_per_point=8, gn_threads=512, max_points_per_scan=VDS_N)  # (a runner's tables are sized by this field too)
    b = core.BatchRunner(2, 2, VDS_N, 0, max_range=1000.0, min_range=0.0, with_ekf=False, max_points_per_scan=VDS_N, **CAPS)
    assert b.free_running
    team = b.team_geometry()[0]
    for s in range(2):
        for k in range(2):
            b.upload_scan(s, k, frames[(k + s) % 2])  # member 1 sees the scans in the other order
        b.upload_imu(s, np.zeros((0, 7)), [0, 0])
    b.run()
    per_call = core.Icp(1000.0, 0.0, gn_workgroups=team, **geom, **CAPS)
    want = [per_call.register_frame(f, None) for f in frames]
    r = core.SeqRunner(2, VDS_N, 0, max_range=1000.0, min_range=0.0, with_ekf=False, gn_workgroups=team, **geom, **CAPS)
    for k in range(2):
        r.upload_scan(k, frames[k])
    r.upload_imu(np.zeros((0, 7)), [0, 0])
    r.run()
    for what, out in (("seq", r.results()), ("batch", b.results(0))):
        for k in range(2):
            for key in ("n_valid", "n_down", "n_src"):
                assert out["stats"][k][key] == per_call.stats[k][key] == rows[k]["stats"][key], (what, k, key)
            assert out["stats"][k] == per_call.stats[k], (what, k, out["stats"][k], per_call.stats[k])
            assert np.array_equal(out["kiss_poses"][k], want[k]), (what, k, np.abs(out["kiss_poses"][k] - want[k]).max())
    other = b.results(1)["stats"]
    assert [other[k]["n_down"] for k in range(2)] == [rows[1 - k]["stats"]["n_down"] for k in range(2)]
    h = C.c_void_p()
    L.check(L.lib().ptl_batch_icp(b._h, 0, C.byref(h)))
    d = _dump(h)
    _check_table(d, ("batch", which))
    assert d["vmask"] + 1 == hs.vds_scene(VDS_N, 1)[3] and d["vmask2"] + 1 == hs.vds_scene(VDS_N, 2)[3]
    L.check(L.lib().ptl_seq_icp(r._h, C.byref(h)))
    d = _dump(h)
    _check_table(d, ("seq", which))
    assert d["vmask"] + 1 == hs.vds_scene(VDS_N, 1)[3] and d["vmask2"] + 1 == hs.vds_scene(VDS_N, 2)[3]
    for x in (per_call, r, b):
        x.close()


# ------------------------------------------------------------------------------------------------ C. rebuilds on a table that is needed
DRIVE_N, DRIVE_RANGE, DRIVE_MIN, DRIVE_PTS, REBUILD_EVERY = hd.DRIVE_N, hd.DRIVE_RANGE, hd.DRIVE_MIN, hd.DRIVE_PTS, hd.REBUILD_EVERY
_drive_reference = hd.drive_reference  # (cached: the oracle's run of the drive and the simulator's answers, tests/helpers/hash_drive.py)
INT_STATS = ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points")  # tests/test_gpu_batch.py
DRIVERS = ("per_call", "seq", "free8", "free4", "free_two_block_classes", "lockstep")


def _run_drive(driver, cap, rebuild_every, n=DRIVE_N, then=0):
    """the first n scans (and, separately enqueued, `then` more) of the drive through `driver` on a cap-slot table: (poses, stats, table dump)"""
    frames = _drive_reference()["frames"]
    over = dict(voxel_size=1.0, deskew=0, rebuild_every=rebuild_every, map_table_capacity=cap, map_block_capacity=1 << 12, max_points_per_scan=DRIVE_PTS)
    if driver == "per_call":
        icp = core.Icp(DRIVE_RANGE, DRIVE_MIN, **over)
        try:
            poses = [icp.register_frame(f, None) for f in frames[:n + then]]
            return np.array(poses), icp.stats, _dump(icp)
        finally:
            icp.close()
    kw = dict(max_range=DRIVE_RANGE, min_range=DRIVE_MIN, with_ekf=False, **over)
    if driver == "seq":
        r = core.SeqRunner(DRIVE_N, DRIVE_PTS, 0, gn_workgroups=32, gn_lanes_per_point=8, gn_threads=512, **kw)
        upload, imu, icp_of = r.upload_scan, r.upload_imu, lambda h: L.lib().ptl_seq_icp(r._h, C.byref(h))
    else:
        if driver == "lockstep":
            kw.update(gn_lanes_per_point=32, gn_threads=1024, free_running=False)
        if driver == "free_two_block_classes":
            kw.update(map_small_blocks=1 << 12)
        r = core.BatchRunner(1, DRIVE_N, DRIVE_PTS, 0, **kw)
        assert r.free_running == (driver != "lockstep")
        if driver in ("free8", "free4"):
            assert r.debug_map_points_per_thread(int(driver[-1])) == int(driver[-1])
        upload, imu, icp_of = functools.partial(r.upload_scan, 0), functools.partial(r.upload_imu, 0), lambda h: L.lib().ptl_batch_icp(r._h, 0, C.byref(h))
    try:
        for k, f in enumerate(frames):
            upload(k, f)
        imu(np.zeros((0, 7)), [0] * DRIVE_N)
        r.run(n)
        if then:
            r.enqueue(then)
            r.wait()
        out = r.results() if driver == "seq" else r.results(0)
        h = C.c_void_p()
        L.check(icp_of(h))
        return out["kiss_poses"], out["stats"], _dump(h)
    finally:
        r.close()


@pytest.mark.parametrize("driver", DRIVERS)
def test_rebuilds_on_a_table_at_half_load(driver):
    """a drive that leaves its map behind, a rebuild every 3 scans, on the smallest table that never passes 3/4 (peak load above 1/2):
    the oracle's integer statistics on every scan and its poses to 1e-9, the same bits as on a 2^22-slot table - the size of the table must
    not be observable - and after the last scan a table that holds the directory's voxels, with the simulator's tombstones since the last
    rebuild"""
    ref = _drive_reference()
    poses, stats, d = _run_drive(driver, ref["cap"], REBUILD_EVERY)
    assert len(poses) == len(stats) == DRIVE_N
    for k in range(DRIVE_N):
        for key in INT_STATS:
            assert stats[k][key] == ref["stats"][k][key], (driver, k, key, stats[k][key], ref["stats"][k][key])
    dev = np.abs(poses - ref["poses"]).max()
    print(f"{driver}: poses within {dev:.3e} of the oracle's, table of {ref['cap']} slots")
    assert dev < POSE_TOL, dev
    big_poses, big_stats, big = _run_drive(driver, 1 << 22, REBUILD_EVERY)
    assert np.array_equal(poses, big_poses) and list(stats) == list(big_stats), driver
    assert (big["tab_used"], big["n_live"]) == (d["tab_used"], d["n_live"])
    _check_table(big, (driver, "2^22"))
    _check_against_sim(d, ref["sim"], driver, DRIVE_PTS)
    assert d["err_flags"] == 0 and (d["ent"]["key"] == hs.TOMB_KEY).sum() > 100


@pytest.mark.parametrize("driver", DRIVERS)
def test_without_rebuilds_the_same_drive_fills_the_table(driver):
    """rebuild_every = 0 on the same table: the scans before the one at which the simulator's `used` passes 3/4 go through, that one reports
    the table flag"""
    ref = _drive_reference()
    k = ref["refused"]
    poses, stats, d = _run_drive(driver, ref["cap"], 0, n=k)
    assert len(poses) == k and d["err_flags"] == 0 and d["tab_used"] <= ref["cap"] // 4 * 3
    for i in range(k):
        assert all(stats[i][key] == ref["stats"][i][key] for key in INT_STATS), (driver, i)
    with pytest.raises(RuntimeError, match=r"error -3: .*0x4"):
        _run_drive(driver, ref["cap"], 0, n=k, then=1)
