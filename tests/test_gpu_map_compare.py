"""The map distance on the device (csrc/compare_kernels.h) against its numpy restatement (tests/helpers/map_compare_numpy.py):
brute force over `map_points()` of the reference handle, so that the 27-voxel neighbourhood itself is what is checked.  The per-point values
and every count are compared bit for bit / exactly - a minimum does not depend on the order of its terms.  The sums are compared within

    |device - numpy| <= (n + 2) * eps * sum          n = number of matched queries, eps = 2^-52

Derivation: both sides add n non-negative terms, each in an order of its own (the device: strided partial sums and a tree; numpy: pairwise).
A sum of n non-negative terms in any order is within (n - 1) u of the exact sum, relatively, u = eps / 2 the unit roundoff (every partial sum
is at most the total and each of the n - 1 additions rounds once); two such sums differ by at most 2 (n - 1) u = (n - 1) eps.  The terms
of sum_dist are square roots: the device's and numpy's are each correctly rounded or within one ulp (eps relative) of each other, which adds
eps * sum.  (n - 1 + 1) eps <= (n + 2) eps; sum_dist2's terms are the same bits on both sides.

Per-call `core.Icp` maps with small capacities."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.helpers import map_compare_numpy as mc
from tests.helpers.map_compare_cases import VS, hand_cases

pytestmark = pytest.mark.gpu

CAPS = dict(map_block_capacity=1 << 14, map_table_capacity=1 << 16)
EPS = np.finfo(np.float64).eps
CMP_CHUNK = 1 << 17  # csrc/compare_kernels.h: queries staged at a time
PTL_ERR_ARG, PTL_ERR_CAPACITY = -1, -3


def _icp(voxel, P=20, n_max=1 << 14, **over):
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core
    kw = dict(voxel_size=voxel, max_points_per_voxel=P, max_points_per_scan=n_max, **CAPS)
    kw.update(over)
    return core.Icp(1.0e9, 0.0, **kw)


def _lex(a):
    return np.lexsort(a.T[::-1])


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _check_summary(s, d2, max_dist, thresholds, what=""):
    """a core.MapDistance against the restatement's summary of the per-point values: counts exactly, sums within the bound above"""
    want = mc.summary(d2, max_dist, thresholds)
    assert (s.n_query, s.n_invalid, s.n_matched, s.n_within) == (want["n_query"], want["n_invalid"], want["n_matched"], want["n_within"]), what
    assert s.max_dist2_seen == want["max_dist2_seen"] and s.max_dist == max_dist and s.thresholds == tuple(thresholds)
    n = want["n_matched"]
    for name in ("sum_dist", "sum_dist2"):
        diff, bound = abs(getattr(s, name) - want[name]), (n + 2) * EPS * want[name]
        print(f"{what} {name}: device {getattr(s, name)!r}, numpy {want[name]!r}, |difference| {diff:.3e}, bound {bound:.3e} (n = {n})")
        assert diff <= bound, (what, name, diff, bound)


def _check(icp, queries, max_dist=None, thresholds=None, what=""):
    """map_distance(per_point=True) of `queries` against brute force over the handle's stored points"""
    md = icp.cfg.voxel_size if max_dist is None else max_dist
    thr = (md,) if thresholds is None else tuple(thresholds)
    s, d2 = icp.map_distance(queries, max_dist=max_dist, thresholds=thresholds, per_point=True)
    want = mc.dist2(queries, icp.map_points(), icp.cfg.voxel_size, md)
    bad = np.flatnonzero(~((d2 == want) | (np.isnan(d2) & np.isnan(want))))
    assert len(bad) == 0, (what, len(bad), np.asarray(queries)[bad[:5]], d2[bad[:5]], want[bad[:5]])
    _check_summary(s, d2, md, thr, what)
    # the summary alone is the same summary
    s2 = icp.map_distance(queries, max_dist=max_dist, thresholds=thresholds)
    assert (s2.n_matched, s2.n_within, s2.sum_dist, s2.sum_dist2) == (s.n_matched, s.n_within, s.sum_dist, s.sum_dist2)
    return s, d2


def _grid(lo, hi, step):
    a = np.arange(lo, hi + step / 2, step)
    g = np.meshgrid(a, a, a, indexing="ij")
    return np.stack([x.reshape(-1) for x in g], axis=1)


def _dyadic_queries(rng, n, lo, hi, denom=64):
    return rng.integers(int(lo * denom), int(hi * denom) + 1, (n, 3)) / float(denom)


# 1. the answers computed by hand; the rounding case of score_need; a full voxel
def test_hand_cases_rounding_case_and_a_full_voxel():
    ref, max_dist, cases = hand_cases()
    icp = _icp(VS, P=4)
    icp.map_add(ref)
    assert icp.map_size()[1] == len(ref)
    q = np.array([c[1] for c in cases])
    s, d2 = _check(icp, q, max_dist=max_dist, thresholds=(0.125, 0.25), what="hand cases")
    for (name, _, w), g in zip(cases, d2):
        assert (np.isnan(g) and np.isnan(w)) or g == w, (name, g, w)
    assert (s.n_query, s.n_invalid, s.n_matched, s.n_within) == (len(cases), 2, 4, (1, 4))
    icp.close()

    # 0.5 - 1 ulp and 1.0 at vs = 0.5, max_dist = vs: the difference rounds to 0.5, the pair is matched, and its voxels are 0 and 2 - on every
    # axis, in both directions
    below = np.nextafter(0.5, 0.0)
    assert 1.0 - below == 0.5, "the exact difference 0.5 + 2^-54 rounds to 0.5"
    icp = _icp(0.5, P=4)
    pts, qs = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            c = 0.125 + 8.0 * len(pts)  # (the other two coordinates: the pairs lie far from one another)
            p, qq = np.full(3, c), np.full(3, c)
            p[axis], qq[axis] = sign * 1.0, sign * below
            pts.append(p)
            qs.append(qq)
    pts, qs = np.array(pts), np.array(qs)
    assert (np.abs(np.trunc(pts / 0.5) - np.trunc(qs / 0.5)).max(axis=1) == 2).all(), "the pairs sit two voxels apart"
    icp.map_add(pts)
    s, d2 = _check(icp, qs, what="rounding case")
    assert (d2 == 0.25).all() and s.n_matched == 6
    icp.close()

    # a full voxel: six points arrive in one voxel of four; the distances are to the four that are stored
    icp = _icp(0.5, P=4)
    six = np.array([[0.0625 * (k + 1), 0.25, 0.25] for k in range(6)])
    icp.map_add(six[:4])  # (calls are ordered: the first four are the stored ones)
    icp.map_add(six[4:])
    assert icp.map_size() == (1, 4)
    s, d2 = _check(icp, six, what="full voxel")
    assert (d2[:4] == 0.0).all() and d2[4] == 0.0625 ** 2 and d2[5] == 0.125 ** 2
    icp.close()


# 2. query counts around the half-wave, the wavefront and the staging chunk; an empty reference
def test_query_counts_and_the_empty_reference():
    rng = np.random.default_rng(7)
    icp = _icp(0.5, P=3)  # (27 stored lattice points would fit a voxel: the cap of 3 binds)
    empty_q = _dyadic_queries(rng, 70, -1.5, 1.5)
    empty_q[3, 1] = np.nan
    s, d2 = icp.map_distance(empty_q, per_point=True)
    assert (s.n_query, s.n_invalid, s.n_matched, s.n_within) == (70, 1, 0, (0,)) and np.isnan(d2[3]) and np.isinf(np.delete(d2, 3)).all()
    assert (s.sum_dist, s.sum_dist2, s.max_dist2_seen) == (0.0, 0.0, 0.0)
    icp.map_add(_grid(-1.0, 1.0, 0.125))
    assert icp.map_size()[1] < 17 ** 3
    for n in (0, 1, 31, 32, 33, 63, 64, 65, CMP_CHUNK + 1):
        q = _dyadic_queries(rng, n, -1.75, 1.75)
        if n > 40:
            q[n // 2] = [np.inf, 0.0, 0.0]
        s, d2 = _check(icp, q, thresholds=(0.0625, 0.25, 0.5), what=f"n = {n}")
        assert s.n_query == n and len(d2) == n
        if n == 0:
            assert (s.n_matched, s.sum_dist, s.device_ms) == (0, 0.0, 0.0)
        if n > 1000:
            assert 0 < s.n_matched < n - 1, "some queries lie beyond max_dist of every stored point"
    icp.close()


# 3. long probe chains, the wrap, tombstones: the hash scenes as reference maps, queried with their own points jittered by dyadic offsets
def test_hash_scenes_as_reference_maps():
    from tests.helpers import hash_scenes as hs
    cap = 1 << 12
    sc = hs.map_stage_scene(cap)
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core
    icp = core.Icp(sc["max_range"], 0.0, voxel_size=1.0, map_table_capacity=cap, map_block_capacity=1 << 12, max_points_per_scan=4096)
    rng = np.random.default_rng(11)

    def probe(what):
        pts = icp.map_points()
        own = pts[::9] + rng.integers(-8, 9, (len(pts[::9]), 3)) / 16.0
        gone = hs.points_in(sc["absent"], 0.5)
        _check(icp, np.concatenate([own, gone]), thresholds=(0.25, 0.5, 1.0), what=what)

    for b in sc["batches"]:
        icp.map_add(b)
    probe("insert")
    before = icp.map_size()[0]
    icp.map_add(np.zeros((0, 3)), origin=sc["origin"])
    assert icp.map_size()[0] < before - 50, "the prune leaves tombstones"
    probe("prune")
    icp.map_add(sc["reinsert"])
    probe("reinsert")
    icp.close()


# 4. both block classes, and a voxel that moved to a full block: the map of a free-running batch with map_small_blocks
def test_a_map_with_small_and_full_blocks():
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import _lib as L, core
    from tests.helpers import full_voxel_scenes as fv
    frames = fv.box_sweeps()
    P = fv.BOX_P_TWO_CLASSES
    kw = dict(max_range=fv.BOX_RANGE, min_range=fv.BOX_MIN, with_ekf=False, max_points_per_scan=fv.BOX_PTS, **fv.BOX_ICP)
    kw.update(max_points_per_voxel=P, map_small_blocks=1 << 12)
    r = core.BatchRunner(1, fv.BOX_N, fv.BOX_PTS, 0, team_workgroups=2, free_running=True, **kw)
    try:
        for k, f in enumerate(frames):
            r.upload_scan(0, k, f)
        r.upload_imu(0, np.zeros((0, 7)), [0] * fv.BOX_N)
        r.run()
        member = core.Icp.__new__(core.Icp)  # a view of the batch's own handle: the runner owns it
        member.cfg = core.icp_cfg(fv.BOX_RANGE, fv.BOX_MIN, **dict(fv.BOX_ICP, max_points_per_voxel=P))
        member._h = C.c_void_p()
        L.check(L.lib().ptl_batch_icp(r._h, 0, C.byref(member._h)))
        try:
            pts = member.map_points()
            vox = np.trunc(pts / member.cfg.voxel_size).astype(np.int64)
            _, counts = np.unique(vox, axis=0, return_counts=True)
            assert (counts <= 5).any() and (counts > 5).any(), "voxels of both block classes"
            rng = np.random.default_rng(3)
            q = pts[::2] + rng.integers(-16, 17, (len(pts[::2]), 3)) / 32.0
            _check(member, q, thresholds=(0.25, 1.0), what="two block classes")
            s, (xyz, d2) = member.map_compare(member, per_point=True)
            assert s.n_query == s.n_matched == len(pts) and (d2 == 0.0).all()
            assert np.array_equal(xyz[_lex(xyz)], pts[_lex(pts)])
        finally:
            member._h = None
    finally:
        r.close()


# 5. the pool source
def test_pool_source_against_the_array_source():
    rng = np.random.default_rng(5)
    cloud = _dyadic_queries(rng, 3000, -3.0, 3.0, denom=32)
    moved = cloud[:2000] + np.array([0.0625, -0.03125, 0.125])
    ref, src, src2 = _icp(0.5, P=5), _icp(0.5, P=5), _icp(0.5, P=20)
    ref.map_add(cloud)
    src.map_add(moved)
    thr = (0.0625, 0.125, 0.5)
    s, (xyz, d2) = ref.map_compare(src, thresholds=thr, per_point=True)
    pts = src.map_points()
    assert s.n_query == len(pts) == len(xyz) and 0 < s.n_matched
    sa, d2a = ref.map_distance(pts, thresholds=thr, per_point=True)
    o, oa = _lex(xyz), _lex(pts)
    assert np.array_equal(xyz[o], pts[oa]) and _same(d2[o], d2a[oa])
    assert (s.n_matched, s.n_within, s.n_invalid, s.max_dist2_seen) == (sa.n_matched, sa.n_within, sa.n_invalid, sa.max_dist2_seen)
    _check_summary(s, d2, 0.5, thr, "pool source")
    want = mc.dist2(xyz, ref.map_points(), 0.5, 0.5)
    assert _same(d2, want)
    assert ref.map_compare(src, thresholds=thr).n_within == s.n_within

    # a handle against itself
    me, (mx, md2) = ref.map_compare(ref, per_point=True)
    assert me.n_query == me.n_matched == ref.map_size()[1] and (md2 == 0.0).all() and me.sum_dist == 0.0 and me.n_within == (me.n_query,)

    # the same points in another order (and another cap: every voxel keeps all of them): equal sorted outputs
    src3 = _icp(0.5, P=20)
    src2.map_add(moved)
    src3.map_add(moved[::-1])
    a, (ax, ad) = ref.map_compare(src2, thresholds=thr, per_point=True)
    b, (bx, bd) = ref.map_compare(src3, thresholds=thr, per_point=True)
    oa, ob = _lex(ax), _lex(bx)
    assert len(ax) == len(moved) and np.array_equal(ax[oa], bx[ob]) and _same(ad[oa], bd[ob])
    assert (a.n_matched, a.n_within) == (b.n_matched, b.n_within)
    for h in (ref, src, src2, src3):
        h.close()


# 6. the pass only reads: both maps and a continued registration are unchanged bit for bit; two calls give identical bytes
def test_read_only_and_repeatable():
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import synth
    seq = synth.make_sequence(seed=31, n_scans=4, H=16, W=128)
    kw = dict(voxel_size=0.5, max_points_per_scan=16 * 128, scan_cols=128, **CAPS)
    from ptudes_lab_amd import core
    a, b = core.Icp(70.0, 1.0, **kw), core.Icp(70.0, 1.0, **kw)
    for k in range(2):
        x = seq.scan(k).astype(np.float64)
        pa, pb = a.register_frame(x), b.register_frame(x)
        assert np.array_equal(pa, pb)
    other = _icp(0.5)
    other.map_add(a.map_points()[::2] + 0.03125)
    before, before_other = a.map_points(), other.map_points()
    q = before[::3] + 0.0625
    r1 = a.map_distance(q, thresholds=(0.1, 0.5), per_point=True)
    r2 = a.map_distance(q, thresholds=(0.1, 0.5), per_point=True)
    assert r1[1].tobytes() == r2[1].tobytes()
    c1 = a.map_compare(other, per_point=True)
    c2 = a.map_compare(other, per_point=True)
    o1 = other.map_compare(a)
    assert c1[1][0].tobytes() == c2[1][0].tobytes() and c1[1][1].tobytes() == c2[1][1].tobytes()
    for x, y in ((r1[0], r2[0]), (c1[0], c2[0])):
        assert [getattr(x, f) for f in ("n_matched", "n_within", "sum_dist", "sum_dist2", "max_dist2_seen")] == \
               [getattr(y, f) for f in ("n_matched", "n_within", "sum_dist", "sum_dist2", "max_dist2_seen")]
    assert o1.n_query == len(before)
    after, after_other = a.map_points(), other.map_points()
    # (the export's order is not specified: sorted rows)
    assert np.array_equal(after[_lex(after)], before[_lex(before)]) and np.array_equal(after_other[_lex(after_other)], before_other[_lex(before_other)])
    assert a.map_size() == b.map_size()
    for k in range(2, 4):  # the registration goes on as in the handle that was never compared
        x = seq.scan(k).astype(np.float64)
        assert np.array_equal(a.register_frame(x), b.register_frame(x))
    pa, pb = a.map_points(), b.map_points()
    assert np.array_equal(pa[_lex(pa)], pb[_lex(pb)])
    for h in (a, b, other):
        h.close()


def _refused(code, fn):
    with pytest.raises((RuntimeError, ValueError)) as e:
        fn()
    if code == PTL_ERR_ARG:
        assert isinstance(e.value, ValueError)
    else:
        assert f"libptudes_mi error {code}:" in str(e.value), str(e.value)
    return str(e.value)


# 7. refusals through the binding: each message names the numbers; nothing written
def test_refusals():
    from ptudes_lab_amd import _lib
    ref, src = _icp(0.5), _icp(0.5)
    ref.map_add(_grid(-0.5, 0.5, 0.25))
    src.map_add(_grid(-0.5, 0.5, 0.25) + 0.0625)
    q = np.zeros((3, 3))
    msg = _refused(PTL_ERR_ARG, lambda: ref.map_distance(q, max_dist=0.75))
    assert "max_dist = 0.75" in msg and "voxel size = 0.5" in msg
    assert "max_dist = 0" in _refused(PTL_ERR_ARG, lambda: ref.map_distance(q, max_dist=0.0))
    _refused(PTL_ERR_ARG, lambda: ref.map_distance(q, max_dist=float("nan")))
    assert "n_thresholds = 9" in _refused(PTL_ERR_ARG, lambda: ref.map_distance(q, thresholds=[0.1] * 9))
    assert "n_thresholds = 0" in _refused(PTL_ERR_ARG, lambda: ref.map_distance(q, thresholds=[]))
    msg = _refused(PTL_ERR_ARG, lambda: ref.map_distance(q, thresholds=[0.1, 0.6]))
    assert "threshold 1 = 0.6" in msg and "max_dist = 0.5" in msg
    assert "threshold 0 = 0" in _refused(PTL_ERR_ARG, lambda: ref.map_distance(q, thresholds=[0.0, 0.1]))
    msg = _refused(PTL_ERR_ARG, lambda: ref.map_compare(src, thresholds=[0.2, 0.1]))
    assert "threshold 1 = 0.1" in msg and "threshold 0 = 0.2" in msg and "ascending" in msg
    L = _lib.lib()
    cfg = _lib.MapCmpCfg()
    _lib.check(L.ptl_map_cmp_default_cfg(C.byref(cfg), 0.5))
    res = _lib.MapCmpResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    blank = b"\x5a" * C.sizeof(res)
    assert L.ptl_icp_map_distance(ref._h, C.byref(cfg), _lib.dptr(q), -1, C.byref(res), None) == PTL_ERR_ARG
    assert "n = -1" in L.ptl_last_error().decode() and bytes(res) == blank
    assert L.ptl_icp_map_distance(ref._h, C.byref(cfg), None, 3, C.byref(res), None) == PTL_ERR_ARG
    assert "3 queries" in L.ptl_last_error().decode() and bytes(res) == blank
    # max_points one below the count: the count is named, nothing written; the two arrays come together
    n = src.map_size()[1]
    xyz, d2, w = np.full((n, 3), -7.0), np.full(n, -7.0), C.c_int64(-7)
    rc = L.ptl_icp_map_compare(ref._h, src._h, C.byref(cfg), C.byref(res), _lib.dptr(xyz), _lib.dptr(d2), n - 1, C.byref(w))
    msg = L.ptl_last_error().decode()
    assert rc == PTL_ERR_CAPACITY and str(n) in msg and str(n - 1) in msg
    assert (xyz == -7.0).all() and (d2 == -7.0).all()
    rc = L.ptl_icp_map_compare(ref._h, src._h, C.byref(cfg), C.byref(res), _lib.dptr(xyz), None, n, C.byref(w))
    assert rc == PTL_ERR_ARG and "together" in L.ptl_last_error().decode()
    rc = L.ptl_icp_map_compare(ref._h, src._h, C.byref(cfg), C.byref(res), _lib.dptr(xyz), _lib.dptr(d2), n, C.byref(w))
    assert rc == 0 and w.value == n and res.n_query == n and (d2 >= 0.0).all()
    # a stale struct
    cfg.struct_size = 80
    assert L.ptl_icp_map_distance(ref._h, C.byref(cfg), _lib.dptr(q), 3, C.byref(res), None) == PTL_ERR_ARG
    assert "80" in L.ptl_last_error().decode() and "88" in L.ptl_last_error().decode()
    # the handles are as usable as before
    assert ref.map_distance(q).n_query == 3
    for h in (ref, src):
        h.close()


def _block(output):
    """the numbers of the printed comparison block"""
    m = re.search(r"map comparison: reference (\S+) \((\d+) points\), max dist (\S+) m", output)
    assert m, output
    dirs = re.findall(r"(accuracy|completeness) \([^)]*\): (\d+) queries, (\d+) matched, mean (\S+) mm, rms (\S+) mm", output)
    rows = re.findall(r"at (\S+) m: precision (\S+), recall (\S+), F (\S+)", output)
    assert len(dirs) == 2, output
    return int(m.group(2)), float(m.group(3)), [(d[0], int(d[1]), int(d[2]), d[3], d[4]) for d in dirs], [tuple(r) for r in rows]


# 8. the commands
def test_commands_compare_the_map_they_built(tmp_path):
    from click.testing import CliRunner
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import fly, synth
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    run = CliRunner().invoke
    n = 6
    seq = synth.make_sequence(seed=1000, n_scans=n)
    kt = np.arange(0, n * seq.scan_dt + 0.3, 0.02)
    gt, ref_ply = str(tmp_path / "gt.csv"), str(tmp_path / "ref.ply")
    pu.save_poses_nc_gt_format(gt, t=[seq.t_base + float(t) for t in kt], poses=[seq.pose_at(np.array([t]))[0] for t in kt])
    base = ["flyby", "--synthetic", "1000", "--end-scan", "5", "--nc-gt-poses", gt]
    res = run(ptudes_cli, base + ["--save-map", ref_ply])
    assert res.exit_code == 0, res.output
    ref_pts = pu.load_map_ply(ref_ply)

    # the same map against the file it wrote: the reference handle has the run map's voxel size and points per voxel, so it reloads completely
    res = run(ptudes_cli, base + ["--compare-map", ref_ply])
    assert res.exit_code == 0, res.output
    n_ref, max_dist, dirs, rows = _block(res.output)
    assert n_ref == len(ref_pts) and max_dist == 0.5
    for _, queries, matched, mean, rms in dirs:
        assert queries == matched == len(ref_pts) and float(mean) == 0.0 and float(rms) == 0.0
    assert [r[0] for r in rows] == ["0.05", "0.1", "0.2"] and all(float(x) == 1.0 for r in rows for x in r[1:])
    # --compare-threshold / --compare-max-dist are echoed
    res = run(ptudes_cli, base + ["--compare-map", ref_ply, "--compare-threshold", "0.05,0.25", "--compare-max-dist", "0.25"])
    assert res.exit_code == 0 and [r[0] for r in _block(res.output)[3]] == ["0.05", "0.25"] and _block(res.output)[1] == 0.25, res.output

    # ekf-bench: the filter's map against the ground-truth map, equal to MapAccumulator.compare on the same two clouds
    poses_csv, err_ply, run_ply = str(tmp_path / "p.csv"), str(tmp_path / "err.ply"), str(tmp_path / "run.ply")
    # (the fly-by moves its poses to the start scan's; ekf-bench's map is in the filter's frame, which starts at the identity as well)
    ekf = ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "5", "--use-imu-prediction"]
    res = run(ptudes_cli, ekf + ["--compare-map", ref_ply, "--save-map-error", err_ply, "--save-map", run_ply, "--save-nc-gt-poses", poses_csv])
    assert res.exit_code == 0, res.output
    got = _block(res.output)
    run_pts = pu.load_map_ply(run_ply)
    lut, _ = fly.synthetic_range_scans(seq, 0, 0)
    acc = fly.MapAccumulator(lut, voxel_size=0.5)
    step = int(acc._icp.cfg.max_points_per_scan)
    for off in range(0, len(run_pts), step):
        acc._icp.map_add(run_pts[off:off + step])
    assert acc.map_size()[1] == len(run_pts)
    want, (wx, wd2) = acc.compare(ref_pts, per_point=True, reference_name=ref_ply)
    assert _block("\n".join(want.lines())) == got
    assert want.precision == want.accuracy.fractions and all(0.0 < p <= 1.0 for p in want.precision[1:])
    f = want.f_score
    assert all(abs(f[k] - 2 * want.precision[k] * want.recall[k] / (want.precision[k] + want.recall[k])) < 1e-15 for k in range(3) if f[k] > 0)
    # against the restatement: a few hundred of the map's points against the whole reference cloud (brute force: rows in small blocks)
    sub = slice(None, None, max(1, len(wx) // 256))
    assert _same(wd2[sub], mc.dist2(wx[sub], ref_pts, 0.5, 0.5, block=32))
    assert want.accuracy.n_query == len(run_pts) and want.completeness.n_query == len(ref_pts)
    # the error map: one finite-or-NaN scalar per map point, the square roots of the per-point values
    epts, extras = pu.load_map_ply(err_ply, scalars=True)
    dist = extras["dist"]
    assert len(epts) == len(dist) == len(run_pts) and (np.isnan(dist) | (np.isfinite(dist) & (dist >= 0.0))).all()
    o, ow = _lex(epts), _lex(wx)
    wdist = np.sqrt(wd2)
    wdist[~np.isfinite(wd2)] = np.nan
    assert np.array_equal(epts[o], wx[ow]) and _same(dist[o], wdist[ow])
    acc.close()

    # --compare-pose: a translated copy of a reference, brought back by a pure dyadic translation, reproduces the untransformed numbers.
    # The reference is the copy moved back, (ref - t) + t as the doubles give it: the host's ((1 x + 0 y) + 0 z) + t is that sum exactly
    shifted, moved_back, pose = str(tmp_path / "shifted.npy"), str(tmp_path / "moved_back.npy"), str(tmp_path / "pose.txt")
    t = np.array([4.0, -2.5, 0.75])
    np.save(shifted, ref_pts - t)
    np.save(moved_back, (ref_pts - t) + t)
    open(pose, "w").write("1 0 0 4\n0 1 0 -2.5\n0 0 1 0.75\n")
    a = run(ptudes_cli, base + ["--compare-map", shifted, "--compare-pose", pose])
    b = run(ptudes_cli, base + ["--compare-map", moved_back])
    assert a.exit_code == 0 and b.exit_code == 0, a.output + b.output
    assert _block(a.output) == _block(b.output) and _block(a.output)[0] == len(ref_pts)
    # ... and differ from the copy left where it is
    c = run(ptudes_cli, base + ["--compare-map", shifted])
    assert c.exit_code == 0 and _block(c.output)[3] != _block(a.output)[3], c.output
