"""The map score on the device (csrc/score_kernels.h) against its numpy restatement (tests/helpers/map_score_numpy.py) run
on `map_points()` of the same handle: every stored point, matched by sorting rows.  Neighbour counts and the sparse sets are equal exactly
(the membership expression is the same on both sides, without contraction); the rest within derived bounds
(tests/helpers/map_score_check.py holds the check; tests/test_gpu_hash_tables.py uses it too):

  atol_lambda = 8 * 27 * P * eps * radius^2   Sigma's entries are sums of at most 27 P terms of at most radius^2 each, accumulated in
                                              another order on the device (two lanes per point, then one add): a few n eps radius^2 per
                                              entry, and an eigenvalue moves by at most the perturbation's norm (Weyl)
  atol_h = 1.5 * atol_lambda / sigma_floor^2 + 8 * eps * max(1, |h|)
                                              d ln(lambda + floor^2) <= d lambda / floor^2, three of them, times 0.5; the second term is for log
                                              itself: ROCm documents 1 ulp for the double-precision log of its device library (HIP math API,
                                              double precision table), three logs and the sums around them stay below 8 eps of the result
  means: (n_scored - 1) eps relative (plane variance) and (n_scored - 1) eps sum|h_i| / n_scored absolute (entropy) for the summation order of
  non-negative terms / of terms of either sign, plus the per-point bound.

Per-call `core.Icp` maps with small capacities (tests/test_gpu_posed_map.py's CAPS)."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers.map_score_check import check as _check, lex as _lex, sorted_score as _sorted_score

pytestmark = pytest.mark.gpu

CAPS = dict(map_block_capacity=1 << 16, map_table_capacity=1 << 18)
H, W, N = 32, 256, 6
BOUNDS = 1.5
PTL_ERR_ARG, PTL_ERR_CAPACITY = -1, -3


def _icp(voxel, P=20, n_max=1 << 16, cols=64, **over):
    from ptudes_lab_amd import core
    kw = dict(voxel_size=voxel, max_points_per_voxel=P, scan_cols=cols, max_points_per_scan=n_max, **CAPS)
    kw.update(over)
    return core.Icp(1.0e9, 0.0, **kw)


def _lattice_cloud():
    from tests.helpers import lattice_scenes as ls
    lone = np.array([[40.25, 0.25, 0.25], [-40.25, 30.25, 0.25], [0.25, -55.25, 7.25], [-0.25, -0.25, 33.25]])
    return np.concatenate([ls.lattice_block(), ls.outlier_cluster(), lone])


# 1. every neighbour at two lattice steps lies exactly at the radius, both signs of every coordinate, the cap binds around 0, sparse points
def test_lattice_block_with_outliers_and_isolated_points():
    cloud = _lattice_cloud()
    icp = _icp(1.0, P=20)
    icp.map_add(cloud)
    voxels, points = icp.map_size()
    assert points < len(cloud), "the 20-point cap binds in the double-width voxels around 0"
    s, ref = _check(icp, 20, want_sparse=True)
    assert s.n_sparse >= 4 and s.n_scored > 10000
    # an interior lattice point away from 0 has its 33 neighbours within 1.0 (1 + 6 + 12 + 8 + 6 at exactly 1.0)
    _, xyz, n, pv, _ = _sorted_score(icp)
    inner = (np.abs(xyz) > 2.5).all(axis=1) & (np.abs(xyz) < 4.5).all(axis=1)
    assert inner.any() and (n[inner] == 33).all()
    # min_neighbours = 1 scores the isolated points too
    _check(icp, 20, min_neighbours=1, want_sparse=False)


# 2. a radius below the voxel size, small blocks of three points
def test_lattice_block_three_points_per_voxel_radius_below_the_voxel():
    icp = _icp(1.0, P=3)
    icp.map_add(_lattice_cloud())
    s, _ = _check(icp, 3, radius=0.75, min_neighbours=3, want_sparse=True)
    assert s.n_scored > 0


# 3. coordinates on and 1 - 2 ulp beside voxel faces, large |k|
def test_boundary_cloud():
    from tests.helpers import lattice_scenes as ls
    cloud = ls.boundary_cloud(0.5)
    icp = _icp(0.5, P=20)
    icp.map_add(cloud)
    s, _ = _check(icp, 20, min_neighbours=2)
    assert s.n_scored > 0
    _check(icp, 20, radius=0.25, min_neighbours=2, sigma_floor=0.001)


class _Fix:
    pass


@pytest.fixture(scope="module")
def fx():
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core, fly, synth
    f = _Fix()
    f.seq = synth.make_sequence(seed=31, n_scans=N, H=H, W=W)
    f.lut, f.scans = fly.synthetic_range_scans(f.seq)
    kt = np.arange(0, N * f.seq.scan_dt + 0.3, 0.02)
    f.knots = [(f.seq.t_base + float(t), f.seq.pose_at(np.array([t]))[0]) for t in kt]
    f.traj = core.Traj([k[0] for k in f.knots], [k[1] for k in f.knots], BOUNDS, BOUNDS)
    return f


def _posed(fx, traj=None):
    from ptudes_lab_amd import fly
    acc = fly.MapAccumulator(fx.lut, voxel_size=0.5, **CAPS)
    for sc in fx.scans:
        acc.update(sc, traj=traj or fx.traj)
    return acc


def _same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) and x.dtype == y.dtype for x, y in zip(a, b))


# 4. a posed map built twice: the per-point values do not depend on block ids; scoring twice; the map is left alone
def test_posed_map_built_twice_scores_bit_equal(fx):
    a, b = _posed(fx), _posed(fx)
    sa = _sorted_score(a._icp)
    sb = _sorted_score(b._icp)
    assert sa[0].n_points == a.map_size()[1] > 10000 and sa[0].n_scored > 0
    assert _same_bits(sa[1:], sb[1:])
    assert (sa[0].n_points, sa[0].n_scored, sa[0].n_sparse) == (sb[0].n_points, sb[0].n_scored, sb[0].n_sparse)
    pts, size = a.map_points(), a.map_size()
    again = _sorted_score(a._icp)
    assert _same_bits(sa[1:], again[1:])
    assert again[0].mean_plane_var == sa[0].mean_plane_var and again[0].mean_entropy == sa[0].mean_entropy
    after = a.map_points()  # (the export's order is not specified: sorted rows)
    assert a.map_size() == size and np.array_equal(after[_lex(after)], pts[_lex(pts)])
    # through the accumulator, and against the restatement
    assert a.score().n_scored == sa[0].n_scored
    _check(a._icp, 20)


# 5. the score orders a sharp map before a blurred one, and the device agrees with the restatement on both
def test_ordering_of_ground_truth_and_yawed_poses(fx):
    from ptudes_lab_amd import core
    from tests.helpers import map_score_numpy as ms
    ang = np.radians(2.0)
    yawed = []
    for i, (t, p) in enumerate(fx.knots):
        c, s = np.cos(ang), np.sin(ang) * (1.0 if i % 2 == 0 else -1.0)
        Rz = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
        yawed.append(p @ Rz)
    bad_traj = core.Traj([k[0] for k in fx.knots], yawed, BOUNDS, BOUNDS)
    good, bad = _posed(fx), _posed(fx, bad_traj)
    means = []
    for acc in (good, bad):
        pts = acc.map_points()
        n, pv, ent, _ = ms.score_points(pts, 0.5, 5, 0.005)
        means.append(ms.summary(n, pv, ent, 5)["mean_plane_var"])
    print(f"restatement: mean plane variance {means[0]:.6e} (ground truth) against {means[1]:.6e} (yawed by +-2 deg)")
    assert means[0] < means[1], "the scene does not separate the two trajectories"
    s_good, _ = _check(good._icp, 20)
    s_bad, _ = _check(bad._icp, 20)
    assert s_good.mean_plane_var < s_bad.mean_plane_var


def _refused(code, fn):
    with pytest.raises((RuntimeError, ValueError)) as e:
        fn()
    if code == PTL_ERR_ARG:
        assert isinstance(e.value, ValueError)
    else:
        assert f"libptudes_mi error {code}:" in str(e.value), str(e.value)
    return str(e.value)


# 6. refusals: an error code, nothing written, the map still usable
def test_refusals_and_the_empty_map():
    from ptudes_lab_amd import _lib, core
    from tests.helpers import lattice_scenes as ls
    icp = _icp(1.0, P=20)
    empty = icp.map_score()
    assert (empty.n_points, empty.n_scored, empty.n_sparse) == (0, 0, 0)
    assert (empty.mean_plane_var, empty.mean_entropy, empty.mean_neighbours) == (0.0, 0.0, 0.0)
    assert (empty.radius, empty.min_neighbours, empty.sigma_floor) == (1.0, 5, 0.01)
    s0, (xyz0, n0, _, _) = icp.map_score(per_point=True)
    assert len(xyz0) == len(n0) == 0 and s0.n_points == 0
    icp.map_add(ls.lattice_block(-2.0, 2.0))
    want = icp.map_score()
    assert want.n_points == icp.map_size()[1] > 0
    msg = _refused(PTL_ERR_ARG, lambda: icp.map_score(radius=0.0))
    assert "radius = 0" in msg and "voxel size = 1" in msg
    msg = _refused(PTL_ERR_ARG, lambda: icp.map_score(radius=1.5))
    assert "1.5" in msg and "voxel size = 1" in msg
    assert "min_neighbours = 0" in _refused(PTL_ERR_ARG, lambda: icp.map_score(min_neighbours=0))
    assert "sigma_floor = 0" in _refused(PTL_ERR_ARG, lambda: icp.map_score(sigma_floor=0.0))
    _refused(PTL_ERR_ARG, lambda: icp.map_score(radius=float("nan")))

    # max_points one below the count: the count is named, the summary and the arrays keep their bytes
    L, n = _lib.lib(), want.n_points
    cfg = _lib.MapScoreCfg()
    _lib.check(L.ptl_map_score_default_cfg(C.byref(cfg), 1.0))
    res = _lib.MapScoreResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    xyz, nb, pv, ent = np.full((n, 3), -7.0), np.full(n, -7, np.int32), np.full(n, -7.0), np.full(n, -7.0)
    w = C.c_int64(-7)
    args = (_lib.dptr(xyz), nb.ctypes.data_as(C.POINTER(C.c_int32)), _lib.dptr(pv), _lib.dptr(ent))
    rc = L.ptl_icp_map_score(icp._h, C.byref(cfg), C.byref(res), *args, n - 1, C.byref(w))
    assert rc == PTL_ERR_CAPACITY and str(n) in L.ptl_last_error().decode() and str(n - 1) in L.ptl_last_error().decode()
    assert bytes(res) == b"\x5a" * C.sizeof(res) and w.value == -7
    assert (xyz == -7.0).all() and (nb == -7).all() and (pv == -7.0).all() and (ent == -7.0).all()
    # the four arrays come together or not at all
    rc = L.ptl_icp_map_score(icp._h, C.byref(cfg), C.byref(res), args[0], None, args[2], args[3], n, C.byref(w))
    assert rc == PTL_ERR_ARG and "together" in L.ptl_last_error().decode() and bytes(res) == b"\x5a" * C.sizeof(res)
    # ... and with room for all of them the call goes through
    rc = L.ptl_icp_map_score(icp._h, C.byref(cfg), C.byref(res), *args, n, C.byref(w))
    assert rc == 0 and w.value == n and res.n_points == n and (nb >= 1).all()

    # points per voxel: a handle with 99 would need more staging than the score allows, but no such handle exists - creation refuses more
    # than 32 (the search's limit), which is where this case ends
    assert "max_points_per_voxel" in _refused(PTL_ERR_ARG, lambda: _icp(1.0, P=99))

    # the map is as usable as before
    again = icp.map_score()
    assert (again.n_scored, again.mean_plane_var, again.mean_entropy) == (want.n_scored, want.mean_plane_var, want.mean_entropy)
    icp.map_add(ls.outlier_cluster())
    assert icp.map_score().n_points == n + 64


def _block_values(output):
    import re
    m = re.search(r"points: (\d+) \(scored (\d+), sparse (\d+)\)", output)
    assert m, output
    assert "map score: radius" in output and "mean plane variance:" in output and "wall thickness" in output and "mean map entropy:" in output
    return tuple(int(g) for g in m.groups())


# 7. the commands print the block and write the scalars of the map they built
def test_commands_print_the_score_and_write_the_scalars(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd import core, fly, synth
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    from ptudes_lab_amd.sequence import sweep_times
    p, m1, m2 = str(tmp_path / "p.csv"), str(tmp_path / "m.ply"), str(tmp_path / "m2.ply")
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "5", "--use-imu-prediction",
                                          "--save-nc-gt-poses", p, "--save-map", m1, "--map-score"])
    assert res.exit_code == 0, res.output
    pts, (nb, pv, ent) = pu.load_map_ply(m1, scalars=True)
    counts = _block_values(res.output)
    assert counts[0] == len(pts) and counts[1] == int((nb >= 5).sum()) and counts[2] == int((nb < 5).sum())
    rows = pu.read_newer_college_gt(p)
    seq = synth.make_sequence(seed=1000, n_scans=6)
    r = core.SeqRunner(6, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    for k in range(6):
        r.upload_scan(k, seq.scan(k))
    m = core.Icp(1.0e9, 0.0, voxel_size=0.5, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 21,
                 map_table_capacity=1 << 23)
    traj = core.Traj([t for t, _ in rows], [q for _, q in rows], BOUNDS, BOUNDS)
    assert r.build_map(m, traj, sweep_times(seq))[1] == 0
    want = _sorted_score(m)[1:]
    o = _lex(pts)
    assert _same_bits(want, (pts[o], nb[o], pv[o], ent[o]))
    # without --save-map the block is printed all the same
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "5", "--use-imu-prediction", "--map-score",
                                          "--map-from", "kiss"])
    assert res.exit_code == 0 and _block_values(res.output)[0] > 0 and "Map saved to" not in res.output, res.output

    res = CliRunner().invoke(ptudes_cli, ["flyby", "--synthetic", "1000", "--nc-gt-poses", p, "--end-scan", "5", "--save-map", m2, "--map-score",
                                          "--score-radius", "0.25"])
    assert res.exit_code == 0, res.output
    got, (nb, pv, ent) = pu.load_map_ply(m2, scalars=True)
    assert "radius 0.25 m" in res.output and _block_values(res.output)[0] == len(got) and f"map num points: {len(got)}" in res.output
    pose0_inv = np.linalg.inv(rows[0][1])
    lut, scans = fly.synthetic_range_scans(seq)
    acc = fly.MapAccumulator(lut, voxel_size=0.5)
    t2 = core.Traj([t for t, _ in rows], [pose0_inv @ q for _, q in rows], BOUNDS, BOUNDS)
    for sc in scans:
        acc.update(sc, traj=t2)
    _, (wx, wn, wpv, went) = acc.score(radius=0.25, per_point=True)
    o, ow = _lex(got), _lex(wx)
    assert _same_bits((wx[ow], wn[ow], wpv[ow], went[ow]), (got[o], nb[o], pv[o], ent[o]))


def test_native_packet_bag_into_the_map(tmp_path):
    import json
    from click.testing import CliRunner
    from ptudes_lab_amd import bag, core, fly, synth
    from ptudes_lab_amd import packets as pk
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    from ptudes_lab_amd.ins.data import GRAV
    from tests import bagwriter as bw
    from tests.helpers import ouster_packets_numpy as opn
    Hs, Ws, n = 16, 64, 4
    profile = "RNG19_RFL8_SIG16_NIR16"
    seq = synth.make_sequence(seed=1010, n_scans=n, H=Hs, W=Ws)
    meta = {"beam_altitude_angles": list(np.linspace(45.0, -45.0, Hs)), "beam_azimuth_angles": [0.0] * Hs,
            "lidar_origin_to_beam_origin_mm": 0.0, "lidar_mode": f"{Ws}x10", "prod_line": "OS-0-16",
            "lidar_to_sensor_transform": np.eye(4).reshape(-1).tolist(), "imu_to_sensor_transform": np.eye(4).reshape(-1).tolist(),
            "data_format": {"pixels_per_column": Hs, "columns_per_frame": Ws, "columns_per_packet": 16, "udp_profile_lidar": profile}}
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    conns = [("/os_node/lidar_packets", "ouster_ros/PacketMsg", bag.OUSTER_PACKETMSG_MD5),
             ("/os_node/imu_packets", "ouster_ros/PacketMsg", bag.OUSTER_PACKETMSG_MD5)]
    msgs, stream, t_bag = [], [], 10**9
    for k in range(n):
        a, e = seq.imu_range_for_scan(k)
        for i in range(a, e):
            ts_ns = int(round(seq.imu[i, 0] * 1e9))
            stream.append(("imu", bw.ouster_imu_packet(ts_ns, ts_ns, ts_ns, seq.imu[i, 1:4] / GRAV, np.degrees(seq.imu[i, 4:7]))))
        x = seq.scan(k).reshape(Hs, Ws, 3)
        img = np.round(np.linalg.norm(x[:, (Ws - np.arange(Ws)) % Ws, :], axis=2) * 1000.0).astype(np.uint32)
        t0 = int(round((seq.t_base + k * seq.scan_dt) * 1e9))
        ts = np.uint64(t0) + (np.arange(1, Ws + 1, dtype=np.uint64) * np.uint64(int(seq.scan_dt * 1e9) // Ws))
        stream += [("lidar", pkt) for pkt in opn.encode_sweep(profile, img, ts, np.ones(Ws, np.uint16), 100 + k, 16)]
    for kind, buf in stream:
        t_bag += 1000
        msgs.append((0 if kind == "lidar" else 1, t_bag, bw.packet_msg(buf)))
    bw.write_bag(tmp_path / "x.bag", conns, msgs)
    kt = np.arange(0, n * seq.scan_dt + 0.3, 0.02)
    poses = str(tmp_path / "gt.csv")
    pu.save_poses_nc_gt_format(poses, t=[seq.t_base + float(t) for t in kt], poses=[seq.pose_at(np.array([t]))[0] for t in kt])

    out = str(tmp_path / "bag.ply")
    res = CliRunner().invoke(ptudes_cli, ["flyby", str(tmp_path / "x.bag"), "-m", str(tmp_path / "meta.json"), "--nc-gt-poses", poses,
                                          "--native-packets", "--save-map", out])
    assert res.exit_code == 0, res.output
    got = pu.load_map_ply(out)
    assert len(got) > 0 and f"map num points: {len(got)}" in res.output and "0 skipped scans" in res.output

    # the same decoded sweeps through MapAccumulator.update(scan, traj=): every column at its decoded time
    info = pk.read_metadata_json(str(tmp_path / "meta.json"))
    rows = pu.read_newer_college_gt(poses)
    pose0_inv = np.linalg.inv(rows[0][1])
    traj = core.Traj([t for t, _ in rows], [pose0_inv @ q for _, q in rows], BOUNDS, BOUNDS)
    lut = core.Lut(Hs, Ws, info.beam_altitude_angles, info.beam_azimuth_angles, 0.0, np.eye(4))
    acc = fly.MapAccumulator(lut, voxel_size=0.5)
    feed = pk.PacketFeed([(kind, buf, 0.0) for kind, buf in stream], info)
    scans = [d for _, d in feed.withScanIdx() if not hasattr(d, "lacc")]
    assert len(scans) == n
    for sc in scans:
        assert acc.update(sc, traj=traj) == int(np.count_nonzero(sc.range))
    want = acc.map_points()
    assert np.array_equal(want[_lex(want)], got[_lex(got)])

    # ekf-bench on the same bag: the map of the filter's trajectory, scored, with and without the file
    m2 = str(tmp_path / "ekf.ply")
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", str(tmp_path / "x.bag"), "-m", str(tmp_path / "meta.json"), "--save-map", m2,
                                          "--map-score"])
    assert res.exit_code == 0, res.output
    pts, (nb, pv, ent) = pu.load_map_ply(m2, scalars=True)
    assert _block_values(res.output)[0] == len(pts) > 0 and f"Map saved to: {m2}" in res.output
    assert np.array_equal(np.isnan(pv), nb < 5) and np.array_equal(np.isnan(ent), nb < 5)
