"""Posed scans into the world map on the device: the fused per-call form against the three-call path (bit-equal: one
definition of the arithmetic) and against the numpy definition (tests/helpers/posed_map_numpy.py), the resident forms of both runners,
the runner left untouched, refusals and skipping, and the two commands.

Fixture (the recipe of tests/test_dewarp.py): synth.make_sequence(seed=31, n_scans=6, H=32, W=256), ground truth as knots every 20 ms,
range images on the ouster column convention, map capacities 1 << 16 / 1 << 18, voxel 0.5 - the smallest shape where the column index,
the row-major pixel order, more than one 256-thread block per row's worth of pixels and the ordered compaction can each go wrong.
Bounds against numpy: coordinates are tens of metres (ulp ~ 1e-14), the geodesic goes through log / exp (the existing device-vs-oracle
bound is 1e-10 on the poses): 1e-9 m, as the issue sets."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, N = 32, 256, 6
CAPS = dict(map_block_capacity=1 << 16, map_table_capacity=1 << 18)
BOUNDS = 1.5
PTL_ERR_CAPACITY, PTL_ERR_STATE = -3, -4


def _sorted(p):
    p = np.asarray(p)
    return p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]


def _same_map(a, b):
    """bit-equal maps: sizes and the lexicographically sorted rows"""
    assert a.map_size() == b.map_size()
    assert np.array_equal(_sorted(a.map_points()), _sorted(b.map_points()))


def _near(a_pts, b_pts, tol):
    from scipy.spatial import cKDTree
    assert len(a_pts) == len(b_pts) and len(a_pts) > 0
    da, _ = cKDTree(b_pts).query(a_pts)
    db, _ = cKDTree(a_pts).query(b_pts)
    print(f"neighbour distance both ways: {da.max():.3e} {db.max():.3e} (bound {tol:.0e})")
    assert da.max() < tol and db.max() < tol


class _Fix:
    pass


@pytest.fixture(scope="module")
def fx():
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core, fly, synth
    from ptudes_lab_amd.sequence import sweep_times
    from tests.helpers import posed_map_numpy as pm
    f = _Fix()
    f.seq = synth.make_sequence(seed=31, n_scans=N, H=H, W=W)
    f.alt, f.az = np.linspace(45.0, -45.0, H), np.zeros(H)
    f.lut, f.scans = fly.synthetic_range_scans(f.seq)
    kt = np.arange(0, N * f.seq.scan_dt + 0.3, 0.02)
    f.knots = [(f.seq.t_base + float(t), f.seq.pose_at(np.array([t]))[0]) for t in kt]
    f.traj = core.Traj([k[0] for k in f.knots], [k[1] for k in f.knots], BOUNDS, BOUNDS)
    f.t0t1 = sweep_times(f.seq)
    f.xyz = [f.seq.scan(k) for k in range(N)]  # f32, sensor frame, (0,0,0) = no return
    # the numpy definition, computed once: per range-image scan (column times of the scan) and per xyz sweep (sweep times)
    f.ref_range = [pm.posed_points(pm.range_image_points(s.range_mm, f.alt, f.az), np.asarray(s.timestamp, dtype=np.float64) * 1e-9, f.knots, BOUNDS)
                   for s in f.scans]
    f.ref_xyz = [pm.posed_points(np.asarray(x, dtype=np.float64).reshape(H, W, 3), pm.sweep_column_times(t[0], t[1], W), f.knots, BOUNDS)
                 for x, t in zip(f.xyz, f.t0t1)]
    assert all(p is not None for p in f.ref_range + f.ref_xyz)
    return f


def _map_icp(cols=W, **over):
    from ptudes_lab_amd import core
    kw = dict(voxel_size=0.5, scan_cols=cols, max_points_per_scan=H * W, **CAPS)
    kw.update(over)
    return core.Icp(1.0e9, 0.0, **kw)


def _numpy_map(point_sets):
    m = _map_icp()
    for p in point_sets:
        m.map_add(p)
    return m


def _acc(fx):
    from ptudes_lab_amd import fly
    return fly.MapAccumulator(fx.lut, voxel_size=0.5, **CAPS)


def test_fused_per_call_equals_the_three_call_path(fx):
    from ptudes_lab_amd import utils as pu
    three, fused = _acc(fx), _acc(fx)
    for sc in pu.pose_scans_from_nc_gt(fx.scans, nc_gt_poses=fx.knots):
        three.update(sc)
    got = [fused.update(sc, traj=fx.traj) for sc in fx.scans]
    assert got == [int(np.count_nonzero(sc.range_mm)) for sc in fx.scans]
    assert three.scans == fused.scans == N and fused.skipped == 0
    assert three.returns == fused.returns == sum(got)
    _same_map(three, fused)
    ref = _numpy_map(fx.ref_range)
    assert ref.map_size() == fused.map_size()
    _near(fused.map_points(), ref.map_points(), 1e-9)


def _seq_runner(fx, **kw):
    from ptudes_lab_amd import core
    r = core.SeqRunner(N, H * W, 0, max_range=fx.seq.max_range, min_range=fx.seq.min_range, with_ekf=False, scan_cols=W, **CAPS, **kw)
    for k in range(N):
        r.upload_scan(k, fx.xyz[k])
    return r


def test_resident_xyz_sweeps(fx):
    r = _seq_runner(fx)  # uploaded, never run
    m = _map_icp()
    n_valid, n_skipped = r.build_map(m, fx.traj, fx.t0t1)
    assert n_skipped == 0 and n_valid == sum(len(p) for p in fx.ref_xyz)
    ref = _numpy_map(fx.ref_xyz)
    assert m.map_size() == ref.map_size()
    _near(m.map_points(), ref.map_points(), 1e-9)
    # first / last: scans 2 .. 4 only
    m2, ref2 = _map_icp(), _numpy_map(fx.ref_xyz[2:5])
    n_valid, n_skipped = r.build_map(m2, fx.traj, fx.t0t1, first=2, last=4)
    assert (n_valid, n_skipped) == (sum(len(p) for p in fx.ref_xyz[2:5]), 0)
    assert m2.map_size() == ref2.map_size() and m2.map_size() != m.map_size()
    _near(m2.map_points(), ref2.map_points(), 1e-9)
    # the per-call xyz form is the same definition: bit-equal to the resident one
    from tests.helpers import posed_map_numpy as pm
    m3 = _map_icp()
    for k in range(2, 5):
        nv, sk = m3.map_add_posed(fx.traj, pm.sweep_column_times(fx.t0t1[k][0], fx.t0t1[k][1], W), xyz=fx.xyz[k], H=H)
        assert (nv, sk) == (len(fx.ref_xyz[k]), False)
    _same_map(m2, m3)


def test_resident_range_images_equal_the_fused_per_call_path(fx):
    from ptudes_lab_amd import core
    from tests.helpers import posed_map_numpy as pm
    b = core.BatchRunner(3, N, H * W, 0, max_range=fx.seq.max_range, min_range=fx.seq.min_range, with_ekf=False, range_input=True,
                         scan_cols=W, **CAPS)
    b.set_lut(fx.lut)
    for s in range(3):
        for k in range(N):
            b.upload_range(s, k, fx.scans[k].range_mm)
    m = _map_icp()
    n_valid, n_skipped = b.build_map(1, m, fx.traj, fx.t0t1)
    per_call = _map_icp()
    total = 0
    for k in range(N):
        nv, sk = per_call.map_add_posed(fx.traj, pm.sweep_column_times(fx.t0t1[k][0], fx.t0t1[k][1], W), range_mm=fx.scans[k].range_mm, lut=fx.lut)
        assert not sk
        total += nv
    assert (n_valid, n_skipped) == (total, 0) and total == sum(int(np.count_nonzero(s.range_mm)) for s in fx.scans)
    _same_map(m, per_call)


def _results_equal(a, b):
    assert set(a) == set(b)
    for key in a:
        if key == "stats":  # every field of every row, bit for bit (a NaN equals itself here)
            assert [[(k, np.float64(v).tobytes()) for k, v in row.items()] for row in a[key]] == \
                   [[(k, np.float64(v).tobytes()) for k, v in row.items()] for row in b[key]]
        else:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


def _imu(fx):
    n_imu = fx.seq.imu_range_for_scan(N - 1)[1]
    return n_imu, fx.seq.imu[:n_imu], [fx.seq.imu_range_for_scan(k)[1] for k in range(N)]


def test_seq_runner_is_untouched_by_a_map_build(fx):
    from ptudes_lab_amd import core
    n_imu, imu, ends = _imu(fx)
    outs = []
    for build in (False, True):
        r = core.SeqRunner(N, H * W, n_imu, max_range=fx.seq.max_range, min_range=fx.seq.min_range, use_imu_prediction=True, with_ekf=True,
                           scan_cols=W, **CAPS)
        for k in range(N):
            r.upload_scan(k, fx.xyz[k])
        r.upload_imu(imu, ends)
        r.run(3)
        if build:
            m = _map_icp()
            n_valid, n_skipped = r.build_map(m, fx.traj, fx.t0t1)
            assert n_skipped == 0 and n_valid == sum(len(p) for p in fx.ref_xyz) and m.map_size()[1] > 0
        r.advance(3)
        outs.append(r.results())
    assert len(outs[0]["res_t"]) == N
    _results_equal(outs[0], outs[1])


def test_batch_sequence_is_untouched_by_a_map_build(fx):
    from ptudes_lab_amd import core
    n_imu, imu, ends = _imu(fx)
    outs = []
    for build in (False, True):
        b = core.BatchRunner(2, N, H * W, n_imu, max_range=fx.seq.max_range, min_range=fx.seq.min_range, use_imu_prediction=True,
                             with_ekf=True, scan_cols=W, **CAPS)
        assert b.free_running
        for s in range(2):
            for k in range(N):
                b.upload_scan(s, k, fx.xyz[k])
            b.upload_imu(s, imu, ends)
        b.run(3)
        if build:
            m = _map_icp()
            assert b.build_map(1, m, fx.traj, fx.t0t1) == (sum(len(p) for p in fx.ref_xyz), 0)
        b.enqueue(3)
        b.wait()
        outs.append(b.results(1))
    assert len(outs[0]["res_t"]) == N
    _results_equal(outs[0], outs[1])


def _refused(code, fn):
    from ptudes_lab_amd import _lib
    with pytest.raises((RuntimeError, ValueError)) as e:
        fn()
    if code == -1:
        assert isinstance(e.value, ValueError)
    else:
        assert f"libptudes_mi error {code}:" in str(e.value), str(e.value)
    return str(e.value)


def test_refusals_and_skipping(fx):
    from ptudes_lab_amd import _lib, core
    r = _seq_runner(fx)
    full, first5 = _map_icp(), _map_icp()
    assert r.build_map(first5, fx.traj, fx.t0t1, last=4)[1] == 0
    # sweep times that put scan 5 beyond the bounds: skipped as a whole, the map is that of scans 0 .. 4
    late = fx.t0t1.copy()
    late[5] += (fx.knots[-1][0] - late[5][1]) + BOUNDS + 0.1
    n_valid, n_skipped = r.build_map(full, fx.traj, late)
    assert n_skipped == 1 and n_valid == sum(len(p) for p in fx.ref_xyz[:5])
    _same_map(full, first5)
    # ... and per call
    from tests.helpers import posed_map_numpy as pm
    ts = pm.sweep_column_times(fx.t0t1[0][0], fx.t0t1[0][1], W)
    ts[W // 2] = fx.knots[-1][0] + BOUNDS + 0.1  # one column
    before = full.map_size()
    assert full.map_add_posed(fx.traj, ts, xyz=fx.xyz[0], H=H) == (0, True) and full.map_size() == before

    def still_works():
        m = _map_icp()
        assert r.build_map(m, fx.traj, fx.t0t1, last=4)[1] == 0
        _same_map(m, first5)

    # a map handle with another scan_cols
    other = _map_icp(cols=W // 2)
    _refused(PTL_ERR_CAPACITY, lambda: r.build_map(other, fx.traj, fx.t0t1))
    _refused(PTL_ERR_CAPACITY, lambda: other.map_add_posed(fx.traj, ts, xyz=fx.xyz[0], H=H))
    assert other.map_size() == (0, 0)
    still_works()
    # a trajectory on another device: with one device the rule is tested through the handle's device_id (its first member, an int)
    t2 = core.Traj([k[0] for k in fx.knots], [k[1] for k in fx.knots], BOUNDS, BOUNDS)
    dev = C.c_int.from_address(t2._h.value)
    assert dev.value == 0
    dev.value = 1
    m = _map_icp()
    assert "device" in _refused(-1, lambda: r.build_map(m, t2, fx.t0t1))
    assert "device" in _refused(-1, lambda: m.map_add_posed(t2, ts, xyz=fx.xyz[0], H=H))
    dev.value = 0
    assert r.build_map(m, t2, fx.t0t1, last=4)[1] == 0
    _same_map(m, first5)
    # a batch with a sweep ring: its sweeps are gone
    ring = core.BatchRunner(1, N, H * W, 0, max_range=fx.seq.max_range, min_range=fx.seq.min_range, with_ekf=False, resident_scans=2,
                            scan_cols=W, **CAPS)
    assert "ring" in _refused(PTL_ERR_STATE, lambda: ring.build_map(0, m, fx.traj, fx.t0t1))
    # range images without a LUT
    rr = core.SeqRunner(N, H * W, 0, with_ekf=False, scan_cols=W, **CAPS)
    rr.upload_range(0, fx.scans[0].range_mm)
    assert "LUT" in _refused(PTL_ERR_STATE, lambda: rr.build_map(m, fx.traj, fx.t0t1, last=0))
    # the runner's own registration handle is no map container
    still_works()
    # the pool runs out: reported as map_add reports it, no hang
    small = _map_icp()
    _lib.check(_lib.lib().ptl_icp_debug_limit_capacity(small._h, 50, -1))
    msg = _refused(PTL_ERR_CAPACITY, lambda: r.build_map(small, fx.traj, fx.t0t1))
    ref = _map_icp()
    _lib.check(_lib.lib().ptl_icp_debug_limit_capacity(ref._h, 50, -1))
    assert _refused(PTL_ERR_CAPACITY, lambda: ref.map_add(fx.ref_xyz[0])) == msg
    still_works()


def test_commands_write_the_maps_they_print(fx, tmp_path):
    import re
    from click.testing import CliRunner
    from ptudes_lab_amd import fly, synth
    from ptudes_lab_amd import utils as pu
    from ptudes_lab_amd.cli.run import ptudes_cli
    p, m1, m2 = str(tmp_path / "p.csv"), str(tmp_path / "m.ply"), str(tmp_path / "m2.ply")
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "5", "--use-imu-prediction",
                                          "--save-nc-gt-poses", p, "--save-map", m1])
    assert res.exit_code == 0, res.output
    pts = pu.load_map_ply(m1)
    assert np.isfinite(pts).all() and len(pts) > 0
    assert int(re.search(r"(\d+) voxels, (\d+) points", res.output).group(2)) == len(pts)
    # = build_map in-process on the same sweeps with the rows of the poses file
    rows = pu.read_newer_college_gt(p)
    assert len(rows) == 6
    seq = synth.make_sequence(seed=1000, n_scans=6)
    from ptudes_lab_amd import core
    from ptudes_lab_amd.sequence import sweep_times
    r = core.SeqRunner(6, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    for k in range(6):
        r.upload_scan(k, seq.scan(k))
    m = core.Icp(1.0e9, 0.0, voxel_size=0.5, scan_cols=seq.W, max_points_per_scan=seq.H * seq.W, map_block_capacity=1 << 21,
                 map_table_capacity=1 << 23)
    traj = core.Traj([t for t, _ in rows], [q for _, q in rows], BOUNDS, BOUNDS)
    assert r.build_map(m, traj, sweep_times(seq))[1] == 0
    assert np.array_equal(_sorted(m.map_points()), _sorted(pts))
    # flyby on the same poses file = the three-call MapAccumulator driven from it with the same shift to the start scan
    res = CliRunner().invoke(ptudes_cli, ["flyby", "--synthetic", "1000", "--nc-gt-poses", p, "--end-scan", "5", "--save-map", m2])
    assert res.exit_code == 0, res.output
    got = pu.load_map_ply(m2)
    assert "map of scans: 0 - 5" in res.output and f"map num points: {len(got)}" in res.output and "0 skipped scans" in res.output
    pose0_inv = np.linalg.inv(rows[0][1])
    shifted = [(t, pose0_inv @ q) for t, q in rows]
    lut, scans = fly.synthetic_range_scans(seq)
    acc = fly.MapAccumulator(lut, voxel_size=0.5)
    for sc in pu.pose_scans_from_nc_gt(scans, nc_gt_poses=shifted):
        acc.update(sc)
    assert acc.scans == 6
    assert np.array_equal(_sorted(acc.map_points()), _sorted(got))
