"""The IMU deskew on the device: the filter's knots against its per-call state, the column table against the numpy
restatement (tests/helpers/imu_deskew_numpy.py), the whole pipeline against an oracle chain built here, every path and driver
against each other, nothing moves with the mode off, it deskews better than constant velocity, and the guards."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cpu as orc
from ptudes_lab_amd import core, synth
from tests.helpers import imu_deskew_numpy as dk

pytestmark = pytest.mark.gpu

W = 1024
KW = dict(max_range=70.0, min_range=1.0)


def _wobble(n, H=64, seed=2000):
    return synth.make_path_sequence(seed=seed, n_scans=n, H=H, W=W, step_m=1.0, wobble_deg=5.0, yaw_rate=0.5)


def _times(seq, n):
    k = np.arange(n)
    return np.stack([seq.t_base + k * seq.scan_dt, seq.t_base + (k + 1) * seq.scan_dt], axis=1)


def _imu_end(seq, n):
    return [seq.imu_range_for_scan(k)[1] for k in range(n)]


def _seq_runner(seq, n, imu_deskew=True, **kw):
    r = core.SeqRunner(n, seq.H * seq.W, _imu_end(seq, n)[-1], use_imu_prediction=True, imu_deskew=imu_deskew, **KW, **kw)
    for k in range(n):
        r.upload_scan(k, seq.scan(k))
    r.upload_imu(seq.imu[: _imu_end(seq, n)[-1]], _imu_end(seq, n))
    if imu_deskew:
        r.upload_sweep_times(_times(seq, n))
    return r


def test_knots_equal_the_filters_nav_after_each_sample():
    seq = _wobble(3, H=4)
    e = core.Ekf()
    e.enable_knots(64)
    exp = []
    for i, row in enumerate(seq.imu[:25]):
        e.process_imu(row[1:4], row[4:7], row[0])
        nav = e.nav
        exp.append(np.concatenate([[row[0]], nav[:3], nav[3:7]]))
        if i == 12:  # a pose update restarts the list with the state after it
            e.process_pose(seq.pose_at(row[0] - seq.t_base)[0])
            nav = e.nav
            exp = [np.concatenate([[e.ts], nav[:3], nav[3:7]])]
        kn, ovf = e.knots()
        assert not ovf and len(kn) == len(exp)
        assert np.abs(kn - np.array(exp)).max() < 1e-12
    # a sample that does not advance time adds no knot
    e.process_imu(seq.imu[24, 1:4], seq.imu[24, 4:7], seq.imu[24, 0])
    assert len(e.knots()[0]) == len(exp)


def test_column_table_equals_the_restatement():
    n = 6
    seq = _wobble(n)
    icp, e = core.Icp(**KW), core.Ekf()
    e.enable_knots(32)
    t = _times(seq, n)
    for k in range(n):
        a, b = seq.imu_range_for_scan(k)
        e.process_imu_batch(seq.imu[a:b])
        kn, _ = e.knots()
        core.icp_ekf_step(icp, e, [], seq.scan(k), use_imu_prediction=True, sweep=tuple(t[k]))
        mode, ref = dk.column_table(kn, t[k, 0], t[k, 1], W)
        assert mode == 2
        assert np.abs(icp.column_table() - ref).max() < 1e-12, k
    assert list(icp.deskew_modes()) == [2] * n


def test_column_table_through_a_full_turn(golden_dir):
    """knots from tests/golden/ekf_steps_turn.npz - its IMU samples (2.2 rad/s) and its measured poses, two of them 175 degrees off - so
    that the knots' attitudes take every case of the matrix-to-quaternion conversion (asserted).  The scans hold no valid point:
    every registration returns its guess, the filter's own pose, and its update moves no state; the fixture's pose follows it."""
    import os
    from tests.helpers.so3_cases import quat_case, quat_to_R
    g = np.load(os.path.join(golden_dir, "ekf_steps_turn.npz"))
    rows = np.c_[g["imu_ts"], g["imu_lacc"], g["imu_avel"]]
    icp, e = core.Icp(**KW), core.Ekf()
    e.enable_knots(32)
    scan = np.zeros((W, 3), dtype=np.float32)
    seen, start = [], 0
    for k, i in enumerate(int(i) for i in g["upd_idx"]):
        e.process_imu_batch(rows[start:i + 1])
        start = i + 1
        kn, ovf = e.knots()
        assert not ovf and len(kn) >= 10
        seen.append(quat_case(quat_to_R(kn[:, 4:8])))
        t0, t1 = kn[0, 0], kn[-1, 0]
        core.icp_ekf_step(icp, e, [], scan, use_imu_prediction=True, sweep=(t0, t1))
        mode, ref = dk.column_table(kn, t0, t1, W)
        assert mode == 2
        assert np.abs(icp.column_table() - ref).max() < 1e-12, k
        e.process_pose(g["upd_pose"][k])
    assert list(icp.deskew_modes()) == [2] * len(g["upd_idx"])
    assert (np.bincount(np.concatenate(seen), minlength=4) >= 20).all()


def _oracle_chain(seq, n):
    """oracle.cpu.EKF supplies the knots, the restatement deskews, oracle.cpu.ICP(deskew=0) registers, the EKF takes the KISS pose"""
    icp, ekf = orc.ICP(deskew=0, **KW), orc.EKF()
    t = _times(seq, n)
    kiss, res, modes = [], [], []
    knots = []
    for k in range(n):
        a, b = seq.imu_range_for_scan(k)
        for row in seq.imu[a:b]:
            ekf.process_imu(row[1:4], row[4:7], row[0])
            nav = ekf.nav
            if not knots or row[0] > knots[-1][0]:
                knots.append(np.concatenate([[row[0]], nav[:3], nav[3:7]]))
        mode, tab = dk.column_table(np.array(knots), t[k, 0], t[k, 1], W)
        modes.append(mode)
        x = seq.scan(k).astype(np.float64)
        pts = dk.deskew(x, tab, W) if mode == 2 else x
        pose = icp.register_frame(pts, None, ekf.pose_mat())
        kiss.append(pose)
        ekf.process_pose(pose)
        res.append(ekf.pose_mat())
        nav = ekf.nav
        knots = [np.concatenate([[ekf.ts], nav[:3], nav[3:7]])]
    return dict(kiss_poses=np.array(kiss), res_poses=np.array(res), stats=icp.stats, modes=modes)


def test_pipeline_matches_the_oracle_chain():
    n = 50
    seq = _wobble(n)
    ref = _oracle_chain(seq, n)
    r = _seq_runner(seq, n)
    r.run()
    out = r.results()
    assert list(r.deskew_modes()) == ref["modes"] and ref["modes"][0] == 2
    assert np.abs(out["kiss_poses"] - ref["kiss_poses"]).max() < 1e-9
    assert np.abs(out["res_poses"] - ref["res_poses"]).max() < 1e-9
    for a, b in zip(out["stats"], ref["stats"]):
        assert (a["iterations"], a["n_corr_last"], a["sum_cand"]) == (b["iterations"], b["n_corr_last"], b["sum_cand"])


BATCH_GEOM = dict(gn_workgroups=32, gn_lanes_per_point=8, gn_threads=512)  # a batch of <= 8 sequences runs each on 256 / 8 = 32 workgroups


def _batch(seqs, n, free_running, resident_scans=0, chunk=None):
    """a batch in IMU mode over `seqs`; resident_scans > 0: a sweep ring, sweeps uploaded `chunk` scans ahead of each launch"""
    b = core.BatchRunner(len(seqs), n, seqs[0].H * W, _imu_end(seqs[0], n)[-1], use_imu_prediction=True, free_running=free_running,
                         imu_deskew=True, resident_scans=resident_scans, **KW)
    for j, sq in enumerate(seqs):
        b.upload_imu(j, sq.imu[: _imu_end(sq, n)[-1]], _imu_end(sq, n))
        b.upload_sweep_times(j, _times(sq, n))
    if not resident_scans:
        for j, sq in enumerate(seqs):
            for k in range(n):
                b.upload_scan(j, k, sq.scan(k))
        b.run()
        return b
    for k0 in range(0, n, chunk):
        for j, sq in enumerate(seqs):
            for k in range(k0, k0 + chunk):
                b.upload_scan(j, k, sq.scan(k))
        b.enqueue(chunk)
        b.wait()
    return b


def _percall(seq, n, **icp_over):
    icp, e = core.Icp(**KW, **icp_over), core.Ekf()
    e.enable_knots(32)
    t = _times(seq, n)
    kp, rp = [], []
    for k in range(n):
        a, b = seq.imu_range_for_scan(k)
        kiss, pose, _ = core.icp_ekf_step(icp, e, seq.imu[a:b], seq.scan(k), use_imu_prediction=True, sweep=tuple(t[k]))
        kp.append(kiss)
        rp.append(pose)
    return np.array(kp), np.array(rp)


def test_every_path_gives_the_same_rows():
    n = 12
    seqs = [_wobble(n), _wobble(n, seed=2001)]
    # the sequence runner with a batch's geometry per sequence, and the per-call fused step with the same geometry
    singles = []
    for sq in seqs:
        r = _seq_runner(sq, n, **BATCH_GEOM)
        r.run()
        singles.append(r.results())
        assert list(r.deskew_modes()) == [2] * n
    kp, rp = _percall(seqs[0], n, **BATCH_GEOM)
    assert np.array_equal(kp, singles[0]["kiss_poses"]) and np.array_equal(rp, singles[0]["res_poses"])
    # batch: lockstep, free-running, free-running with a sweep ring - each against the sequence runner
    for b in (_batch(seqs, n, False), _batch(seqs, n, True), _batch(seqs, n, True, resident_scans=4, chunk=4)):
        for j in range(2):
            out = b.results(j)
            assert list(b.deskew_modes(j)) == [2] * n
            for key in ("kiss_poses", "res_poses", "res_t"):
                assert np.array_equal(out[key], singles[j][key]), (b.free_running, j, key)
            assert out["stats"] == singles[j]["stats"]


def test_mode_off_moves_nothing():
    n = 8
    seq = _wobble(n)
    a = _seq_runner(seq, n, imu_deskew=False)
    a.run()
    ra = a.results()
    b = _seq_runner(seq, n, imu_deskew=True)
    b.run()
    b.imu_deskew(False)
    b.run()
    rb = b.results()
    for key in ("kiss_poses", "res_poses", "res_t"):
        assert np.array_equal(ra[key], rb[key]), key
    assert list(b.deskew_modes()) == [0, 0] + [1] * (n - 2)
    # the knot list alone changes nothing the filter computes
    e1, e2 = core.Ekf(), core.Ekf()
    e2.enable_knots(300)
    for e in (e1, e2):
        e.process_imu_batch(seq.imu[:40])
        e.process_pose(seq.pose_at(seq.imu[39, 0] - seq.t_base)[0])
        e.process_imu_batch(seq.imu[40:80])
    assert np.array_equal(e1.nav, e2.nav) and np.array_equal(e1.cov, e2.cov)


def _rmse_aligned(P, G):
    """position RMSE of poses P against ground truth G expressed in P's frame: P_0 G_0^-1 G_k"""
    A = P[0] @ np.linalg.inv(G[0])
    d = P[:, :3, 3] - (A @ G)[:, :3, 3]
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


# Measured on the MI355X (tools/imu_deskew_cost.py, profiles/r07_imu_deskew_cost.json), this accelerating, yawing, fast-wobbling
# trajectory: KISS-pose position RMSE 0.761 m constant velocity, 0.041 m IMU (ratio 0.054).  (On the gentler wobbles the KISS-pose gain is
# small or negative - DESIGN.md 3.12.)
ACCURACY_MARGIN = 0.25


def test_it_deskews_better_than_constant_velocity():
    n = 40
    seq = synth.make_path_sequence(seed=2000, n_scans=n, H=64, W=W, step_m=0.5, ramp_sweeps=6, yaw_rate=1.0, wobble_deg=5.0, wobble_hz=2.5)
    cv = _seq_runner(seq, n, imu_deskew=False)
    cv.run()
    imu = _seq_runner(seq, n, imu_deskew=True)
    imu.run()
    rc, ri = cv.results(), imu.results()
    # each at its own reference instant: mid-sweep / the filter's time at the update
    e_cv = _rmse_aligned(rc["kiss_poses"], seq.gt_poses(0.5)[:n])
    e_imu = _rmse_aligned(ri["kiss_poses"], seq.pose_at(ri["res_t"] - seq.t_base))
    print(f"kiss-pose position RMSE: constant velocity {e_cv:.4f} m, IMU {e_imu:.4f} m, ratio {e_imu / e_cv:.3f}")
    assert e_imu < ACCURACY_MARGIN * e_cv


def test_guards_leave_handles_usable():
    n = 4
    seq = _wobble(n, H=16)
    ie = _imu_end(seq, n)
    with pytest.raises(RuntimeError):
        core.SeqRunner(n, seq.H * W, ie[-1], with_ekf=False, imu_deskew=True, **KW)
    r = core.SeqRunner(n, seq.H * W, ie[-1], use_imu_prediction=True, imu_deskew=True, **KW)
    for k in range(n):
        r.upload_scan(k, seq.scan(k))
    r.upload_imu(seq.imu[: ie[-1]], ie)
    with pytest.raises(RuntimeError, match="sweep times"):
        r.run()
    with pytest.raises(ValueError, match="knots"):
        r.imu_deskew(True, knot_capacity=5)
    r.imu_deskew(True)
    r.upload_sweep_times(_times(seq, n))
    r.run()
    assert list(r.deskew_modes()) == [2] * n
    # explicit per-point t01 and the fused step's capacity check
    icp, e = core.Icp(**KW), core.Ekf()
    with pytest.raises(RuntimeError, match="knot"):
        core.icp_ekf_step(icp, e, seq.imu[:10], seq.scan(0), sweep=(seq.t_base, seq.t_base + 0.1))
    e.enable_knots(4)
    with pytest.raises(ValueError):
        core.icp_ekf_step(icp, e, seq.imu[:10], seq.scan(0), sweep=(seq.t_base, seq.t_base + 0.1))
    with pytest.raises(ValueError):
        core.icp_ekf_step(icp, e, seq.imu[:3], seq.scan(0), t01=seq.column_times(), sweep=(seq.t_base, seq.t_base + 0.1))
    core.icp_ekf_step(icp, e, seq.imu[:3], seq.scan(0), sweep=(seq.t_base, seq.t_base + 0.1))
    # overflow: PTL_ERR_CAPACITY, not a quiet deskew with a truncated list
    e.process_imu_batch(seq.imu[3:9])
    assert e.knots()[1]
    with pytest.raises(RuntimeError, match="error -3"):
        core.icp_ekf_step(icp, e, [], seq.scan(1), sweep=(seq.t_base + 0.1, seq.t_base + 0.2))
    assert icp.deskew_modes()[-1] == 0
    # a constant-velocity step on the same handle is recorded as such
    core.icp_ekf_step(icp, e, seq.imu[9:12], seq.scan(2))
    assert list(icp.deskew_modes()) == [0, 0, 1]


def test_batch_guards_leave_the_batch_usable():
    n = 4
    seqs = [_wobble(n, H=16), _wobble(n, H=16, seed=2001)]
    ie = _imu_end(seqs[0], n)
    with pytest.raises(RuntimeError):
        core.BatchRunner(2, n, 16 * W, ie[-1], with_ekf=False, imu_deskew=True, **KW)
    b = core.BatchRunner(2, n, 16 * W, ie[-1], use_imu_prediction=True, imu_deskew=True, **KW)
    for j, sq in enumerate(seqs):
        for k in range(n):
            b.upload_scan(j, k, sq.scan(k))
        b.upload_imu(j, sq.imu[: ie[-1]], ie)
    b.upload_sweep_times(0, _times(seqs[0], n))
    with pytest.raises(RuntimeError, match="sweep times"):
        b.run()
    b.upload_sweep_times(1, _times(seqs[1], n))
    with pytest.raises(ValueError, match="knots"):
        b.imu_deskew(True, knot_capacity=5)
    b.imu_deskew(True)
    for j, sq in enumerate(seqs):
        b.upload_sweep_times(j, _times(sq, n))
    b.run()
    assert [list(b.deskew_modes(j)) for j in range(2)] == [[2] * n] * 2


def test_resident_events_and_cli(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    from ptudes_lab_amd.sequence import run_events, run_resident, sweep_times, synthetic_events
    n = 6
    seq = _wobble(n)
    res = run_resident(seq, n, use_imu_prediction=True, imu_deskew=True)
    assert list(res["deskew_modes"]) == [2] * n
    meta = SimpleNamespace(format=SimpleNamespace(columns_per_frame=seq.W, pixels_per_column=seq.H), prod_line="SYNTH", mode="1024x10")
    t = sweep_times(seq, n)
    ev = run_events(iter(list(synthetic_events(seq, n))), meta, use_imu_prediction=True, imu_deskew=True,
                    sweep_time_fn=lambda ts: (ts - seq.scan_dt, ts))
    # the fused per-call loop on the same sweeps: same filter, same tables as the resident runner's (same geometry)
    assert np.abs(np.array(ev["res_poses"]) - res["res_poses"]).max() < 1e-6
    assert np.abs(np.array(ev["res_t"]) - (t[:, 1] - 0.01)).max() < 1e-6
    with pytest.raises(ValueError, match="fused"):
        run_events(iter([]), meta, imu_deskew=True, fused=False, sweep_time_fn=lambda ts: (ts - 0.1, ts))
    # CLI
    out_csv = str(tmp_path / "poses.csv")
    r = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "10", "--use-imu-prediction",
                                        "--imu-deskew", "--save-nc-gt-poses", out_csv])
    assert r.exit_code == 0, r.output
    assert len(np.loadtxt(out_csv, delimiter=",", comments="#", ndmin=2)) == 11
    r = CliRunner().invoke(ptudes_cli, ["ekf-bench", "ouster", "--imu-deskew", "nofile.pcap"])
    assert r.exit_code != 0 and "--synthetic" in r.output
