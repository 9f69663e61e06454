"""The fixed-interval RTS smoother on the device: the filter's history log (inside d_ekf_step) against the per-call state and
the CPU oracle, the backward pass (k_ekf_smooth) against the numpy restatement (tests/helpers/rts_numpy.py), its invariants,
that nothing the filter computes moves with the log on, that every path gives the same smoothed rows, that it smooths, the
guards, and the CLI."""
from types import SimpleNamespace

import numpy as np
import numpy.random as npr
import pytest

from ptudes_lab_amd import _lib as L
from ptudes_lab_amd import core, synth
from ptudes_lab_amd.sequence import run_events, run_resident, synthetic_events
from tests.helpers import rts_numpy as rn

pytestmark = pytest.mark.gpu

TOL_POS, TOL_ROT, TOL_COV = 1e-9, 1e-9, 1e-8


def _sim_stream(duration=2.0, corr_t=0.1, seed=0):
    """the `ekf-bench sim` stream: (ideal, noisy) IMU pairs, a GT filter's pose as the correction every corr_t"""
    from ptudes_lab_amd.cli.ekf_bench import sim_imu
    npr.seed(seed)
    out = []
    for a, b in sim_imu(freq=100.0, acc_noise_std=0.4, gyr_noise_std=0.4):
        out.append((a, b))
        if a.ts > duration + 0.02:
            break
    return out


def _run_sim(ekf, ekf_gt=None, corr_t=0.1, duration=2.0, hook=None):
    """the sim loop (cli/ekf_bench.py ptudes_ekf_sim) on core.Ekf handles; returns the update epochs' (gt pose, filtered pose)"""
    ekf_gt = ekf_gt or core.Ekf()
    start = last = None
    gts, filt = [], []
    for a, b in _sim_stream(duration):
        ts = a.ts
        if start is None:
            start = last = ts
        ekf_gt.process_imu(a.lacc, a.avel, ts)
        if hook:
            hook("imu", b)
        ekf.process_imu(b.lacc, b.avel, ts)
        if ts - last > corr_t:
            g = ekf_gt.pose_mat()
            if hook:
                hook("pre", g)
            ekf.process_pose(g)
            if hook:
                hook("post", g)
            gts.append(g)
            filt.append(ekf.pose_mat())
            last = ts
        if ts - start > duration:
            break
    return np.array(gts), np.array(filt)


def _fx(nav, row, ts_prev):
    """Fx of one active IMU sample, rebuilt from the nav state before it (es_ekf.py:216-223)"""
    dt = row[0] - ts_prev
    Rp = rn.quat_to_R(nav[3:7])
    a = row[1:4] - nav[13:16]
    Rd = rn.exp_so3((row[4:7] - nav[10:13]) * dt)
    F = np.eye(18)
    F[0:3, 3:6] = dt * np.eye(3)
    F[3:6, 6:9] = -dt * Rp @ rn.skew(a)
    F[3:6, 12:15] = -dt * Rp
    F[6:9, 6:9] = Rd.T
    F[6:9, 9:12] = -dt * np.eye(3)
    return F


def _check_smoothed(log, sm, label=""):
    """GPU smoothed rows against rts_numpy on the downloaded log + the invariants"""
    ref = rn.rts(log)
    n = len(log["ts"])
    assert len(sm["poses"]) == n and n > 1, label
    assert np.array_equal(sm["t"], log["ts"]), label
    for k in ("poses", "nav", "cov"):
        assert np.isfinite(sm[k]).all(), (label, k)
    dp = np.abs(sm["nav"][:, 0:3] - ref["nav"][:, 0:3]).max()
    dr = max(np.linalg.norm(rn.log_so3(rn.quat_to_R(a[3:7]).T @ rn.quat_to_R(b[3:7]))) for a, b in zip(sm["nav"], ref["nav"]))
    dpose = np.abs(sm["poses"][:, :3, 3] - ref["poses"][:, :3, 3]).max()
    drest = np.abs(sm["nav"][:, 7:] - ref["nav"][:, 7:]).max()
    dc = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(sm["cov"], ref["cov"]))
    cond = max(np.linalg.cond(P) for P in log["P_pred"])
    msg = f"{label}: |dpos| {dp:.2e} |drot| {dr:.2e} |dcov|rel {dc:.2e} |dnav rest| {drest:.2e}, max cond(P_pred) {cond:.2e}"
    assert dp <= TOL_POS and dpose <= TOL_POS and dr <= TOL_ROT and dc <= TOL_COV and drest <= 1e-8, msg
    # invariants: the last row is the filter's own, the smoother never loses information, P^s is a covariance (symmetrised
    # exactly - except the last row, which is the filter's P_{N|N} bit for bit, and the filter does not symmetrise its P)
    assert np.array_equal(sm["nav"][-1], log["nav_post"][-1]) and np.array_equal(sm["cov"][-1], log["P_post"][-1]), label
    for k in range(n):
        assert np.trace(sm["cov"][k]) <= np.trace(log["P_post"][k]) * (1 + 1e-12), (label, k)
        if k < n - 1:
            assert np.array_equal(sm["cov"][k], sm["cov"][k].T), (label, k)
        assert np.linalg.eigvalsh(sm["cov"][k]).min() >= -1e-12, (label, k)
    return ref


# ------------------------------------------------------------------------------------------------ 3: log fidelity (per-call)
def test_log_fidelity_per_call_against_state_oracle_and_rebuilt_phi():
    from oracle import cpu as orc
    e, o = core.Ekf(), orc.EKF()
    e.enable_smoother(64)
    pre, post = [], []
    cur = {"phi": np.eye(18), "ts": None, "phis": []}

    def hook(kind, x):
        if kind == "imu":
            nav, _ = e.state()
            if cur["ts"] is not None:  # the first sample only latches
                cur["phi"] = _fx(nav, np.array([x.ts, *x.lacc, *x.avel]), cur["ts"]) @ cur["phi"]
            cur["ts"] = x.ts
            o.process_imu(x.lacc, x.avel, x.ts)
        elif kind == "pre":
            pre.append(e.state() + (o.nav, o.cov))
            cur["phis"].append(cur["phi"])
            cur["phi"] = np.eye(18)
        else:
            o.process_pose(x)
            post.append(e.state() + (o.nav, o.cov))

    _run_sim(e, hook=hook)
    log = e.smoother_log()
    n = len(log["ts"])
    assert n == len(pre) == len(post) > 10 and not log["overflow"]
    for k in range(n):
        assert np.array_equal(log["nav_pred"][k], pre[k][0]) and np.array_equal(log["P_pred"][k], pre[k][1]), k
        assert np.array_equal(log["nav_post"][k], post[k][0]) and np.array_equal(log["P_post"][k], post[k][1]), k
        assert np.abs(log["nav_pred"][k] - pre[k][2]).max() < 1e-9 and np.abs(log["P_pred"][k] - pre[k][3]).max() < 1e-9, k
        assert np.abs(log["nav_post"][k] - post[k][2]).max() < 1e-9 and np.abs(log["P_post"][k] - post[k][3]).max() < 1e-9, k
        assert np.abs(log["Phi"][k] - cur["phis"][k]).max() < 1e-12, k
    assert log["ts"][-1] == e.ts


# ------------------------------------------------------------------------------------------------ 4 / 5 / 8: sim stream
def test_sim_stream_smoother_arithmetic_invariants_and_it_smooths():
    e = core.Ekf()
    e.enable_smoother(64)
    gts, filt = _run_sim(e)
    log = e.smoother_log()
    sm = e.smooth()
    _check_smoothed(log, sm, "sim")
    assert np.array_equal(sm["poses"][-1], filt[-1])
    # at the update epochs, against the GT filter's poses
    f_err = np.sqrt(np.mean(np.sum((filt[:, :3, 3] - gts[:, :3, 3]) ** 2, axis=1)))
    s_err = np.sqrt(np.mean(np.sum((sm["poses"][:, :3, 3] - gts[:, :3, 3]) ** 2, axis=1)))
    assert s_err < f_err, (s_err, f_err)


def test_turn_stream_smoother_arithmetic_and_invariants(golden_dir):
    """tests/golden/ekf_steps_turn.npz (the attitude passes through all of SO(3), two updates 175 degrees off): the backward pass takes
    R_to_rotvec / rotvec_to_R of attitudes in every case of R_to_quat - against the restatement at the sim stream's tolerances"""
    import os
    from tests.helpers.so3_cases import quat_case, quat_to_R
    g = np.load(os.path.join(golden_dir, "ekf_steps_turn.npz"))
    e = core.Ekf()
    e.enable_smoother(64)
    upd = {int(i): k for k, i in enumerate(g["upd_idx"])}
    for i in range(len(g["imu_ts"])):
        e.process_imu(g["imu_lacc"][i], g["imu_avel"][i], g["imu_ts"][i])
        if i in upd:
            e.process_pose(g["upd_pose"][upd[i]])
    log = e.smoother_log()
    assert len(log["ts"]) == len(upd) and not log["overflow"]
    assert np.abs(log["nav_post"][:, :3] - g["nav_after_upd"][:, :3]).max() <= 1e-9
    assert len(set(quat_case(quat_to_R(log["nav_post"][:, 3:7])))) == 4  # the smoothed epochs themselves take all four cases
    sm = e.smooth()
    _check_smoothed(log, sm, "turn")


def _resident(seq, n, use_imu, smooth=True, plain=False, **kw):
    """a SeqRunner over seq (plain: configured like one sequence of a BatchRunner, tests/test_gpu_batch.py)"""
    n_imu = seq.imu_range_for_scan(n - 1)[1]
    if not plain:
        kw.update(max_range=seq.max_range, min_range=seq.min_range, scan_cols=seq.W)
    r = core.SeqRunner(n, seq.H * seq.W, n_imu, use_imu_prediction=use_imu, with_ekf=True, **kw)
    for k in range(n):
        r.upload_scan(k, seq.scan(k))
    r.upload_imu(seq.imu[:n_imu], [seq.imu_range_for_scan(k)[1] for k in range(n)])
    if smooth:
        r.enable_smoother(True)
    return r


@pytest.mark.parametrize("use_imu", [True, False])
def test_ouster_sequence_smoother_arithmetic_and_nothing_else_moves(use_imu):
    n = 100
    seq = synth.make_sequence(seed=1900, n_scans=n)
    on, off = _resident(seq, n, use_imu), _resident(seq, n, use_imu, smooth=False)
    on.run()
    off.run()
    a, b = on.results(), off.results()
    for k in ("res_poses", "res_t", "kiss_poses"):
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"]
    log = on.smoother_log()
    assert len(log["ts"]) == len(a["res_t"]) == n
    assert np.array_equal(log["ts"], a["res_t"])
    sm = on.smooth()
    _check_smoothed(log, sm, f"ouster use_imu={use_imu}")
    assert np.array_equal(sm["poses"][-1], a["res_poses"][-1])


# ------------------------------------------------------------------------------------------------ 6 / 7: every path
def _batch(seqs, n, **kw):
    n_imu = seqs[0].imu_range_for_scan(n - 1)[1]
    b = core.BatchRunner(len(seqs), n, seqs[0].H * seqs[0].W, n_imu, use_imu_prediction=True, with_ekf=True, **kw)
    return b, n_imu


def _upload(b, seqs, n, n_imu, upto=None):
    for s, sq in enumerate(seqs):
        for k in range(n if upto is None else upto):
            b.upload_scan(s, k, sq.scan(k))
        b.upload_imu(s, sq.imu[:n_imu], [sq.imu_range_for_scan(k)[1] for k in range(n)])


@pytest.mark.parametrize("driver", ["free", "lockstep"])
def test_batch_smoothed_rows_equal_seq_runner_and_fused_loop_and_forward_outputs_do_not_move(driver):
    n, S = 12, 3
    seqs = [synth.make_sequence(seed=1950 + s, n_scans=n) for s in range(S)]
    b, n_imu = _batch(seqs, n, free_running=driver == "free")
    b_off, _ = _batch(seqs, n, free_running=driver == "free")
    _upload(b, seqs, n, n_imu)
    _upload(b_off, seqs, n, n_imu)
    b.enable_smoother(True)
    b.run(5)        # cold start + 5 scans ...
    b.enqueue(n - 5)  # ... the log continues
    b.wait()
    b_off.run()
    b.smooth()
    for s in range(S):
        x, y = b.results(s), b_off.results(s)
        for k in ("res_poses", "res_t", "kiss_poses"):
            assert np.array_equal(x[k], y[k]), (s, k)
        assert x["stats"] == y["stats"]
    # sequence 0 alone (the batch's workgroups per sequence), and the fused per-call loop
    r = _resident(seqs[0], n, True, plain=True, gn_workgroups=32, gn_lanes_per_point=8, gn_threads=512)
    r.run()
    assert np.array_equal(r.results()["res_poses"], b.results(0)["res_poses"])
    sm_r, sm_b = r.smooth(), b.smoothed(0)
    for k in ("t", "poses", "nav", "cov"):
        assert np.array_equal(sm_r[k], sm_b[k]), k
    _check_smoothed(b.smoother_log(0), sm_b, f"batch {driver}")
    if driver == "free":
        sq = seqs[0]
        meta = SimpleNamespace(format=SimpleNamespace(columns_per_frame=sq.W, pixels_per_column=sq.H))
        ev = run_events(iter(list(synthetic_events(sq, n))), meta, use_imu_prediction=True, fused=True, smooth=True)
        rr = run_resident(sq, n, use_imu_prediction=True, map_table_capacity=1 << 22, smooth=True)
        assert np.array_equal(np.array(ev["res_poses"]), rr["res_poses"])  # (tests/test_gpu_dropin.py: the forward runs agree)
        assert np.array_equal(ev["smoothed_poses"], rr["smoothed_poses"])
        assert np.array_equal(ev["smoothed_t"], rr["smoothed_t"])
    # one run equals the split run
    b.run()
    b.smooth()
    for s in range(S):
        one = b.smoothed(s)
        assert np.array_equal(one["poses"], b_split_rows(seqs, n, driver, s)), s


_SPLIT = {}


def b_split_rows(seqs, n, driver, s):
    """smoothed poses of sequence s from a batch run split as run(4) + enqueue(rest) (cached per driver)"""
    if driver not in _SPLIT:
        b, n_imu = _batch(seqs, n, free_running=driver == "free")
        _upload(b, seqs, n, n_imu)
        b.enable_smoother(True)
        b.run(4)
        b.enqueue(n - 4)
        b.wait()
        b.smooth()
        _SPLIT[driver] = [b.smoothed(q, nav=False, cov=False)["poses"] for q in range(len(seqs))]
    return _SPLIT[driver][s]


def test_sweep_ring_batch_smooths_like_a_resident_one():
    n, S, R = 12, 2, 4
    seqs = [synth.make_sequence(seed=1970 + s, n_scans=n) for s in range(S)]
    res, n_imu = _batch(seqs, n)
    _upload(res, seqs, n, n_imu)
    res.enable_smoother(True)
    res.run()
    res.smooth()
    ring, _ = _batch(seqs, n, resident_scans=R)
    _upload(ring, seqs, n, n_imu, upto=R)
    ring.enable_smoother(True)
    L.check(L.lib().ptl_batch_reset(ring._h))
    for k0 in range(0, n, R - 1):
        m = min(R - 1, n - k0)
        for s, sq in enumerate(seqs):
            for k in range(max(k0, R), min(k0 + m, n)):
                ring.upload_scan(s, k, sq.scan(k))
        ring.enqueue(m)
        ring.wait()
    ring.smooth()
    for s in range(S):
        a, b = res.smoothed(s), ring.smoothed(s)
        for k in ("t", "poses", "nav", "cov"):
            assert np.array_equal(a[k], b[k]), (s, k)


# ------------------------------------------------------------------------------------------------ 8: a jitter sequence
def _kabsch_rmse(P, Q):
    """position RMSE of P against Q after the best rigid alignment"""
    mp, mq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((P - mp).T @ (Q - mq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    Rm = Vt.T @ D @ U.T
    return float(np.sqrt(np.mean(np.sum(((P - mp) @ Rm.T - (Q - mq)) ** 2, axis=1))))


def test_jitter_sequence_smoothed_rmse_not_above_filtered():
    n = 60
    seq = synth.make_sequence(seed=1990, n_scans=n, ray_jitter_deg=0.05)
    r = _resident(seq, n, True)
    r.run()
    out = r.results()
    sm = r.smooth(nav=False, cov=False)
    gt = seq.pose_at(out["res_t"] - seq.t_base)[:, :3, 3]
    f = _kabsch_rmse(out["res_poses"][:, :3, 3], gt)
    s = _kabsch_rmse(sm["poses"][:, :3, 3], gt)
    assert s <= f, (s, f)


# ------------------------------------------------------------------------------------------------ 9: guards
def test_guards_leave_the_handles_usable():
    e = core.Ekf()
    with pytest.raises(RuntimeError, match="not enabled"):
        e.smooth()
    e.enable_smoother(5)
    _run_sim(e, duration=1.05)  # 10 updates
    log = e.smoother_log()
    assert log["overflow"] and len(log["ts"]) == 5
    with pytest.raises(RuntimeError, match="error -3"):
        e.smooth()
    e.enable_smoother(32)  # a fresh log: the same handle runs on and smooths
    _run_sim(e, duration=1.05)
    log = e.smoother_log()
    assert not log["overflow"] and len(log["ts"]) >= 9
    _check_smoothed(log, e.smooth(), "after overflow")
    # a sequence runner: smoothing without the log, then with it
    n = 6
    seq = synth.make_sequence(seed=1995, n_scans=n)
    r = _resident(seq, n, True, smooth=False)
    r.run()
    with pytest.raises(RuntimeError, match="error -4"):
        r.smooth()
    r.enable_smoother(True)
    r.run()
    assert len(r.smooth()["poses"]) == n
    # ICP-only: refused, and the runner still runs
    ic = core.SeqRunner(n, seq.H * seq.W, 0, with_ekf=False, scan_cols=seq.W)
    for k in range(n):
        ic.upload_scan(k, seq.scan(k))
    ic.upload_imu(np.zeros((0, 7)), [0] * n)
    with pytest.raises(RuntimeError, match="error -4"):
        ic.enable_smoother(True)
    ic.run()
    assert len(ic.results()["kiss_poses"]) == n
    b, n_imu = _batch([seq], n)
    _upload(b, [seq], n, n_imu)
    b.run()
    with pytest.raises(RuntimeError, match="error -4"):
        b.smooth()


# ------------------------------------------------------------------------------------------------ 10: CLI
def test_ouster_cli_save_smoothed_poses(tmp_path):
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    a, b = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    base = ["ekf-bench", "ouster", "--synthetic", "1000", "--end-scan", "50", "--use-imu-prediction", "--save-nc-gt-poses", a]
    r0 = CliRunner().invoke(ptudes_cli, base)
    assert r0.exit_code == 0, r0.output
    r1 = CliRunner().invoke(ptudes_cli, base + ["--save-smoothed-poses", b])
    assert r1.exit_code == 0, r1.output
    ta = np.loadtxt(a, delimiter=",", comments="#", ndmin=2)
    tb = np.loadtxt(b, delimiter=",", comments="#", ndmin=2)
    assert ta.shape == tb.shape and len(ta) == 51
    assert np.array_equal(ta[:, :2], tb[:, :2])  # the timestamp columns
    assert not np.array_equal(ta[:, 2:], tb[:, 2:])

    def strip(s):  # run-dependent lines: the output time stamp and the timings
        return [ln for ln in s.splitlines() if not ln.startswith(("time:", "  ESEKF", "  KissICP", "  Stats"))]
    assert strip(r0.output) == strip(r1.output)


def test_sim_cli_smooth_prints_both_ates():
    from click.testing import CliRunner
    from ptudes_lab_amd.cli.run import ptudes_cli
    npr.seed(0)  # (sim_imu draws from the global RNG)
    res = CliRunner().invoke(ptudes_cli, ["ekf-bench", "sim", "-t", "2.0", "--smooth"])
    assert res.exit_code == 0, res.output
    lines = [ln for ln in res.output.splitlines() if ln.startswith("RMSE at the")]
    assert len(lines) == 2 and "(filtered)" in lines[0] and "(RTS smoothed)" in lines[1]
    f, s = (float(ln.split("trans ")[1].split()[0]) for ln in lines)
    assert s < f, res.output
