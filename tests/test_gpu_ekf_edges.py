"""The device's error-state filter on the edge streams of tests/helpers/ekf_edge_streams.py (irregular IMU timing and batch
lengths across the 64-sample chunks, row swaps at every pivot column of the 6x6 inverse, stiff measurement covariances, huge and
vanishing innovations, a 20 000-sample run), against the longdouble restatement tests/helpers/ekf_longdouble.py.  DESIGN.md 3.15.2.

Tolerance, per stream and quantity, in the same process: e_dev <= 4 * e_orc + floor, e_dev = device against restatement, e_orc = C
oracle against restatement, floor = the oracle's error on the reference's own goldens.  Nothing is taken from the device's output.
"""
import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from ptudes_lab_amd import core, synth
from tests.helpers import ekf_edge_streams as es
from tests.helpers import ekf_longdouble as eld

pytestmark = pytest.mark.gpu


def _ratio(a, b):
    return a / b if b > 0 else float("inf") if a > 0 else 1.0


def _expected_knots(events):
    """the knot rule restated on the host, as the knots' times: before the first update a knot after the first sample, then after
    every sample whose ts exceeds the last knot's; an update restarts the list with one knot at the current time"""
    ts, cur = [], 0.0
    for e in events:
        if e[0] == "imu":
            cur = float(e[1][0])
            if not ts or cur > ts[-1]:
                ts.append(cur)
        else:
            ts = [cur]
    return ts


def feed_stream(name):
    """both feeders over stream `name` -> {event index: (nav, P)} of the batch-fed handle at the checkpoints.  On `irregular` the two
    handles must hold the same bits after every run and every update, and the knot list must follow the rule."""
    s = es.stream(name)
    ck = set(es.checkpoints(name, s.events))
    bits = name == "irregular"
    one, bat = core.Ekf(), core.Ekf()
    if bits:
        bat.enable_knots(2048)
        one.enable_knots(2048)
    out, run = {}, []

    def flush():
        if run:
            bat.process_imu_batch(np.array(run))
            run.clear()

    for i, e in enumerate(s.events):
        if e[0] == "imu":
            one.process_imu(e[1][1:4], e[1][4:7], e[1][0])
            run.append(e[1])
            if i + 1 < len(s.events) and s.events[i + 1][0] == "imu":
                continue
            flush()
        else:
            flush()
            for h in (one, bat):
                h.process_pose(e[1], e[2])
        if i in ck:
            out[i] = bat.state()
            if bits:
                n1, c1 = one.state()
                assert np.array_equal(n1, out[i][0]) and np.array_equal(c1, out[i][1]), (name, i, e[0])
                assert one.ts == bat.ts
        if bits and (e[0] == "pose" or i + 1 == len(s.events) or s.events[i + 1][0] == "pose"):
            want = _expected_knots(s.events[:i + 1])
            for h in (one, bat):
                kn, ovf = h.knots()
                assert not ovf and list(kn[:, 0]) == want, (name, i, len(kn), len(want))
            assert np.array_equal(one.knots()[0], bat.knots()[0])
            if e[0] == "pose":  # the restarted list's one knot is the state right after the update
                assert np.array_equal(kn[0, 1:4], out[i][0][:3]) and np.array_equal(kn[0, 4:8], out[i][0][3:7])
    if name != "irregular":  # the other streams: the two feeders agree at the end
        (n1, c1), (nb, cb) = one.state(), bat.state()
        assert np.array_equal(n1, nb) and np.array_equal(c1, cb), name
    return out


@pytest.mark.parametrize("name", es.STREAMS)
def test_ekf_handle_on_edge_stream(name):
    got = feed_stream(name)
    ref = es.restatement(name)[0]
    assert sorted(got) == sorted(ref)
    assert all(np.isfinite(v[0]).all() and np.isfinite(v[1]).all() for v in got.values())
    e_dev, e_orc, floor = es.errors(got, ref), es.oracle_errors(name), es.golden_floor()
    for q in range(2):
        print(f"{name} {('nav', 'cov')[q]}: e_dev {e_dev[q]:.3g} e_orc {e_orc[q]:.3g} ratio {_ratio(e_dev[q], e_orc[q]):.3g} floor {floor[q]:.3g}")
    for q in range(2):
        assert es.within(e_dev[q], e_orc[q], floor[q]), (name, ("nav", "cov")[q], e_dev[q], e_orc[q], floor[q])


# ------------------------------------------------------------------------------------------------ the runners' filter paths
ROWS = ("res_poses", "res_t", "kiss_poses")
LOG = ("ts", "nav_pred", "P_pred", "Phi", "nav_post", "P_post")


def _run_runners():
    """SeqRunner, lockstep BatchRunner and free-running BatchRunner over the same 9 sweeps and the `irregular` IMU rows split
    5, 1, 1, 63, 64, 65, 129, 2, 128 -> per runner (results, smoother log) of sequence 0 (and of sequence 1 for the batches)"""
    n, H, W = 9, 32, 256
    seqs = [synth.make_sequence(seed=31, n_scans=n, H=H, W=W), synth.make_sequence(seed=32, n_scans=n, H=H, W=W)]
    scans = [[sq.scan(k) for k in range(n)] for sq in seqs]
    rows, end = es.runner_imu()
    out = {}
    r = core.SeqRunner(n, H * W, len(rows), use_imu_prediction=False, with_ekf=True, scan_cols=W,
                       gn_workgroups=32, gn_lanes_per_point=8, gn_threads=512)
    for k in range(n):
        r.upload_scan(k, scans[0][k])
    r.upload_imu(rows, end)
    r.enable_smoother(True)
    r.run()
    out["seq"] = [(r.results(), r.smoother_log())]
    r.close()
    for free in (False, True):
        b = core.BatchRunner(2, n, H * W, len(rows), use_imu_prediction=False, with_ekf=True, scan_cols=W, free_running=free)
        assert b.free_running == free
        for s in range(2):
            for k in range(n):
                b.upload_scan(s, k, scans[s][k])
            b.upload_imu(s, rows, end)
        b.enable_smoother(True)
        b.run()
        out["free" if free else "lockstep"] = [(b.results(s), b.smoother_log(s)) for s in range(2)]
        b.close()
    return out, rows, end


def test_batched_runner_refuses_an_empty_imu_interval():
    """why the runner test's second run length is 1 and not 0: the batched runner answers an empty interval with an error status
    (the sequence runner skips such a scan, as the reference's driver loop does)"""
    b = core.BatchRunner(2, 3, 1024, 4, with_ekf=True, max_points_per_scan=1024, scan_cols=64)
    with pytest.raises(Exception, match="at least one IMU sample"):
        b.upload_imu(0, np.zeros((4, 7)), [2, 2, 4])
    b.close()


def test_runners_filter_paths_on_irregular_imu_rows():
    out, rows, end = _run_runners()
    res, log = out["seq"][0]
    assert len(res["res_t"]) == len(log["ts"]) == 9 and not log["overflow"]
    # the three runners: the same bits for the same sequence
    for name in ("lockstep", "free"):
        r2, l2 = out[name][0]
        for k in ROWS:
            assert np.array_equal(res[k], r2[k]), (name, k)
        for k in LOG:
            assert np.array_equal(log[k], l2[k]), (name, k)
    (r1, l1), (r2, l2) = out["lockstep"][1], out["free"][1]  # ... and for the batches' second sequence
    for k in ROWS:
        assert np.array_equal(r1[k], r2[k]), k
    for k in LOG:
        assert np.array_equal(l1[k], l2[k]), k
    assert not np.array_equal(out["free"][0][0]["res_poses"], out["free"][1][0]["res_poses"])
    # against the restatement, over the run's own registration poses
    floor = es.golden_floor()
    for s, (res, log) in enumerate(out["free"]):
        ref = es.runner_replay(eld.EkfLD(), rows, end, res["kiss_poses"])
        orc = es.runner_replay(es._PhiTracker(), rows, end, res["kiss_poses"])
        assert np.array_equal(res["res_t"], ref["res_t"]) and np.array_equal(log["ts"], ref["res_t"])
        got = dict(log, res_poses=res["res_poses"])
        assert all(np.isfinite(got[k]).all() for k in got if k != "overflow")
        e_dev, e_orc = es.runner_errors(got, ref), es.runner_errors(orc, ref)
        for q, nm in enumerate(("nav", "cov", "Phi")):
            print(f"runner sequence {s} {nm}: e_dev {e_dev[q]:.3g} e_orc {e_orc[q]:.3g} ratio {_ratio(e_dev[q], e_orc[q]):.3g} floor {floor[q]:.3g}")
        for q, nm in enumerate(("nav", "cov", "Phi")):
            assert es.within(e_dev[q], e_orc[q], floor[q]), (s, nm, e_dev[q], e_orc[q], floor[q])
