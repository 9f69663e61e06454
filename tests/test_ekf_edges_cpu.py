"""The edge streams of the error-state filter (tests/helpers/ekf_edge_streams.py) do what they claim, on the longdouble
restatement alone; and the C oracle against the restatement on every stream.  No GPU.  DESIGN.md 3.15.2."""
import numpy as np
import pytest

from tests.helpers import ekf_edge_streams as es
from tests.helpers import ekf_longdouble as eld

TOL = 1e-9  # SURVEY.md 8(d), the tolerance the reference's own goldens are held to everywhere else


def _reports(name):
    return es.restatement(name)[1].reports


def test_restatement_is_wider_than_fp64_and_its_so3_maps_invert_each_other():
    assert np.finfo(eld.LD).eps <= 2.0 ** -63
    rng = np.random.default_rng(5)
    for s in (1e-9, 1e-5, 0.99e-4, 1.01e-4, 0.3, 2.0, 3.1):  # both sides of the series threshold, and near pi
        v = eld.ld(rng.normal(size=3))
        v = v / np.sqrt(v @ v) * eld.LD(s)
        R = eld.exp_so3(v)
        assert float(np.abs(R @ R.T - np.eye(3)).max()) <= 8 * np.finfo(eld.LD).eps
        assert float(np.abs(eld.log_so3(R) - v).max()) <= 64 * np.finfo(eld.LD).eps * max(1.0, 1.0 / (np.pi - s))
    A = eld.ld(rng.normal(size=(6, 6)))
    Ai, rep = eld.inv_gauss_jordan(A)
    assert float(np.abs(Ai @ A - np.eye(6)).max()) <= 1e-15 * rep["cond"]
    assert eld.inv_gauss_jordan(np.diag(eld.ld([3, 1, 2, 5, 4, 6])))[1]["zero_factors"] == 30


@pytest.mark.parametrize("variant", ["default", "init", "cov", "turn", "inverted", "sim"])
def test_restatement_reproduces_the_reference_goldens(variant):
    nav, cov = es.golden_replays()[variant]["golden"]
    print(f"{variant}: restatement against the golden nav {nav:.3g} cov {cov:.3g}")
    assert nav <= TOL and cov <= TOL


def test_floor_is_the_oracles_error_on_the_goldens():
    """the floor of the device tolerance: oracle against restatement over the goldens, far below the 1e-9 they are pinned at"""
    floor = es.golden_floor()
    print("floor (nav, cov, Phi):", floor)
    assert all(0.0 < f <= 1e-10 for f in floor)
    # what the goldens do NOT reach (the reason for the edge streams): four row swaps in all, cond(S) below 1e5
    reps = [r for v in es.golden_replays().values() for r in v["reports"]]
    assert sum(len(r["swaps"]) for r in reps) <= 4 and max(r["cond"] for r in reps) < 1e5


def test_irregular_stream_conditions():
    s = es.stream("irregular")
    runs = es.run_lengths(s.events)
    for L in es.IRREGULAR_RUNS:
        assert L in runs, L
    assert s.events[0][0] == "pose"  # an update before any sample ...
    assert any(a[0] == "pose" and b[0] == "pose" for a, b in zip(s.events[1:], s.events[2:]))  # ... and two back to back later
    ts = np.array([e[1][0] for e in s.events if e[0] == "imu"])
    dt = np.diff(ts)
    assert (dt == 0.0).sum() >= 1 and (dt < 0.0).sum() == 1 and (dt >= 0.3).sum() >= 1
    assert {float(f"{d:.0e}") for d in dt if d > 0} >= {1e-5, 0.002, 0.01, 0.05, 0.3}
    assert max(runs) == 1025  # one more than the 1024 rows the host stages at a time (ptl_ekf::buf_rows)
    first = _reports("irregular")[0]
    assert first["zero_factors"] == 30 and first["swaps"] == []  # S exactly diagonal: every elimination factor is exactly zero


def test_pivot_stream_swaps_rows_at_every_pivot_column():
    sw = np.zeros(6, dtype=int)
    for r in _reports("pivot"):
        for c in r["swaps"]:
            sw[c] += 1
    print("pivot: row swaps at pivot columns 0..4:", sw[:5])
    assert (sw[:5] >= 1).all(), sw


def test_stiff_stream_reaches_an_ill_conditioned_innovation_covariance():
    c = max(r["cond"] for r in _reports("stiff"))
    print(f"stiff: largest cond(S) {c:.3g}")
    assert c >= 1e9


def test_innov_stream_has_a_huge_and_a_vanishing_innovation():
    s = es.stream("innov")
    f = es.restatement("innov")[1]
    ang = np.array([float(np.sqrt(r["innovation"][3:] @ r["innovation"][3:])) for r in f.reports])
    kinds = np.array(s.info["kinds"])
    assert ang[kinds == "big"].min() > 2.8
    assert np.array([float(np.abs(r["innovation"][:3]).max()) for r in f.reports])[kinds == "big"].min() > 10.0
    # "zero": the measurement is the oracle's predicted pose bit for bit.  A filter's Log of R^T R with its own R is exactly zero
    # (R^T R is exactly symmetric in any precision, so the quaternion's vector part is 0 - 0); the restatement's own state differs
    # from the oracle's by rounding, so on ITS run the angle is below 1e-9 and takes the series branch, not exactly zero.
    assert (kinds == "zero").sum() >= 9 and ang[kinds == "zero"].max() < 1e-9 < float(eld.SMALL_ANGLE)
    poses = [e[1] for e in s.events if e[0] == "pose"]
    for T, k in zip(poses, kinds):
        if k == "zero":
            R = eld.ld(T[:3, :3])
            assert (eld.log_so3(R.T @ R) == 0).all()
            assert (np.asarray(T[:3, :3].T @ T[:3, :3]) == np.asarray(T[:3, :3].T @ T[:3, :3]).T).all()


def test_long_stream_is_long():
    s = es.stream("long")
    assert sum(e[0] == "imu" for e in s.events) == 20000 and sum(e[0] == "pose" for e in s.events) == 2000
    assert len(es.checkpoints("long", s.events)) == 20


@pytest.mark.parametrize("name", es.STREAMS)
def test_oracle_against_restatement(name):
    """the oracle's own error on every edge stream (what the device's tolerance is relative to).  Measured, with one sanity bound:
    fp64 against 80 bits over at most 2e4 steps cannot differ by more than 1e-6 unless one of the two restates another filter."""
    en, ec = es.oracle_errors(name)
    print(f"{name}: oracle against restatement nav {en:.3g} cov {ec:.3g}")
    assert en <= 1e-6 and ec <= 1e-6
