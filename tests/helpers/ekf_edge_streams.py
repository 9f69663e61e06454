"""Edge streams of the error-state filter: irregular IMU timing and batch lengths, pivoting in the 6x6 inverse, stiff measurement
covariances, large and zero innovations, a long run.  DESIGN.md 3.15.2.

A stream is a list of events built once from a seed, ("imu", row7) and ("pose", T44, cov66 | None); every consumer (the longdouble
restatement tests/helpers/ekf_longdouble.py, the C oracle, the device) replays the same list.  A measurement is the C oracle's
predicted pose at that instant composed with a seeded perturbation, so the oracle is run once to materialise the list.

The tolerance of every comparison with the device is relative to the oracle's own error against the restatement:
e_dev <= FACTOR * e_orc + floor, the floor being the largest oracle-against-restatement error over the reference's own golden
streams (golden_floor).  Nothing here is taken from the device's output.
"""
import functools
import os
from collections import namedtuple

import numpy as np

from oracle import cpu as orc
from tests.helpers import ekf_longdouble as eld

LD = eld.LD
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
STREAMS = ("irregular", "pivot", "stiff", "innov", "long")
FACTOR = 4.0
# IMU samples between two updates of `irregular`: one chunk of the kernel is 64 samples, the host stages 1024 rows at a time
IRREGULAR_RUNS = (1, 2, 63, 64, 65, 127, 128, 129, 7, 1025)
IRREGULAR_DTS = (0.0, 1e-5, 0.002, 0.01, 0.05, 0.3)
# per-scan run lengths of the runner test (the batched runner refuses an empty interval, so the issue's 0 is a 1)
RUNNER_RUNS = (5, 1, 1, 63, 64, 65, 129, 2, 128)
_SEED = dict(irregular=2001, pivot=2002, stiff=2003, innov=2004, long=2005)
BIG_ROTVEC, BIG_SHIFT = np.array([0.3, -2.9, 0.4]), np.array([40.0, -25.0, 10.0])

Stream = namedtuple("Stream", "name events info")


def _exp64(v):
    return np.asarray(eld.exp_so3(eld.ld(v)), dtype=np.float64)


def _imu_rows(rng, ts, rate):
    """smooth seeded sinusoids: a steady turn of 0.6 * rate about a seeded axis plus 0.5 * rate of slow oscillation (the attitude
    leaves the identity and keeps going), accelerations near [0, 0, 9.78], a little noise"""
    n = len(ts)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    f, ph = rng.uniform(0.15, 0.6, size=(2, 3)), rng.uniform(0, 2 * np.pi, size=(2, 3))
    t = ts[:, None] - ts[0]
    avel = 0.6 * rate * axis + 0.5 * rate * np.sin(2 * np.pi * f[0] * t + ph[0]) + rng.normal(scale=0.002, size=(n, 3))
    lacc = np.array([0.0, 0.0, 9.78]) + 0.5 * np.sin(2 * np.pi * f[1] * t + ph[1]) + rng.normal(scale=0.02, size=(n, 3))
    return np.ascontiguousarray(np.c_[ts, lacc, avel])


def _perturb(rng, rot=0.01, shift=0.03):
    T = np.eye(4)
    T[:3, :3] = _exp64(rng.normal(scale=rot / np.sqrt(3.0), size=3))
    T[:3, 3] = rng.normal(scale=shift / np.sqrt(3.0), size=3)
    return T


def _materialise(name, plan, info):
    """plan: ("imu", row) / ("pose", kind, cov, perturbation) -> events, the measurements from one run of the C oracle"""
    ekf = orc.EKF()
    events, kinds = [], []
    for p in plan:
        if p[0] == "imu":
            ekf.process_imu(p[1][1:4], p[1][4:7], p[1][0])
            events.append(("imu", p[1]))
            continue
        _, kind, cov, D = p
        T = ekf.pose_mat()
        if kind != "zero":  # "zero": exactly the predicted pose
            T = T @ D
        ekf.process_pose(T, cov)
        events.append(("pose", T, cov))
        kinds.append(kind)
    info = dict(info, kinds=kinds)
    return Stream(name, events, info)


def _every(rows, every, pose_of):
    plan, k = [], 0
    for i, r in enumerate(rows):
        plan.append(("imu", r))
        if (i + 1) % every == 0:
            plan.append(pose_of(k))
            k += 1
    return plan


@functools.lru_cache(maxsize=None)
def stream(name):
    rng = np.random.default_rng(_SEED[name])
    if name == "irregular":
        n = sum(IRREGULAR_RUNS)
        dts = rng.choice(IRREGULAR_DTS[:5], size=n, p=[0.08, 0.08, 0.34, 0.45, 0.05])
        starts = np.cumsum((0,) + IRREGULAR_RUNS[:-1])
        # the first sample of the SECOND chunk of the 127-, 128- and 129-sample runs: the one long gap, the one step back, a repeat
        dts[starts[5] + 64], dts[starts[6] + 64], dts[starts[7] + 64] = 0.3, -0.004, 0.0
        dts[starts[9] + 1024] = 0.0  # ... and the row past the host's staging buffer
        ts = 10.0 + np.cumsum(dts)
        rows = _imu_rows(rng, ts, 0.8)
        plan = [("pose", "plain", None, _perturb(rng))]  # an update before any sample
        a = 0
        for L in IRREGULAR_RUNS:
            plan += [("imu", r) for r in rows[a:a + L]]
            a += L
            plan.append(("pose", "plain", None, _perturb(rng)))
            if L == 64:
                plan.append(("pose", "plain", None, _perturb(rng)))  # two updates back to back
        return _materialise(name, plan, dict(rows=rows, runs=IRREGULAR_RUNS))
    if name == "pivot":
        rows = _imu_rows(rng, 10.0 + 0.01 * np.arange(1, 301), 0.8)

        def pose_of(k):
            A = rng.normal(size=(6, 6)) * (0.05 * np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0]))[:, None]
            return ("pose", "plain", A @ A.T + 1e-6 * np.eye(6), _perturb(rng))
        return _materialise(name, _every(rows, 10, pose_of), dict(rows=rows))
    if name == "stiff":
        rows = _imu_rows(rng, 10.0 + 0.01 * np.arange(1, 401), 0.8)
        covs = [np.zeros((6, 6)), 1e-12 * np.eye(6), 1e6 * np.eye(6), np.diag([1e-10, 1e-2, 1e4, 1e-8, 1.0, 1e-12])]
        return _materialise(name, _every(rows, 10, lambda k: ("pose", "plain", covs[k % 4], _perturb(rng))), dict(rows=rows))
    if name == "innov":
        rows = _imu_rows(rng, 10.0 + 0.01 * np.arange(1, 301), 0.8)

        def pose_of(k):
            if k % 3 == 0:
                D = np.eye(4)
                D[:3, :3] = _exp64((1.0 if (k // 3) % 2 == 0 else -1.0) * BIG_ROTVEC)
                D[:3, 3] = BIG_SHIFT
                return ("pose", "big", None, D)
            return ("pose", "zero" if k % 3 == 1 else "plain", None, _perturb(rng))
        return _materialise(name, _every(rows, 10, pose_of), dict(rows=rows))
    if name == "long":
        rows = _imu_rows(rng, 10.0 + 0.005 * np.arange(1, 20001), 1.5)
        return _materialise(name, _every(rows, 10, lambda k: ("pose", "plain", None, _perturb(rng))), dict(rows=rows))
    raise KeyError(name)


def run_lengths(events):
    """IMU samples between consecutive updates (and before the first / after the last, when there are any)"""
    out, n = [], 0
    for e in events:
        if e[0] == "imu":
            n += 1
        else:
            out.append(n)
            n = 0
    return out + ([n] if n else [])


def checkpoints(name, events):
    """indices of the events after which the state is compared: after every update and after every run of samples; on `long`
    after every 100th update only"""
    if name == "long":
        poses = [i for i, e in enumerate(events) if e[0] == "pose"]
        return poses[99::100]
    return [i for i, e in enumerate(events)
            if e[0] == "pose" or i + 1 == len(events) or events[i + 1][0] == "pose"]


# ------------------------------------------------------------------------------------------------ errors
def nav_err(a, ref):
    """the sign-invariant quaternion distance of tests/test_gpu_parity.py::_nav_close, as a number"""
    a, ref = eld.ld(a), eld.ld(ref)
    q = min(np.abs(a[3:7] - ref[3:7]).max(), np.abs(a[3:7] + ref[3:7]).max())
    return float(max(np.abs(a[:3] - ref[:3]).max(), q, np.abs(a[7:] - ref[7:]).max()))


def cov_err(P, ref):
    P, ref = eld.ld(P), eld.ld(ref)
    return float(np.abs(P - ref).max() / max(LD(1), np.abs(ref).max()))


def errors(got, ref):
    """largest (nav, cov) error of the checkpoints `got` {i: (nav, P)} against `ref`"""
    return (max(nav_err(got[i][0], ref[i][0]) for i in got), max(cov_err(got[i][1], ref[i][1]) for i in got))


def within(e_dev, e_orc, floor, factor=FACTOR):
    return e_dev <= factor * e_orc + floor


# ------------------------------------------------------------------------------------------------ the two host replays
def replay(f, events, ckpts, state):
    ck, out = set(ckpts), {}
    for i, e in enumerate(events):
        if e[0] == "imu":
            f.process_imu(e[1][1:4], e[1][4:7], e[1][0])
        else:
            f.process_pose(e[1], e[2])
        if i in ck:
            out[i] = state(f)
    return out


def _ld_state(f):
    return f.nav(), f.P.copy()


def _orc_state(f):
    return f.nav, f.cov


@functools.lru_cache(maxsize=None)
def restatement(name):
    """(checkpoints {i: (nav, P)}, the filter with its per-update reports) of the longdouble restatement"""
    s = stream(name)
    f = eld.EkfLD()
    return replay(f, s.events, checkpoints(name, s.events), _ld_state), f


@functools.lru_cache(maxsize=None)
def oracle(name):
    s = stream(name)
    return replay(orc.EKF(), s.events, checkpoints(name, s.events), _orc_state)


@functools.lru_cache(maxsize=None)
def oracle_errors(name):
    return errors(oracle(name), restatement(name)[0])


# ------------------------------------------------------------------------------------------------ goldens: the floor
def _golden_events(variant):
    g = np.load(os.path.join(GOLDEN, f"ekf_steps_{variant}.npz"))
    init = (None, None, None) if variant not in ("init", "inverted") else (g["init_grav"], g["init_bacc"], g["init_bgyr"])
    upd = {int(i): k for k, i in enumerate(g["upd_idx"])}
    ev = []
    for i in range(len(g["imu_ts"])):
        ev.append(("imu", np.r_[g["imu_ts"][i], g["imu_lacc"][i], g["imu_avel"][i]]))
        if i in upd:
            ev.append(("pose", g["upd_pose"][upd[i]], g["upd_cov"][upd[i]] if bool(g["has_cov"]) else None))
    return g, init, ev


class _PhiTracker:
    """the C oracle with the running product of its Fx since the last update (fp64), what the device's smoother log calls Phi"""

    def __init__(self, *init):
        self.f, self.Phi, self.seen = orc.EKF(*init), np.eye(18), False

    def process_imu(self, lacc, avel, ts):
        self.f.process_imu(lacc, avel, ts)
        if self.seen:  # the first sample only latches
            self.Phi = self.f.fx @ self.Phi
        self.seen = True

    def process_pose(self, pose, cov=None):
        self.f.process_pose(pose, cov)
        self.Phi = np.eye(18)


def phi_err(Phi, ref):
    return cov_err(Phi, ref)


@functools.lru_cache(maxsize=None)
def golden_replays():
    """per golden stream: (restatement-against-golden nav, cov error; oracle-against-restatement nav, cov, Phi error; reports)"""
    out = {}
    for v in ("default", "init", "cov", "turn", "inverted"):
        g, init, ev = _golden_events(v)
        f, o = eld.EkfLD(*init), _PhiTracker(*init)
        gn = gc = on = oc = op = 0.0
        ii = ku = 0
        for e in ev:
            if e[0] == "imu":
                for x in (f, o):
                    x.process_imu(e[1][1:4], e[1][4:7], e[1][0])
                gn = max(gn, nav_err(g["nav_after_imu"][ii], f.nav()))
                ii += 1
                op = max(op, phi_err(o.Phi, f.Phi))
            else:
                gc = max(gc, cov_err(g["cov_pre"][ku], f.P))
                for x in (f, o):
                    x.process_pose(e[1], e[2])
                gn = max(gn, nav_err(g["nav_after_upd"][ku], f.nav()))
                gc = max(gc, cov_err(g["cov_post"][ku], f.P))
                ku += 1
            on, oc = max(on, nav_err(o.f.nav, f.nav())), max(oc, cov_err(o.f.cov, f.P))
        out[v] = dict(golden=(gn, gc), oracle=(on, oc, op), reports=f.reports)
    # ekf-bench sim: an ideal filter whose pose corrects a noisy one (the measurements materialised by the oracle's ideal filter)
    g = np.load(os.path.join(GOLDEN, "ekf_sim.npz"))
    ts = g["ts"]
    o_gt, o, f_gt, f = orc.EKF(), _PhiTracker(), eld.EkfLD(), eld.EkfLD()
    last, on, oc, op = ts[0], 0.0, 0.0, 0.0
    for i in range(len(ts)):
        for x in (o_gt, f_gt):
            x.process_imu(g["ideal_lacc"][i], g["ideal_avel"][i], ts[i])
        for x in (o, f):
            x.process_imu(g["noisy_lacc"][i], g["noisy_avel"][i], ts[i])
        op = max(op, phi_err(o.Phi, f.Phi))
        if ts[i] - last > 0.1:
            T = o_gt.pose_mat()
            for x in (o, f):
                x.process_pose(T)
            last = ts[i]
        on, oc = max(on, nav_err(o.f.nav, f.nav()), nav_err(o_gt.nav, f_gt.nav())), max(oc, cov_err(o.f.cov, f.P))
    out["sim"] = dict(golden=(max(nav_err(g["nav"], f.nav()), nav_err(g["nav_gt"], f_gt.nav())), cov_err(g["cov"], f.P)),
                      oracle=(on, oc, op), reports=f.reports)
    return out


def golden_floor():
    """(nav, cov, Phi): the largest oracle-against-restatement error over the reference's own golden streams"""
    r = golden_replays()
    return tuple(max(v["oracle"][k] for v in r.values()) for k in range(3))


# ------------------------------------------------------------------------------------------------ the runner replay
def runner_imu():
    """(rows, imu_end) of the runner test: the first rows of `irregular`, RUNNER_RUNS samples before scan 0 / between scans"""
    end = np.cumsum(RUNNER_RUNS)
    return stream("irregular").info["rows"][:end[-1]].copy(), [int(e) for e in end]


def runner_replay(f, rows, imu_end, kiss_poses):
    """update with pose k, then the samples before scan k + 1: the rows a runner writes and its smoother log holds.  f: an EkfLD or a
    _PhiTracker"""
    ld_ = isinstance(f, eld.EkfLD)
    nav = (lambda: f.nav()) if ld_ else (lambda: f.f.nav)
    cov = (lambda: f.P.copy()) if ld_ else (lambda: f.f.cov)
    pose = (lambda: f.pose_mat()) if ld_ else (lambda: f.f.pose_mat())
    ts = (lambda: f.ts) if ld_ else (lambda: f.f.ts)
    out = dict(res_poses=[], res_t=[], nav_pred=[], P_pred=[], Phi=[], nav_post=[], P_post=[])
    for r in rows[:imu_end[0]]:
        f.process_imu(r[1:4], r[4:7], r[0])
    for k, T in enumerate(kiss_poses):
        out["nav_pred"].append(nav()); out["P_pred"].append(cov()); out["Phi"].append(f.Phi.copy())
        f.process_pose(T, None)
        out["nav_post"].append(nav()); out["P_post"].append(cov())
        out["res_poses"].append(pose()); out["res_t"].append(float(ts()))
        if k + 1 < len(imu_end):
            for r in rows[imu_end[k]:imu_end[k + 1]]:
                f.process_imu(r[1:4], r[4:7], r[0])
    return out


def runner_errors(got, ref):
    """(nav, cov, Phi) errors of a runner's rows (res_poses and the smoother log) against the restatement's"""
    n = len(ref["res_t"])
    en = max(max(nav_err(got[k][i], ref[k][i]) for k in ("nav_pred", "nav_post")) for i in range(n))
    en = max(en, max(float(np.abs(eld.ld(got["res_poses"][i]) - ref["res_poses"][i]).max()) for i in range(n)))
    ec = max(max(cov_err(got[k][i], ref[k][i]) for k in ("P_pred", "P_post")) for i in range(n))
    ep = max(phi_err(got["Phi"][i], ref["Phi"][i]) for i in range(n))
    return en, ec, ep
