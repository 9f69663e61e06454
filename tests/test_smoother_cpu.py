"""The fixed-interval RTS smoother without a GPU: the numpy restatement (tests/helpers/rts_numpy.py) against the batch
weighted-least-squares solution of a linear-Gaussian toy, and the C-ABI's declared entry points against the built library's
exported symbols (both directions, the smoother's entry points included)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import rts_numpy as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptudes_mi.h")


def _toy(N=25, seed=3):
    """a linear 18-state model with the attitude block held at zero (identity transition, no coupling, not measured), its
    Kalman-filter log in the device log's layout, and the inputs of the batch least-squares problem"""
    rng = np.random.default_rng(seed)
    n = 18
    att = slice(rn.PHI, rn.PHI + 3)
    lin = [i for i in range(n) if not rn.PHI <= i < rn.PHI + 3]
    F = np.eye(n)
    F[np.ix_(lin, lin)] += 0.05 * rng.standard_normal((len(lin), len(lin)))
    A = rng.standard_normal((n, n)) * 0.1
    Q = A @ A.T + 0.01 * np.eye(n)
    Q[att, :] = 0.0
    Q[:, att] = 0.0
    Q[att, att] = 1e-4 * np.eye(3)
    H = np.zeros((9, n))
    H[0:3, 0:3] = np.eye(3)           # position
    H[3:6, 3:6] = np.eye(3)           # velocity
    H[6:9, 15:18] = np.eye(3)         # gravity
    H[6:9, 9:12] = 0.5 * np.eye(3)    # + a bias term
    R = 0.04 * np.eye(9)
    P0 = np.diag(rng.uniform(0.5, 2.0, n))
    m0 = np.zeros(n)
    m0[lin] = rng.standard_normal(len(lin))
    # a trajectory and its measurements
    x = m0 + np.sqrt(np.diag(P0)) * rng.standard_normal(n)
    x[att] = 0.0
    zs = []
    for k in range(N):
        if k:
            w = rng.multivariate_normal(np.zeros(n), Q)
            w[att] = 0.0
            x = F @ x + w
        zs.append(H @ x + rng.multivariate_normal(np.zeros(9), R))

    def nav_of(s):  # nav vector with an identity attitude (the attitude error stays zero)
        v = np.zeros(19)
        v[6] = 1.0
        for blk, i in rn._NAV_OF.items():
            v[i:i + 3] = s[blk:blk + 3]
        return v

    log = {k: [] for k in ("nav_pred", "P_pred", "Phi", "nav_post", "P_post")}
    m, P = m0.copy(), P0.copy()
    for k in range(N):
        if k:
            m, P = F @ m, F @ P @ F.T + Q
        log["nav_pred"].append(nav_of(m))
        log["P_pred"].append(P.copy())
        log["Phi"].append(F.copy() if k else np.eye(n))
        S = H @ P @ H.T + R
        K = P @ H.T @ np.linalg.inv(S)
        m = m + K @ (zs[k] - H @ m)
        P = (np.eye(n) - K @ H) @ P
        assert np.allclose(m[att], 0.0)
        log["nav_post"].append(nav_of(m))
        log["P_post"].append(P.copy())
    log = {k: np.array(v) for k, v in log.items()}
    return log, dict(F=F, Q=Q, H=H, R=R, P0=P0, m0=m0, zs=zs, N=N, nav_of=nav_of)


def _wls(t):
    """argmin over x_0..x_{N-1} of the prior, dynamics and measurement terms: the smoothed means; the inverse of the normal
    matrix: the smoothed covariances"""
    F, Q, H, R, P0, m0, zs, N = (t[k] for k in ("F", "Q", "H", "R", "P0", "m0", "zs", "N"))
    n = 18
    Qi, Ri, P0i = np.linalg.inv(Q), np.linalg.inv(R), np.linalg.inv(P0)
    A = np.zeros((n * N, n * N))
    b = np.zeros(n * N)
    s = lambda k: slice(n * k, n * (k + 1))  # noqa: E731
    A[s(0), s(0)] += P0i
    b[s(0)] += P0i @ m0
    for k in range(N):
        A[s(k), s(k)] += H.T @ Ri @ H
        b[s(k)] += H.T @ Ri @ zs[k]
        if k + 1 < N:
            A[s(k), s(k)] += F.T @ Qi @ F
            A[s(k + 1), s(k + 1)] += Qi
            A[s(k), s(k + 1)] -= F.T @ Qi
            A[s(k + 1), s(k)] -= Qi @ F
    x = np.linalg.solve(A, b).reshape(N, n)
    cov = np.linalg.inv(A)
    return x, np.array([cov[s(k), s(k)] for k in range(N)])


def test_rts_restatement_equals_batch_least_squares_on_a_linear_toy():
    log, t = _toy()
    sm = rn.rts(log)
    x_wls, P_wls = _wls(t)
    nav_wls = np.array([t["nav_of"](x) for x in x_wls])
    assert np.abs(sm["nav"] - nav_wls).max() < 1e-10
    assert np.abs(sm["cov"] - P_wls).max() < 1e-10 * np.abs(P_wls).max()
    # the last row is the filter's own
    assert np.array_equal(sm["nav"][-1], log["nav_post"][-1])
    # the box operators with a zero attitude error are the linear ones
    lin = rn.rts(log, boxminus=lambda a, b: _lin_minus(a, b), boxplus=lambda x, d: _lin_plus(x, d))
    assert np.abs(lin["nav"] - sm["nav"]).max() < 1e-12


def _lin_minus(a, b):
    e = np.zeros(18)
    for blk, i in rn._NAV_OF.items():
        e[blk:blk + 3] = a[i:i + 3] - b[i:i + 3]
    return e


def _lin_plus(x, d):
    y = np.array(x)
    for blk, i in rn._NAV_OF.items():
        y[i:i + 3] = x[i:i + 3] + d[blk:blk + 3]
    return y


def test_rts_restatement_attitude_operators_are_inverse():
    rng = np.random.default_rng(0)
    for _ in range(20):
        x = np.zeros(19)
        x[3:7] = rn.R_to_quat(rn.exp_so3(rng.standard_normal(3)))
        x[[0, 1, 2, 7, 8, 9]] = rng.standard_normal(6)
        d = 0.3 * rng.standard_normal(18)
        y = rn.boxplus(x, d)
        assert np.abs(rn.boxminus(y, x) - d).max() < 1e-12


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"#define[^\n]*", " ", src)
    return set(re.findall(r"^[ \t]*(?:const\s+)?[A-Za-z_]\w*[\s\*]+(ptl_\w+)\s*\(", src, flags=re.M))


def _exported(path):
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("nm (binutils) is needed to list the library's exported symbols")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ptl_") and " T " in ln}


def test_every_header_prototype_is_exported_and_every_export_is_declared():
    from ptudes_lab_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (python -c 'import __graft_entry__ as g; g.build()')")
    declared, exported = _declared(), _exported(_lib.LIB_PATH)
    assert declared - exported == set(), "declared in include/ptudes_mi.h, not exported"
    assert exported - declared == set(), "exported, not declared in include/ptudes_mi.h"
    new = {"ptl_ekf_log_enable", "ptl_ekf_smooth", "ptl_ekf_smoother_log", "ptl_seq_smoother_enable", "ptl_seq_smooth",
           "ptl_seq_smoother_log", "ptl_batch_smoother_enable", "ptl_batch_smooth", "ptl_batch_smoothed", "ptl_batch_smoother_log"}
    assert new <= declared
    # the binding knows every one of them, and the ABI version stays (new entry points change no struct or prototype)
    assert set(_lib.PROTOTYPES) == declared
    assert _lib.lib().ptl_abi_version() == 6 == _lib.ABI_VERSION
