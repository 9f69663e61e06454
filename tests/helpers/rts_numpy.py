"""Fixed-interval Rauch-Tung-Striebel smoother over an error-state EKF log, restated in numpy - the definition the device's
backward pass (k_ekf_smooth) is checked against.

Entry k of the log holds x_{k|k-1}, P_{k|k-1}, Phi_{k-1->k} (the product of the IMU transitions since the previous update),
x_{k|k}, P_{k|k}.  nav vectors are [pos(3), q xyzw(4), vel(3), bg(3), ba(3), grav(3)]; the error state is ordered
(pos, vel, phi, bg, ba, grav) and the attitude error is a right perturbation, R = R_hat Exp(phi).

    x^s_N = x_{N|N},  P^s_N = P_{N|N}
    C_k   = P_{k|k} Phi_{k->k+1}^T P_{k+1|k}^{-1}
    e     = x^s_{k+1} [-] x_{k+1|k}             attitude: Log(R_{k+1|k}^T R^s_{k+1}), the rest: difference
    x^s_k = x_{k|k} [+] C_k e                   attitude: R_{k|k} Exp(dphi)
    P^s_k = P_{k|k} + C_k (P^s_{k+1} - P_{k+1|k}) C_k^T,  then (P + P^T) / 2
"""
import numpy as np

POS, VEL, PHI, BG, BA, G = 0, 3, 6, 9, 12, 15
# nav index of each error-state block (the attitude block has no linear counterpart)
_NAV_OF = {POS: 0, VEL: 7, BG: 10, BA: 13, G: 16}


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    th = np.linalg.norm(w)
    K = skew(w)
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * K @ K


def log_so3(R):
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-8:
        return 0.5 * v
    if np.pi - th < 1e-6:  # near pi: from the symmetric part
        A = (R + np.eye(3)) / 2.0
        i = int(np.argmax(np.diag(A)))
        a = A[:, i] / np.sqrt(A[i, i])
        return th * a * (1.0 if a @ v >= 0 else -1.0)
    return th / (2.0 * np.sin(th)) * v


def quat_to_R(q):
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(t + 1.0)
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = np.empty(4)
        q[i] = 0.25 * s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
        q[3] = (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


def boxminus(a, b):
    """a [-] b for nav vectors, in the error-state order"""
    e = np.empty(18)
    for blk, n in _NAV_OF.items():
        e[blk:blk + 3] = a[n:n + 3] - b[n:n + 3]
    e[PHI:PHI + 3] = log_so3(quat_to_R(b[3:7]).T @ quat_to_R(a[3:7]))
    return e


def boxplus(x, d):
    """x [+] d: nav vector plus an error-state increment"""
    y = np.array(x, dtype=np.float64)
    for blk, n in _NAV_OF.items():
        y[n:n + 3] = x[n:n + 3] + d[blk:blk + 3]
    y[3:7] = R_to_quat(quat_to_R(x[3:7]) @ exp_so3(d[PHI:PHI + 3]))
    return y


def pose_of(nav):
    T = np.eye(4)
    T[:3, :3] = quat_to_R(nav[3:7])
    T[:3, 3] = nav[0:3]
    return T


def rts(log, boxminus=boxminus, boxplus=boxplus):
    """log: dict with nav_pred (N,19), P_pred (N,18,18), Phi (N,18,18), nav_post (N,19), P_post (N,18,18).
    Returns dict(nav (N,19), cov (N,18,18), poses (N,4,4), gain (N-1,18,18)).  boxminus / boxplus may be replaced (a linear
    model: plain difference / sum)."""
    navp, Pp, Phi, nav, P = (np.asarray(log[k], dtype=np.float64) for k in ("nav_pred", "P_pred", "Phi", "nav_post", "P_post"))
    N = len(nav)
    xs = np.empty_like(nav)
    Ps = np.empty_like(P)
    gains = np.empty((max(N - 1, 0), 18, 18))
    xs[-1], Ps[-1] = nav[-1], P[-1]
    for k in range(N - 2, -1, -1):
        # P_{k+1|k} X = Phi P_{k|k}  ->  C = X^T = P_{k|k} Phi^T P_{k+1|k}^{-1}
        C = np.linalg.solve(Pp[k + 1], Phi[k + 1] @ P[k]).T
        gains[k] = C
        xs[k] = boxplus(nav[k], C @ boxminus(xs[k + 1], navp[k + 1]))
        S = P[k] + C @ (Ps[k + 1] - Pp[k + 1]) @ C.T
        Ps[k] = 0.5 * (S + S.T)
    poses = np.stack([pose_of(x) for x in xs]) if N else np.zeros((0, 4, 4))
    return dict(nav=xs, cov=Ps, poses=poses, gain=gains)
