"""numpy restatement of the IMU deskew's column table (include/ptudes_mi.h "IMU deskew"; csrc/icp_kernels.h
d_imu_coltab): knots (ts, pos[3], q xyzw[4]) of the filter's nominal pose, column j at t_j = t0 + (j / W)(t1 - t0), M_j = T(t_ref)^-1 T(t_j)
with t_ref the last knot's time and T the SE(3) geodesic between the bracketing knots, extrapolated by the end segment's twist at most the
largest knot interval outside the knots.  Same formulas as the device (csrc/devmath.h), in float64."""
import numpy as np


def quat_to_R(q):
    x, y, z, w = q
    xx, yy, zz, ww = x * x, y * y, z * z, w * w
    return np.array([[xx - yy - zz + ww, 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), -xx + yy - zz + ww, 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), -xx - yy + zz + ww]])


def R_to_quat(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    c, best = 0, R[0, 0]
    if R[1, 1] > best:
        c, best = 1, R[1, 1]
    if R[2, 2] > best:
        c = 2
        best = R[2, 2]
    if tr > best:
        c = 3
    if c == 3:
        q = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + tr]
    elif c == 0:
        q = [1.0 - tr + 2.0 * R[0, 0], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]]
    elif c == 1:
        q = [R[0, 1] + R[1, 0], 1.0 - tr + 2.0 * R[1, 1], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]]
    else:
        q = [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 - tr + 2.0 * R[2, 2], R[1, 0] - R[0, 1]]
    q = np.array(q)
    return q / np.sqrt(q @ q)


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def R_to_rotvec(R):
    q = R_to_quat(R)
    if q[3] < 0.0:
        q = -q
    a = 2.0 * np.arctan2(np.sqrt(q[:3] @ q[:3]), q[3])
    s = 2.0 + a * a / 12.0 + 7.0 * a ** 4 / 2880.0 if a <= 1e-3 else a / np.sin(0.5 * a)
    return s * q[:3]


def rotvec_to_R(v):
    a = np.sqrt(v @ v)
    s = 0.5 - a * a / 48.0 + a ** 4 / 3840.0 if a <= 1e-3 else np.sin(0.5 * a) / a
    return quat_to_R(np.array([s * v[0], s * v[1], s * v[2], np.cos(0.5 * a)]))


def se3_exp(xi):
    """xi = (upsilon, omega), Sophus order -> 4x4"""
    w = xi[3:]
    th2 = w @ w
    th = np.sqrt(th2)
    if th < 1e-6:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        sn, cs = np.sin(th), np.cos(th)
        # b as csrc/devmath.h se3_exp has it: (1 - cos) / th^2 cancels, and b K upsilon carries that into t as 1e-16 / th
        a, b, c = sn / th, (sn * sn / (th2 * (1.0 + cs)) if cs > 0.0 else (1.0 - cs) / th2), (th - sn) / (th2 * th)
    K = skew(w)
    K2 = K @ K
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * K2
    T[:3, 3] = (np.eye(3) + b * K + c * K2) @ xi[:3]
    return T


def se3_log(T):
    w = R_to_rotvec(T[:3, :3])
    th2 = w @ w
    th = np.sqrt(th2)
    k = 1.0 / 12.0 + th2 / 720.0 if th < 1e-6 else (1.0 - th * np.cos(0.5 * th) / (2.0 * np.sin(0.5 * th))) / th2
    K = skew(w)
    return np.concatenate([(np.eye(3) - 0.5 * K + k * (K @ K)) @ T[:3, 3], w])


def inv(T):
    o = np.eye(4)
    o[:3, :3] = T[:3, :3].T
    o[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return o


def knot_pose(k8):
    T = np.eye(4)
    T[:3, :3] = quat_to_R(k8[4:8])
    T[:3, 3] = k8[1:4]
    return T


def knot_of(ts, pos, q):
    return np.concatenate([[ts], pos, q])


def pose_at(knots, t):
    """T(t) on the knot list (n >= 2): P_i Exp(a Log(P_i^-1 P_i+1)), i the largest index with kt_i <= t clamped to [0, n - 2]"""
    kt = knots[:, 0]
    n = len(knots)
    i = int(np.searchsorted(kt, t, side="right")) - 1
    i = min(max(i, 0), n - 2)
    a = (t - kt[i]) / (kt[i + 1] - kt[i])
    P0, P1 = knot_pose(knots[i]), knot_pose(knots[i + 1])
    return P0 @ se3_exp(a * se3_log(inv(P0) @ P1))


def column_times(t0, t1, W):
    return t0 + (np.arange(W) * (1.0 / W)) * (t1 - t0)


def in_bounds(knots, t0, t1, W):
    """every column within one (the largest) knot interval of the knots"""
    if len(knots) < 2:
        return False
    kt = knots[:, 0]
    d = np.max(np.diff(kt))
    ta, tb = t0, t0 + ((W - 1) * (1.0 / W)) * (t1 - t0)
    return bool(kt[0] - d <= ta <= kt[-1] + d and kt[0] - d <= tb <= kt[-1] + d)


def column_table(knots, t0, t1, W):
    """(mode, (W, 4, 4)): mode 2 and M_j = T(t_ref)^-1 T(t_j), or mode 0 and identities (fewer than 2 knots, a column out of bounds)"""
    knots = np.asarray(knots, dtype=np.float64).reshape(-1, 8)
    if not in_bounds(knots, t0, t1, W):
        return 0, np.tile(np.eye(4), (W, 1, 1))
    Tinv = inv(pose_at(knots, knots[-1, 0]))
    return 2, np.array([Tinv @ pose_at(knots, t) for t in column_times(t0, t1, W)])


def deskew(xyz, table, W):
    """point i (column i % W) moved by its column's transform"""
    x = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    M = table[np.arange(len(x)) % W]
    # the device's order of operations (csrc/devmath.h rt_apply, no contraction): ((R0 x + R1 y) + R2 z) + t
    return np.stack([M[:, r, 0] * x[:, 0] + M[:, r, 1] * x[:, 1] + M[:, r, 2] * x[:, 2] + M[:, r, 3] for r in range(3)], axis=1)


def cv_table(xi, W):
    """kiss-icp's constant-velocity table Exp((j / W - 0.5) xi), referred to mid-sweep"""
    return np.array([se3_exp((j * (1.0 / W) - 0.5) * np.asarray(xi)) for j in range(W)])


def mechanise(R, p, v, imu_rows, t_prev, grav):
    """_insMech (reference ins/es_ekf.py:239-257) with zero bias estimates from (R, p, v) at t_prev through imu_rows: knots after each"""
    out = []
    for row in imu_rows:
        dt = row[0] - t_prev
        a = row[1:4]
        ag = R @ a + grav
        p = p + v * dt + 0.5 * ag * dt * dt
        v = v + ag * dt
        R = R @ rotvec_to_R(row[4:7] * dt)
        t_prev = row[0]
        out.append(knot_of(t_prev, p, R_to_quat(R)))
    return out
