"""The 18-state error-state filter restated in numpy.longdouble (x87 80-bit: 64-bit significand), the reference the
edge streams of tests/helpers/ekf_edge_streams.py are held against.

Written from the meaning of the reference's ESEKF.processImu / processPose (ins/es_ekf.py) and NavState (ins/data.py),
not from its code and not from the device's or the C oracle's: the attitude is an xyzw quaternion renormalised through
R -> quat after every change, Exp is Rodrigues' formula (series below 1e-4 rad), Log goes through the quaternion (with the
w < 0 flip), the noise terms are copied by their USE (the velocity block takes the 0.049 term, the attitude block 0.38,
the accelerometer bias 0.0043, the gyro bias 0.000466), the covariance update is the non-Joseph (I - K Jp) P, and the 6x6
inverse is a Gauss-Jordan elimination with partial pivoting (numpy.linalg refuses longdouble) that also reports what it
did: the pivot columns at which it swapped rows, how many elimination factors were exactly zero, and cond(S).
"""
import numpy as np

LD = np.longdouble
# a restatement no wider than the code under test is not a reference: fail here, do not skip
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not wider than fp64 on this machine"

N = 18
POS, VEL, PHI, BG, BA, GRV = 0, 3, 6, 9, 12, 15
GRAV = LD("9.782940329221166")
SEL = np.array([POS, POS + 1, POS + 2, PHI, PHI + 1, PHI + 2])
_ONE, _TWO, _HALF = LD(1), LD(2), LD(1) / LD(2)
_I3 = np.eye(3, dtype=LD)
SMALL_ANGLE = LD("1e-4")


def ld(a):
    return np.array(a, dtype=LD)


def hat(v):
    z = LD(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=LD)


def exp_so3(v):
    """Rodrigues: I + A hat(v) + B hat(v)^2, A = sin(t) / t, B = (1 - cos t) / t^2 (their series below SMALL_ANGLE)"""
    t2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    t = np.sqrt(t2)
    if t < SMALL_ANGLE:
        A = _ONE - t2 / 6 + t2 * t2 / 120
        B = _HALF - t2 / 24 + t2 * t2 / 720
    else:
        A = np.sin(t) / t
        s = np.sin(t * _HALF)
        B = _TWO * s * s / t2
    K = hat(v)
    return _I3 + A * K + B * (K @ K)


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[w * w + x * x - y * y - z * z, _TWO * (x * y - z * w), _TWO * (x * z + y * w)],
                     [_TWO * (x * y + z * w), w * w - x * x + y * y - z * z, _TWO * (y * z - x * w)],
                     [_TWO * (x * z - y * w), _TWO * (y * z + x * w), w * w - x * x - y * y + z * z]], dtype=LD)


def R_to_quat(R):
    """unit xyzw quaternion of a (near) rotation: the largest of (m00, m11, m22, trace) picks the well-conditioned form"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    d = (R[0, 0], R[1, 1], R[2, 2], tr)
    c = int(np.argmax(d))
    q = np.empty(4, dtype=LD)
    if c == 3:
        q[0], q[1], q[2], q[3] = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], _ONE + tr
    else:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i] = _ONE - tr + _TWO * R[i, i]
        q[j] = R[j, i] + R[i, j]
        q[k] = R[k, i] + R[i, k]
        q[3] = R[k, j] - R[j, k]
    return q / np.sqrt(q @ q)


def log_so3(R):
    """rotation vector through the quaternion; w < 0 is flipped so that the angle stays within pi"""
    q = R_to_quat(R)
    if q[3] < 0:
        q = -q
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    a = _TWO * np.arctan2(n, q[3])
    if a < SMALL_ANGLE:
        scale = _TWO + a * a / 12 + 7 * a * a * a * a / 2880
    else:
        scale = a / np.sin(a * _HALF)
    return scale * q[:3]


def inv_gauss_jordan(S):
    """(S^-1, report): Gauss-Jordan on [S | I] with partial pivoting (first largest |entry| of the column at or below the
    diagonal); report = dict(swaps: the pivot columns at which rows were exchanged, zero_factors: elimination factors that
    were exactly zero, cond: the 2-norm condition number of S)"""
    n = S.shape[0]
    M = np.concatenate([np.array(S, dtype=LD), np.eye(n, dtype=LD)], axis=1)
    swaps, zero = [], 0
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if M[p, c] == 0:
            raise np.linalg.LinAlgError("singular matrix")
        if p != c:
            M[[c, p]] = M[[p, c]]
            swaps.append(c)
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r == c:
                continue
            f = M[r, c]
            if f == 0:
                zero += 1
                continue
            M[r] = M[r] - f * M[c]
    cond = float(np.linalg.cond(np.asarray(S, dtype=np.float64)))
    return M[:, n:].copy(), dict(swaps=swaps, zero_factors=zero, cond=cond)


def initial_cov():
    """diagonal: position 10 m, velocity 5 m/s, attitude = the rotation vector of the intrinsic-XYZ Euler angles (10, 10, 10)
    degrees, gyro bias 1.5, accelerometer bias 0.5, gravity 2.5 (standard deviations)"""
    a = LD(10) * (LD(4) * np.arctan(LD(1))) / LD(180)
    c, s, z, o = np.cos(a), np.sin(a), LD(0), LD(1)
    Rx = ld([[o, z, z], [z, c, -s], [z, s, c]])
    Ry = ld([[c, z, s], [z, o, z], [-s, z, c]])
    Rz = ld([[c, -s, z], [s, c, z], [z, z, o]])
    rv = log_so3(Rx @ Ry @ Rz)
    P = np.zeros((N, N), dtype=LD)
    for i in range(3):
        P[POS + i, POS + i] = 100
        P[VEL + i, VEL + i] = 25
        P[PHI + i, PHI + i] = rv[i] * rv[i]
        P[BG + i, BG + i] = LD("1.5") * LD("1.5")
        P[BA + i, BA + i] = LD("0.5") * LD("0.5")
        P[GRV + i, GRV + i] = LD("2.5") * LD("2.5")
    return P


# process noise by use; the literals are the fp64 numbers the filters square (0.049 is not a binary fraction)
_W_VEL = LD(0.049) * LD(0.049)
_W_PHI = LD(0.38) * LD(0.38)
_W_BA = LD(0.0043) * LD(0.0043)
_W_BG = LD(0.000466) * LD(0.000466)
_R_POS = LD(0.02) * LD(0.02)
_R_ATT = LD(0.01) * LD(0.01)


class EkfLD:
    def __init__(self, init_grav=None, init_bacc=None, init_bgyr=None):
        self.pos, self.vel = np.zeros(3, dtype=LD), np.zeros(3, dtype=LD)
        self.q = ld([0, 0, 0, 1])
        self.grav = ld([0, 0, -GRAV]) if init_grav is None else ld(init_grav)
        self.ba = np.zeros(3, dtype=LD) if init_bacc is None else ld(init_bacc)
        self.bg = np.zeros(3, dtype=LD) if init_bgyr is None else ld(init_bgyr)
        self.P = initial_cov()
        self.Fx = np.eye(N, dtype=LD)   # persistent: identity plus the blocks every predict rewrites
        self.W = np.zeros((N, N), dtype=LD)
        self.Phi = np.eye(N, dtype=LD)  # product of the Fx since the last update
        self.ts, self.dt = LD(0), LD(0)
        self.initialized = False
        self.reports = []               # one inverse report per update, plus the innovation (6) as "innovation"

    # ---- accessors
    def nav(self):
        return np.concatenate([self.pos, self.q, self.vel, self.bg, self.ba, self.grav])

    def pose_mat(self):
        T = np.eye(4, dtype=LD)
        T[:3, :3] = quat_to_R(self.q)
        T[:3, 3] = self.pos
        return T

    # ---- predict
    def process_imu(self, lacc, avel, ts):
        ts = LD(ts)
        self.dt = dt = ts - self.ts
        self.ts = ts
        if not self.initialized:  # the first sample only latches its time
            self.initialized = True
            return
        a = ld(lacc) - self.ba
        w = ld(avel) - self.bg
        Rp = quat_to_R(self.q)
        Rd = exp_so3(w * dt)
        ag = Rp @ a + self.grav
        self.pos = self.pos + self.vel * dt + _HALF * ag * dt * dt
        self.vel = self.vel + ag * dt
        self.q = R_to_quat(Rp @ Rd)
        Fx, W = self.Fx, self.W
        Fx[POS:POS + 3, VEL:VEL + 3] = dt * _I3
        Fx[VEL:VEL + 3, PHI:PHI + 3] = -dt * (Rp @ hat(a))
        Fx[VEL:VEL + 3, BA:BA + 3] = -dt * Rp
        Fx[PHI:PHI + 3, PHI:PHI + 3] = Rd.T
        Fx[PHI:PHI + 3, BG:BG + 3] = -dt * _I3
        W[VEL:VEL + 3, VEL:VEL + 3] = dt * dt * _W_VEL * _I3
        W[PHI:PHI + 3, PHI:PHI + 3] = dt * dt * _W_PHI * _I3
        W[BA:BA + 3, BA:BA + 3] = dt * _W_BA * _I3
        W[BG:BG + 3, BG:BG + 3] = dt * _W_BG * _I3
        self.P = Fx @ self.P @ Fx.T + W
        self.Phi = Fx @ self.Phi

    # ---- update
    def process_pose(self, pose, meas_cov=None):
        pose = ld(pose).reshape(4, 4)
        if meas_cov is None:
            Rm = np.diag(ld([_R_POS] * 3 + [_R_ATT] * 3))
        else:
            Rm = ld(meas_cov).reshape(6, 6)
        r = np.empty(6, dtype=LD)
        r[:3] = pose[:3, 3] - self.pos
        r[3:] = log_so3(quat_to_R(self.q).T @ pose[:3, :3])
        P = self.P
        S = P[np.ix_(SEL, SEL)] + Rm
        Si, rep = inv_gauss_jordan(S)
        rep["innovation"] = r.copy()
        self.reports.append(rep)
        K = P[:, SEL] @ Si
        dx = K @ r
        IKH = np.eye(N, dtype=LD)
        IKH[:, SEL] -= K
        P = IKH @ P
        self.pos = self.pos + dx[POS:POS + 3]
        self.vel = self.vel + dx[VEL:VEL + 3]
        self.bg = self.bg + dx[BG:BG + 3]
        self.ba = self.ba + dx[BA:BA + 3]
        self.grav = self.grav + dx[GRV:GRV + 3]
        dth = dx[PHI:PHI + 3]
        self.q = R_to_quat(quat_to_R(self.q) @ exp_so3(dth))
        G = _I3 - hat(_HALF * dth)  # projection of the attitude block only
        P[PHI:PHI + 3, PHI:PHI + 3] = G @ P[PHI:PHI + 3, PHI:PHI + 3] @ G.T
        self.P = P
        self.Phi = np.eye(N, dtype=LD)
