"""csrc/devmath.h, function by function, against mpmath at 50 digits - the host compile and the gfx950 compile of the same
header (tests/hip/devmath_probe.hip, built by tests/helpers/devmath_probe.py into a temporary directory).

The rest of the suite compares the kernels with a CPU oracle that uses the same formulas, on data whose attitude stays below
56 degrees.  Here the inputs are chosen for the branches: every case of the matrix-to-quaternion conversion, angles up to and
at pi, both sides of every series / closed-form switch of the header, matrices off orthogonality, ill-conditioned solves.

References are written from the definitions: Rodrigues' formula and the left Jacobian V in mpmath (cross-checked below against
mpmath's matrix exponential), the exact unit quaternion of the generating rotation vector (convention: scipy's, up to sign),
the orthogonal polar factor from mpmath's SVD, mpmath's LU for inverses and solves.

Errors are absolute, divided by the magnitude of the quantity (1 for rotation entries, quaternions, rotation vectors and
angles; |upsilon| or |t| for translations; cond * |x| for inverses and solves) and quoted in units of 2^-52.  The bound of a
function is four times the worst error of its HOST compile over the grid outside the band 1e-6 <= th < 1e-2 (HOST_WORST
below, measured; ocml documents 1-2 ulp for fp64 sin / cos / atan2 where glibc gives <= 1).  The same bound is then asked of
the host and of the device everywhere, the band included, and of |device - host| per input.

Measured worst scaled errors, units of 2^-52 (host = x86-64 / glibc, device = MI355X / ocml):

    function       host    device   |device - host|
    R_to_quat      1.00    1.00     0.00
    quat_to_R      1.50    1.50     0.00
    rotvec_to_R    2.50    2.50     2.00
    R_to_rotvec    4.00    4.00     4.00
    rot_angle      2.00    2.00     2.00
    rt_project     2.00    2.00     0.00
    mat3_polar     1.50    1.50     0.00
    se3_exp        2.00    2.00     0.00
    se3_exp_gn     2.00    2.00     0.00
    se3_log        2.00    2.40     2.80
    rt_inv         0.96    0.96     0.00
    rt_mul         1.01    1.01     0.00
    mat4_inv       1.78    1.78     0.00
    solve6_ldlt    2.00    2.00     0.00

(whole grid, the band included; se3_exp and se3_exp_gn on the device are bit-equal to the host on every input of the grid.)
se3_exp_gn against se3_exp below th^2 = 2.5e-3: 1.28 on both.  log(exp(xi)) through both functions: 4.00 on both.

se3_exp inside the band 1e-6 <= th < 1e-2 before its coefficient b was rewritten as sin^2 / (th^2 (1 + cos)): host 191 917 units
(4.3e-11 |upsilon|, at th = 1e-6 (1 + 1e-9)) where 8 are allowed - what test_se3_exp_inside_the_cancellation_band[se3_exp-host] fails with on
the older header; outside the band the older form measured 16.5 (at th = 1.3e-2), now 2.0.
"""
import functools

import mpmath as mp
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from tests.helpers import devmath_probe
from tests.helpers.so3_cases import quat_case

mp.mp.dps = 50
EPS = 2.0 ** -52
PI = float(np.pi)

# worst scaled error of the host compile outside the band, in units of 2^-52 (measured; see the table above)
HOST_WORST = {
    "R_to_quat": 1.0,
    "quat_to_R": 1.5,
    "rotvec_to_R": 2.5,
    "R_to_rotvec": 4.0,
    "rot_angle": 2.0,
    "rt_project": 2.0,
    "mat3_polar": 1.5,
    "se3_exp": 2.0,
    "se3_exp_gn": 2.0,
    "se3_log": 2.0,
    "rt_inv": 0.96,
    "rt_mul": 1.01,
    "mat4_inv": 1.78,
    "solve6_ldlt": 2.0,
}
BAND = (1e-6, 1e-2)


def bound(name):
    return 4.0 * HOST_WORST[name] * EPS


@pytest.fixture(scope="session")
def probe(tmp_path_factory):
    return devmath_probe.build(tmp_path_factory.mktemp("devmath_probe"))


# ------------------------------------------------------------------------------------------------ mpmath references

def mpv(x):
    return [mp.mpf(float(v)) for v in x]


def mp_hat(w):
    z = mp.mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def mp_mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def mp_mv(A, v):
    return [sum(A[i][k] * v[k] for k in range(len(v))) for i in range(len(A))]


def mp_T(A):
    return [list(r) for r in zip(*A)]


def mp_abc(th):
    """R = I + a K + b K^2, V = I + b K + c K^2 (closed forms; at 50 digits the cancellation at th = 1e-12 leaves 25)."""
    if th == 0:
        return mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
    return mp.sin(th) / th, (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3


def mp_exp_so3(w, with_V=False):
    w = mpv(w)
    th = mp.sqrt(sum(x * x for x in w))
    a, b, c = mp_abc(th)
    K = mp_hat(w)
    K2 = mp_mm(K, K)
    eye = [[mp.mpf(int(i == j)) for j in range(3)] for i in range(3)]
    R = [[eye[i][j] + a * K[i][j] + b * K2[i][j] for j in range(3)] for i in range(3)]
    if not with_V:
        return R
    return R, [[eye[i][j] + b * K[i][j] + c * K2[i][j] for j in range(3)] for i in range(3)]


def mp_quat(w):
    """unit quaternion xyzw of the rotation vector w"""
    w = mpv(w)
    th = mp.sqrt(sum(x * x for x in w))
    s = mp.mpf(1) / 2 if th == 0 else mp.sin(th / 2) / th
    return [s * w[0], s * w[1], s * w[2], mp.cos(th / 2)]


def mp_quat_to_R(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def mp_project(R9):
    """The rotation of scipy's matrix-to-quaternion rule applied to a 3x3 that need not be orthogonal, exactly."""
    M = [[mp.mpf(float(R9[3 * i + j])) for j in range(3)] for i in range(3)]
    tr = M[0][0] + M[1][1] + M[2][2]
    d = [M[0][0], M[1][1], M[2][2]]
    i = max(range(3), key=lambda k: (d[k], -k))
    q = [None] * 4
    if tr > d[i]:
        q = [M[2][1] - M[1][2], M[0][2] - M[2][0], M[1][0] - M[0][1], 1 + tr]
    else:
        j, k = (i + 1) % 3, (i + 2) % 3
        q[i] = 1 - tr + 2 * M[i][i]
        q[j] = M[j][i] + M[i][j]
        q[k] = M[k][i] + M[i][k]
        q[3] = M[k][j] - M[j][k]
    n = mp.sqrt(sum(x * x for x in q))
    return mp_quat_to_R([x / n for x in q])


def flat(M):
    return [float(x) for r in M for x in r]


def fl(v):
    return [float(x) for x in v]


# ------------------------------------------------------------------------------------------------ inputs (fixed seeds)

def unit(v):
    return v / np.linalg.norm(v)


AXES6 = [np.array(a, float) for a in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])]
NEAR_PI = [PI - e for e in (0.0, 1e-15, 1e-12, 1e-9, 1e-6, 1e-3)]


def switch_angles():
    """at and on both sides of every switch of the header, plus the worst points of the old cancellation band"""
    out = []
    for s in (1e-3, 1e-6, float(np.sqrt(2.5e-3))):
        out += [s * f for f in (0.9, 1 - 1e-9, 1.0, 1 + 1e-9, 1.1)]
    return out + [1.1e-6, 2e-6, 5e-6]


def sweep_angles():
    return [float(a) for a in 10.0 ** np.arange(-12, np.log10(PI), 1.0 / 8)] + [PI]


@functools.lru_cache(maxsize=None)
def rotvecs():
    """(n, 3): angles uniform in [0, pi] about random axes and about +-x, +-y, +-z; the grid near pi; every switch; the sweep"""
    rng = np.random.default_rng(20260101)
    v = [unit(rng.normal(size=3)) * a for a in rng.uniform(0, PI, 2400)]
    v += [ax * a for ax in AXES6 for a in rng.uniform(0, PI, 150)]
    for a in NEAR_PI + switch_angles() + sweep_angles():
        v += [unit(rng.normal(size=3)) * a for _ in range(4)] + [ax * a for ax in AXES6]
    v.append(np.zeros(3))
    return np.array(v)


def is_flip_ambiguous(v):
    """the rotation is within rounding of a half turn: +axis and -axis describe it equally well"""
    return PI - np.linalg.norm(v, axis=-1) < 1e-14


@functools.lru_cache(maxsize=None)
def rot_ref():
    """the double rotation matrices (rounded from the exact ones) of rotvecs(), and their exact quaternions"""
    V = rotvecs()
    R = np.array([flat(mp_exp_so3(v)) for v in V])
    q = np.array([fl(mp_quat(v)) for v in V])
    return R, q


@functools.lru_cache(maxsize=None)
def twists():
    """(n, 6) Sophus order (upsilon, omega): the sweep, the switches and the grid near pi; |upsilon| from 0.1 to 100 m"""
    rng = np.random.default_rng(20260102)
    xi = []
    for a in sweep_angles() + switch_angles() + NEAR_PI[2:]:
        for ax in [unit(rng.normal(size=3)) for _ in range(3)] + [AXES6[rng.integers(6)]]:
            for un in (0.1, 2.0, 10.0, 100.0):
                xi.append(np.concatenate([unit(rng.normal(size=3)) * un, ax * a]))
    xi.append(np.array([1.0, -2.0, 3.0, 0, 0, 0]))
    return np.array(xi)


def th_of(xi):
    w = xi[:, 3:]
    return np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])


def in_band(th):
    return (th >= BAND[0]) & (th < BAND[1])


@functools.lru_cache(maxsize=None)
def exp_ref():
    out = []
    for x in twists():
        R, V = mp_exp_so3(x[3:], with_V=True)
        out.append(flat(R) + fl(mp_mv(V, mpv(x[:3]))))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def log_cases():
    """T = (rounded exact rotation of w, t) -> xi = (V(w)^-1 t, w); t is what the caller has, so it is the scale"""
    X = twists()
    X = X[~is_flip_ambiguous(X[:, 3:])]
    T, ref = [], []
    for x in X:
        R, V = mp_exp_so3(x[3:], with_V=True)
        u = mp.lu_solve(mp.matrix(V), mp.matrix(mpv(x[:3])))
        T.append(flat(R) + list(x[:3]))
        ref.append(fl(u) + list(x[3:]))
    return np.array(T), np.array(ref), np.linalg.norm(X[:, :3], axis=1), th_of(X)


@functools.lru_cache(maxsize=None)
def perturbed():
    """rotations times (I + E), |E| = 1e-12 .. 1e-6, with a translation: what a chain of fp64 products or a caller's raw guess is"""
    rng = np.random.default_rng(20260103)
    R, _ = rot_ref()
    pick = rng.choice(len(R), 600, replace=False)
    A = []
    for n, i in enumerate(pick):
        E = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-12, -6)
        A.append(np.concatenate([((np.eye(3) + E) @ R[i].reshape(3, 3)).ravel(), rng.normal(size=3) * 10.0 ** (n % 4)]))
    return np.array(A)


@functools.lru_cache(maxsize=None)
def rigid_pairs():
    rng = np.random.default_rng(20260104)
    R, _ = rot_ref()
    i, j = rng.choice(len(R), 500), rng.choice(len(R), 500)
    ta = rng.normal(size=(500, 3)) * 10.0 ** rng.integers(-1, 4, (500, 1))
    tb = rng.normal(size=(500, 3)) * 10.0 ** rng.integers(-1, 4, (500, 1))
    return np.hstack([R[i], ta, R[j], tb])


@functools.lru_cache(maxsize=None)
def mat4_cases():
    """rigid poses with translations up to kilometres (the raw guess of a registration), and general 4x4 up to cond 1e8"""
    rng = np.random.default_rng(20260105)
    R, _ = rot_ref()
    A = []
    for n in range(300):
        T = np.eye(4)
        T[:3, :3] = R[rng.integers(len(R))].reshape(3, 3)
        T[:3, 3] = rng.normal(size=3) * 10.0 ** (n % 5)
        A.append(T.ravel())
    for n in range(300):
        U, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        W, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        A.append((U @ np.diag(10.0 ** -np.linspace(0, (n % 9), 4)) @ W).ravel())
    return np.array(A)


def pack27(A, b):
    return np.concatenate([A[np.triu_indices(6)], b])


@functools.lru_cache(maxsize=None)
def solve_cases():
    """JTJ dx = -JTr, packed as the kernels sum it: SPD with condition numbers 1 .. 1e10"""
    rng = np.random.default_rng(20260106)
    S, cond = [], []
    for n in range(440):
        e = n % 11
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        A = Q @ np.diag(10.0 ** np.linspace(0, -e, 6)) @ Q.T
        A = 0.5 * (A + A.T) * 10.0 ** rng.uniform(-2, 6)
        S.append(pack27(A, rng.normal(size=6) * 10.0 ** rng.uniform(-3, 3)))
        cond.append(10.0 ** e)
    return np.array(S), np.array(cond)


def unpack27(s):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    return A + np.triu(A, 1).T, s[21:]


# ------------------------------------------------------------------------------------------------ comparison

def scaled_err(out, ref, scale=1.0, alt=None):
    """(n,) worst absolute error per input over its outputs, divided by scale; alt: a second admissible reference"""
    e = np.abs(out - ref).max(1)
    if alt is not None:
        e = np.minimum(e, np.abs(out - alt).max(1))
    assert not np.isnan(out).any()
    return e / scale


def check(name, side, err, where=""):
    worst = float(err.max())
    print(f"devmath {name:12s} {side:7s} {where:8s} worst {worst / EPS:9.2f} x 2^-52 at input {int(err.argmax())} (bound {4 * HOST_WORST[name]:.1f})")
    assert worst <= bound(name), (name, side, where, worst / EPS, int(err.argmax()))


def both_sides(th, s, rel=1e-6):
    """inputs within rel of the switch s on either side, and exactly representable neighbours further out"""
    return (((th < s) & (th > s * (1 - rel))).any() and ((th >= s) & (th < s * (1 + rel))).any()
            and (th < 0.95 * s).any() and (th > 1.05 * s).any())


SIDES = ["host", pytest.param("device", marks=pytest.mark.gpu)]


def run_pair(probe, name, side, x):
    """the side under test, and the host's result when the device is under test (for the per-input comparison)"""
    out = probe.run(name, side, x)
    return out, (probe.run(name, "host", x) if side == "device" else None)


# ------------------------------------------------------------------------------------------------ coverage of the inputs

def test_inputs_take_every_branch():
    R, _ = rot_ref()
    n = np.bincount(quat_case(R), minlength=4)
    assert (n >= 100).all(), n
    # scipy agrees on which rotations these are
    q = Rotation.from_matrix(R[:50].reshape(-1, 3, 3)).as_quat()
    assert q.shape == (50, 4)
    a = np.linalg.norm(rotvecs(), axis=1)  # axis * angle: the norm is the angle to a rounding
    assert both_sides(a, 1e-3) and (a == 0).any() and (np.abs(a - PI) < 4 * EPS).any()
    for e in (1e-15, 1e-12, 1e-9, 1e-6, 1e-3):
        assert (np.abs(a - (PI - e)) < 4 * EPS).any()
    assert (a > np.radians(120)).sum() > 1000
    th = th_of(twists())
    assert both_sides(th, 1e-6) and both_sides(th, 1e-3) and both_sides(th * th, 2.5e-3)
    assert in_band(th).sum() > 400
    assert th.min() == 0 and 0 < np.sort(th)[1] <= 1.001e-12 and abs(th.max() - PI) < 4 * EPS
    assert np.linalg.norm(twists()[:, :3], axis=1).max() >= 100.0 - 1e-9


def test_reference_agrees_with_matrix_exponential():
    """the Rodrigues / V closed forms used as reference are the SE(3) exponential: mpmath's Taylor expm of the 4x4 twist matrix"""
    X = twists()
    for x in X[:: len(X) // 40]:
        M = mp.zeros(4)
        K = mp_hat(mpv(x[3:]))
        for i in range(3):
            for j in range(3):
                M[i, j] = K[i][j]
            M[i, 3] = mp.mpf(float(x[i]))
        E = mp.expm(M, method="taylor")
        R, V = mp_exp_so3(x[3:], with_V=True)
        t = mp_mv(V, mpv(x[:3]))
        d = max(max(abs(E[i, j] - R[i][j]) for i in range(3) for j in range(3)), max(abs(E[i, 3] - t[i]) for i in range(3)))
        assert d < mp.mpf(10) ** -40 * max(1, np.linalg.norm(x[:3])), (x, d)


# ------------------------------------------------------------------------------------------------ SO(3)

@pytest.mark.parametrize("side", SIDES)
def test_R_to_quat(probe, side):
    R, q = rot_ref()
    out, host = run_pair(probe, "R_to_quat", side, R)
    err = scaled_err(out, q, alt=-q)
    for c in range(4):
        check("R_to_quat", side, err[quat_case(R) == c], f"case {c}")
    sq = Rotation.from_matrix(R.reshape(-1, 3, 3)).as_quat()
    check("R_to_quat", side, scaled_err(out, sq, alt=-sq), "scipy")
    if host is not None:
        check("R_to_quat", "dev-host", scaled_err(out, host))


@pytest.mark.parametrize("side", SIDES)
def test_quat_to_R(probe, side):
    _, q = rot_ref()
    ref = np.array([flat(mp_quat_to_R(mpv(x))) for x in q])  # of the double quaternion, |q| = 1 to rounding
    out, host = run_pair(probe, "quat_to_R", side, q)
    check("quat_to_R", side, scaled_err(out, ref))
    if host is not None:
        check("quat_to_R", "dev-host", scaled_err(out, host))


@pytest.mark.parametrize("side", SIDES)
def test_rotvec_to_R(probe, side):
    R, _ = rot_ref()
    out, host = run_pair(probe, "rotvec_to_R", side, rotvecs())
    check("rotvec_to_R", side, scaled_err(out, R))
    if host is not None:
        check("rotvec_to_R", "dev-host", scaled_err(out, host))


@pytest.mark.parametrize("side", SIDES)
def test_R_to_rotvec_and_rot_angle(probe, side):
    R, _ = rot_ref()
    V = rotvecs()
    a = np.linalg.norm(V, axis=1)
    # within rounding of a half turn the other axis with angle 2 pi - a is the same rotation
    amb = is_flip_ambiguous(V)
    alt = V.copy()
    alt[amb] = -V[amb] / a[amb, None] * (2 * PI - a[amb, None])
    out, host = run_pair(probe, "R_to_rotvec", side, R)
    err = scaled_err(out, V, alt=alt)
    for c in range(4):
        check("R_to_rotvec", side, err[quat_case(R) == c], f"case {c}")
    assert (np.linalg.norm(out, axis=1) <= PI + 4 * EPS).all()  # the w < 0 flip keeps the angle in [0, pi]
    if host is not None:
        # at a half turn the sign of w is rounding: compare the rotations there, the vectors elsewhere
        check("R_to_rotvec", "dev-host", np.minimum(scaled_err(out, host), np.where(amb, scaled_err(out, -host), np.inf)))
    out, host = run_pair(probe, "rot_angle", side, R)
    check("rot_angle", side, scaled_err(out, np.minimum(a, 2 * PI - a)[:, None]))
    if host is not None:
        check("rot_angle", "dev-host", scaled_err(out, host))


@pytest.mark.parametrize("side", SIDES)
def test_rt_project_and_mat3_polar(probe, side):
    A = perturbed()
    R, _ = rot_ref()
    x = np.vstack([A, np.hstack([R[::7], np.ones((len(R[::7]), 3))])])
    assert (np.bincount(quat_case(x[:, :9]), minlength=4) >= 100).all()
    ref = np.array([flat(mp_project(r[:9])) + list(r[9:]) for r in x])
    out, host = run_pair(probe, "rt_project", side, x)
    check("rt_project", side, scaled_err(out, ref))
    assert np.array_equal(out[:, 9:], x[:, 9:])  # the translation passes through
    if host is not None:
        check("rt_project", "dev-host", scaled_err(out, host))
    # orthogonal polar factor U V^T from the SVD
    ref = []
    for r in A:
        U, _, Vt = mp.svd_r(mp.matrix([[mp.mpf(float(r[3 * i + j])) for j in range(3)] for i in range(3)]))
        Q = U * Vt
        ref.append([float(Q[i, j]) for i in range(3) for j in range(3)])
    out, host = run_pair(probe, "mat3_polar", side, A[:, :9])
    check("mat3_polar", side, scaled_err(out, np.array(ref)))
    if host is not None:
        check("mat3_polar", "dev-host", scaled_err(out, host))


# ------------------------------------------------------------------------------------------------ SE(3)

def exp_err(out, ref, X):
    """rotation entries absolute, translation relative to |upsilon|"""
    un = np.linalg.norm(X[:, :3], axis=1)
    return np.maximum(scaled_err(out[:, :9], ref[:, :9]), scaled_err(out[:, 9:], ref[:, 9:], un))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("name", ["se3_exp", "se3_exp_gn"])
def test_se3_exp_outside_the_band(probe, side, name):
    X, ref = twists(), exp_ref()
    m = ~in_band(th_of(X))
    out, host = run_pair(probe, name, side, X)
    check(name, side, exp_err(out, ref, X)[m], "outside")
    if host is not None:
        check(name, "dev-host", exp_err(out, host, X)[m], "outside")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("name", ["se3_exp", "se3_exp_gn"])
def test_se3_exp_inside_the_cancellation_band(probe, side, name):
    """1e-6 <= th < 1e-2: (1 - cos th) / th^2 has lost up to four digits there, and b K upsilon carries it into the translation -
    2.0e-10 m at th = 1.1e-6, |upsilon| = 2 m, in the deskew table of every sweep.  Same bound as everywhere else."""
    X, ref = twists(), exp_ref()
    m = in_band(th_of(X))
    out, host = run_pair(probe, name, side, X)
    check(name, side, exp_err(out, ref, X)[m], "band")
    if host is not None:
        check(name, "dev-host", exp_err(out, host, X)[m], "band")


@pytest.mark.parametrize("side", SIDES)
def test_se3_exp_gn_is_se3_exp_below_its_switch(probe, side):
    """devmath.h said 'differs from se3_exp() by rounding only (<= 1e-16 in R and t)'.  By rounding that is false: each of the two is
    within 2 x 2^-52 of the exact value (table above), so they are within 4 x 2^-52 max(1, |upsilon|) of each other - the bound here,
    and what the comment now says; measured 1.3 x 2^-52 (2.9e-16) on the host."""
    X = twists()
    X = X[th_of(X) ** 2 < 2.5e-3]
    d = np.abs(probe.run("se3_exp_gn", side, X) - probe.run("se3_exp", side, X))
    un = np.maximum(1.0, np.linalg.norm(X[:, :3], axis=1))
    worst = np.maximum(d[:, :9].max(1), d[:, 9:].max(1) / un)
    print(f"devmath se3_exp_gn - se3_exp {side}: worst {worst.max() / EPS:.2f} x 2^-52")
    assert worst.max() <= (HOST_WORST["se3_exp"] + HOST_WORST["se3_exp_gn"]) * EPS


@pytest.mark.parametrize("side", SIDES)
def test_se3_log(probe, side):
    T, ref, tn, th = log_cases()
    out, host = run_pair(probe, "se3_log", side, T)

    def err(o, r):
        return np.maximum(scaled_err(o[:, :3], r[:, :3], tn), scaled_err(o[:, 3:], r[:, 3:]))

    check("se3_log", side, err(out, ref)[~in_band(th)], "outside")
    check("se3_log", side, err(out, ref)[in_band(th)], "band")
    if host is not None:
        check("se3_log", "dev-host", err(out, host))


@pytest.mark.parametrize("side", SIDES)
def test_se3_log_of_exp_round_trip(probe, side):
    """log(exp(xi)) = xi through both functions of the same compile, the figure the accuracy hole was found with"""
    X = twists()
    X = X[~is_flip_ambiguous(X[:, 3:])]
    back = probe.run("se3_log", side, probe.run("se3_exp", side, X))
    un = np.linalg.norm(X[:, :3], axis=1)
    err = np.maximum(scaled_err(back[:, :3], X[:, :3], un), scaled_err(back[:, 3:], X[:, 3:]))
    worst = float(err.max())
    print(f"devmath log(exp) {side}: worst {worst / EPS:.2f} x 2^-52")
    assert worst <= bound("se3_exp") + bound("se3_log")


@pytest.mark.parametrize("side", SIDES)
def test_rt_inv_and_rt_mul(probe, side):
    P = rigid_pairs()
    A = P[:, :12]
    ref = []
    for r in A:
        Rt_ = mp_T([mpv(r[0:3]), mpv(r[3:6]), mpv(r[6:9])])
        ref.append(flat(Rt_) + [-float(x) for x in mp_mv(Rt_, mpv(r[9:]))])
    ref = np.array(ref)
    ta, tb = np.linalg.norm(P[:, 9:12], axis=1), np.linalg.norm(P[:, 21:24], axis=1)
    out, host = run_pair(probe, "rt_inv", side, A)
    assert np.array_equal(out[:, :9], ref[:, :9])  # a transpose is exact
    check("rt_inv", side, scaled_err(out[:, 9:], ref[:, 9:], ta))
    if host is not None:
        check("rt_inv", "dev-host", scaled_err(out[:, 9:], host[:, 9:], ta))
    ref = []
    for r in P:
        Ra, Rb = [mpv(r[0:3]), mpv(r[3:6]), mpv(r[6:9])], [mpv(r[12:15]), mpv(r[15:18]), mpv(r[18:21])]
        t = [x + y for x, y in zip(mp_mv(Ra, mpv(r[21:24])), mpv(r[9:12]))]
        ref.append(flat(mp_mm(Ra, Rb)) + fl(t))
    ref = np.array(ref)
    out, host = run_pair(probe, "rt_mul", side, P)

    def err(o, r):
        return np.maximum(scaled_err(o[:, :9], r[:, :9]), scaled_err(o[:, 9:], r[:, 9:], ta + tb))

    check("rt_mul", side, err(out, ref))
    if host is not None:
        check("rt_mul", "dev-host", err(out, host))


# ------------------------------------------------------------------------------------------------ inverses and solves

@pytest.mark.parametrize("side", SIDES)
def test_mat4_inv(probe, side):
    A = mat4_cases()
    ref = np.array([[float(v) for v in mp.inverse(mp.matrix(a.reshape(4, 4).tolist()))] for a in A])
    scale = np.array([np.linalg.cond(a.reshape(4, 4)) for a in A]) * np.abs(ref).max(1)
    out, host = run_pair(probe, "mat4_inv", side, A)
    assert (out[:, 16] == 1.0).all()
    check("mat4_inv", side, scaled_err(out[:, :16], ref, scale))
    if host is not None:
        check("mat4_inv", "dev-host", scaled_err(out[:, :16], host[:, :16], scale))
    # a singular matrix gives the identity and false: a zero matrix, a zero row, two equal rows
    S = np.zeros((3, 16))
    S[1] = np.diag([1.0, 2.0, 0.0, 1.0]).ravel()
    S[2] = np.array([[1, 2, 3, 4], [1, 2, 3, 4], [0, 1, 0, 0], [0, 0, 1, 0]], float).ravel()
    out = probe.run("mat4_inv", side, S)
    assert np.array_equal(out, np.tile(np.concatenate([np.eye(4).ravel(), [0.0]]), (3, 1)))


@pytest.mark.parametrize("side", SIDES)
def test_solve6_ldlt(probe, side):
    S, cond = solve_cases()
    ref = []
    for s in S:
        A, b = unpack27(s)
        ref.append(fl(mp.lu_solve(mp.matrix(A.tolist()), -mp.matrix(b.tolist()))))
    ref = np.array(ref)
    scale = cond * np.abs(ref).max(1)
    out, host = run_pair(probe, "solve6_ldlt", side, S)
    check("solve6_ldlt", side, scaled_err(out, ref, scale))
    if host is not None:
        check("solve6_ldlt", "dev-host", scaled_err(out, host, scale))
    # the all-zero system of a scan without pairs, and a zero pivot: that component is zero, the others solve the rest
    rng = np.random.default_rng(20260107)
    Z = [np.zeros(27)]
    want = [np.zeros(6)]
    for j in range(6):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        A = Q @ np.diag(rng.uniform(1, 10, 6)) @ Q.T
        A = 0.5 * (A + A.T)
        b = rng.normal(size=6)
        A[j, :] = A[:, j] = 0.0
        b[j] = 0.0
        keep = [k for k in range(6) if k != j]
        x = np.zeros(6)
        x[keep] = fl(mp.lu_solve(mp.matrix(A[np.ix_(keep, keep)].tolist()), -mp.matrix(b[keep].tolist())))
        Z.append(pack27(A, b))
        want.append(x)
    out = probe.run("solve6_ldlt", side, np.array(Z))
    want = np.array(want)
    assert np.array_equal(out[0], np.zeros(6))
    for j in range(6):
        assert out[1 + j, j] == 0.0
    check("solve6_ldlt", side, scaled_err(out, want, 10.0 * np.maximum(np.abs(want).max(1), 1e-300)), "pivot")
