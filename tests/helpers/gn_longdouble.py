"""One Gauss-Newton step of the registration restated in numpy.longdouble (x87 80-bit: 64-bit significand) and, for the 6x6 algebra,
mpmath at 200 bits: the reference the scenes of tests/helpers/gn_step_scenes.py are held against.

Written from the rule in the header of csrc/icp_kernels.h and from Registration.cpp's meaning (r = s - t, J = [I | -hat(s)],
w = k^2 / (k + |r|^2)^2, dx = solve(JTJ, -JTr), T <- Exp(dx) T), not from the kernels' or the C oracle's code: the inputs are exactly the fp64
inputs of the call under test (source points, guess, the map's stored points in export order, max_dist, kernel, voxel size) and everything
that is rounded on the way is rounded to 64 bits of significand or better.

  correspondences  the voxel of a source point is (int)(x / voxel) of its fp64 position (an integer decision, shared with every
                   implementation; the guard below keeps it from depending on rounding); candidates are the stored points of the 27 voxels
                   around it, voxels in (i, j, k) ascending order, points in insertion order; distances in long double (among the candidates within
                   1 mm of the nearest by their fp64 distance: the others cannot win); strictly smaller wins; a pair needs d < max_dist
  guard            per source point: nearest vs second-nearest candidate distance, nearest distance vs the gate, distance to the nearest
                   voxel face (every multiple of the voxel size counts as a face: conservative at 0, where truncation has none)
  system           the 21 + 6 sums in the packed order of the implementations (upper triangle row by row, then JTr), the 16 moments of the
                   8-lane kernel (W | W s | xx xy xz yy yz zz | sum w r | sum w s x r), and an absolute-value shadow of each: the same
                   formula with every subtraction replaced by an addition of magnitudes (s - t -> |s| + |t|, the cross product, -hat(s)).
                   The weight keeps its value in the shadow: given r it is a quotient of positive numbers, and r = s - t is one
                   correctly rounded operation on fp64 inputs in every implementation
  solve            Gaussian elimination with full pivoting at 200 bits on the long-double sums; cond(JTJ) from its eigenvalues; the
                   numerical rank from the eigenvalues of the system re-centred on the weighted centroid of the sources and scaled to a
                   unit diagonal (a congruence: the rank is the geometry's, the conditioning an offset from the origin adds is not), with
                   2^-40 of the largest as zero; below rank 6 the minimum-norm solution and a null-space basis (original coordinates)
  Exp, as_se3      Sophus order (upsilon, omega), closed forms at 200 bits; as_se3 is what a Sophus SE3d holds of a 4x4 (Eigen's matrix ->
                   quaternion branches, normalised), as oracle/icp_numpy.py::as_se3 does in fp64
  step error E     max_i |T p_i - T_ref p_i| over the source points, metres
"""
import mpmath as mp
import numpy as np

LD = np.longdouble
# a restatement no wider than the code under test is not a reference: fail here, do not skip
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not wider than fp64 on this machine"

PREC = 200            # bits of the 6x6 algebra, Exp and as_se3
RANK_TOL = 2.0 ** -40  # of the largest eigenvalue of the centred, unit-diagonal system (long-double sums of 3 000 terms carry 2^-52)
U = 2.0 ** -53
PREFILTER = 1e-3      # metres: candidates farther than this beyond the fp64 nearest are not looked at in long double

_OFFS = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.int64)
# packed upper triangle: entry (a, b), a <= b, at a (11 - a) / 2 + b
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]


# ------------------------------------------------------------------------------------------------ long double <-> mpmath
def to_mp(x):
    """exact: a long double is the sum of two doubles"""
    x = LD(x)
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


def from_mp(m):
    hi = float(m)
    return LD(hi) + LD(float(m - mp.mpf(hi)))


def mat_to_mp(A):
    A = np.asarray(A)
    return mp.matrix([[to_mp(A[i, j]) for j in range(A.shape[1])] for i in range(A.shape[0])])


def mat_from_mp(M):
    return np.array([[from_mp(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], dtype=LD)


# ------------------------------------------------------------------------------------------------ SE(3) at 200 bits
def _hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def exp_se3(dx):
    """4x4 long double of Exp((upsilon, omega)): R = I + sin t / t K + (1 - cos t) / t^2 K^2, V = I + (1 - cos t) / t^2 K + (t - sin t) / t^3 K^2"""
    with mp.workprec(PREC):
        v = mp.matrix([to_mp(x) for x in dx[:3]])
        w = [to_mp(x) for x in dx[3:]]
        t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        t = mp.sqrt(t2)
        K = _hat(w)
        I = mp.eye(3)
        if t == 0:
            R, V = I, I
        else:
            A, B, Cc = mp.sin(t) / t, (1 - mp.cos(t)) / t2, (t - mp.sin(t)) / (t2 * t)
            R = I + A * K + B * (K * K)
            V = I + B * K + Cc * (K * K)
        T = mp.eye(4)
        T[:3, :3] = R
        T[:3, 3] = V * v
        return mat_from_mp(T)


def log_se3(T):
    """(upsilon, omega) of a 4x4 long double rigid transform, the inverse of exp_se3 (angles below pi)"""
    with mp.workprec(PREC):
        M = mat_to_mp(np.asarray(T, dtype=LD))
        R = M[:3, :3]
        q = _quat_of(R)
        if q[3] < 0:
            q = [-x for x in q]
        n = mp.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
        ang = 2 * mp.atan2(n, q[3])
        w = [mp.mpf(0)] * 3 if n == 0 else [ang * x / n for x in q[:3]]
        K = _hat(w)
        I = mp.eye(3)
        if ang == 0:
            Vi = I
        else:
            Vi = I - K / 2 + (1 / ang ** 2 - (1 + mp.cos(ang)) / (2 * ang * mp.sin(ang))) * (K * K)
        u = Vi * M[:3, 3]
        return np.array([from_mp(u[i]) for i in range(3)] + [from_mp(x) for x in w], dtype=LD)


def _quat_of(m):
    """Eigen's matrix -> quaternion (x, y, z, w), normalised: positive trace, otherwise the branch of the largest diagonal entry"""
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    q = [mp.mpf(0)] * 4
    if tr > 0:
        t = mp.sqrt(tr + 1)
        q[3] = t / 2
        t = 1 / (2 * t)
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = mp.sqrt(m[i, i] - m[j, j] - m[k, k] + 1)
        q[i] = t / 2
        t = 1 / (2 * t)
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    n = mp.sqrt(sum(x * x for x in q))
    return [x / n for x in q]


def as_se3(T):
    """what a Sophus SE3d holds of the fp64 4x4 `T`: the rotation of the normalised quaternion of its 3x3 block, and its translation"""
    with mp.workprec(PREC):
        M = mat_to_mp(np.asarray(T, dtype=LD))
        x, y, z, w = _quat_of(M[:3, :3])
        out = mp.eye(4)
        out[:3, :3] = mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        out[:3, 3] = M[:3, 3]
        return mat_from_mp(out)


def mul(A, B):
    """4x4 product at 200 bits"""
    with mp.workprec(PREC):
        return mat_from_mp(mat_to_mp(A) * mat_to_mp(B))


def inv_rigid(T):
    with mp.workprec(PREC):
        M = mat_to_mp(np.asarray(T, dtype=LD))
        out = mp.eye(4)
        out[:3, :3] = M[:3, :3].T
        out[:3, 3] = -(M[:3, :3].T * M[:3, 3])
        return mat_from_mp(out)


def apply(T, p):
    """T p for (N, 3) points, in long double"""
    T = np.asarray(T, dtype=LD)
    p = np.asarray(p, dtype=LD)
    return p @ T[:3, :3].T + T[:3, 3]


def step_error(T, T_ref, pts):
    """dict(E, dt, dr): E = max_i |T p_i - T_ref p_i| (metres); the translation and rotation-angle parts of T_ref^-1 T beside it"""
    a, b = apply(T, pts), apply(T_ref, pts)
    d = a - b
    E = float(np.sqrt((d * d).sum(axis=1)).max()) if len(d) else 0.0
    D = mul(inv_rigid(T_ref), np.asarray(T, dtype=LD))
    xi = log_se3(D)
    return dict(E=E, dt=float(np.sqrt((D[:3, 3] ** 2).sum())), dr=float(np.sqrt((xi[3:] ** 2).sum())))


# ------------------------------------------------------------------------------------------------ the map as a table
def _code(k):
    off = 1 << 20
    return ((k[..., 0] + off) << 42) | ((k[..., 1] + off) << 21) | (k[..., 2] + off)


def voxel_of(p, vs):
    return np.trunc(np.asarray(p, dtype=np.float64) / vs).astype(np.int64)  # (int)(x / vs) of the fp64 position


class MapTable:
    """the stored points (fp64, export order: insertion order within a voxel) binned by voxel: sorted voxel codes, a padded (M + 1, cap, 3)
    table with +inf beyond a voxel's points (row M: the absent voxel), counts"""

    def __init__(self, stored, vs, cap):
        stored = np.ascontiguousarray(stored, dtype=np.float64).reshape(-1, 3)
        self.vs, self.cap, self.n = float(vs), int(cap), len(stored)
        code = _code(voxel_of(stored, vs))
        order = np.argsort(code, kind="stable")
        self.code, first, cnt = np.unique(code[order], return_index=True, return_counts=True)
        assert cnt.max(initial=0) <= cap, "more stored points in a voxel than its capacity"
        rank = np.arange(len(order)) - np.repeat(first, cnt)
        row = np.repeat(np.arange(len(cnt)), cnt)
        self.pts = np.full((len(cnt) + 1, cap, 3), np.inf)
        self.pts[row, rank] = stored[order]
        self.cnt = np.concatenate([cnt, [0]]).astype(np.int64)


def correspondences(src_w, table, max_dist, chunk=256):
    """nearest stored point of every world-frame source point (long double or fp64, (N, 3)) and the guard quantities.
    dict(target (N, 3) fp64, NaN where unpaired; paired (N,) bool; found; d, d_second (long double; +inf if absent, d_second also
    if more than PREFILTER beyond the nearest); gap_second, gap_gate, face
    (fp64 metres); n_cand: stored points visited, summed over the sources)"""
    s = np.asarray(src_w, dtype=LD).reshape(-1, 3)
    n = len(s)
    s64 = s.astype(np.float64)
    vs = table.vs
    k0 = voxel_of(s64, vs)
    rows = np.empty((n, 27), dtype=np.int64)
    M = len(table.code)
    for o, off in enumerate(_OFFS):
        c = _code(k0 + off)
        pos = np.minimum(np.searchsorted(table.code, c), max(M - 1, 0))
        hit = (table.code[pos] == c) if M else np.zeros(n, bool)
        rows[:, o] = np.where(hit, pos, M)
    tgt = np.full((n, 3), np.nan)
    d1 = np.full(n, np.inf, dtype=LD)
    d2nd = np.full(n, np.inf, dtype=LD)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        cand = table.pts[rows[a:b]].reshape(b - a, -1, 3)          # (c, 27 cap, 3), visiting order
        # long double only where it can matter: the candidates within PREFILTER of the nearest by their fp64 distance (whose error, 1e-10 m
        # at coordinates of 1e5 m, is seven orders below it); every other candidate is farther than the guard's margin by a wide berth
        with np.errstate(invalid="ignore"):
            d64 = np.sqrt(((cand - s64[a:b, None, :]) ** 2).sum(axis=2))
        sel = d64 <= (d64.min(axis=1) + PREFILTER)[:, None]
        i, j = np.nonzero(sel)
        diff = cand[i, j].astype(LD) - s[a:b][i]
        q = np.full(d64.shape, np.inf, dtype=LD)
        q[i, j] = (diff * diff).sum(axis=1)
        best = np.argmin(q, axis=1)                                 # the FIRST of the smallest: strictly smaller wins
        ar = np.arange(b - a)
        qb = q[ar, best]
        ok = np.isfinite(qb.astype(np.float64))
        d1[a:b] = np.where(ok, np.sqrt(np.where(ok, qb, 0)), np.inf)
        tgt[a:b][ok] = cand[ar, best][ok]
        q[ar, best] = np.inf
        q2 = q.min(axis=1)
        ok2 = np.isfinite(q2.astype(np.float64))
        d2nd[a:b] = np.where(ok2, np.sqrt(np.where(ok2, q2, 0)), np.inf)
    found = np.isfinite(d1.astype(np.float64))
    paired = found & (d1 < LD(max_dist))
    tgt[~paired] = np.nan
    f = s64 / vs
    face = (np.minimum(f - np.floor(f), np.ceil(f) - f) * vs).min(axis=1) if n else np.zeros(0)
    with np.errstate(invalid="ignore"):
        gap_second = np.where(found, (d2nd - d1).astype(np.float64), np.inf)
        gap_gate = np.where(found, np.abs((d1 - LD(max_dist)).astype(np.float64)), np.inf)
    return dict(target=tgt, paired=paired, found=found, d=d1, d_second=d2nd, gap_second=gap_second, gap_gate=gap_gate, face=face,
                n_cand=int(table.cnt[rows].sum()))


def guard_fails(c, margin=1e-6):
    """(N,) bool: a decision of this point could flip under rounding: within `margin` of a voxel face, of the gate, or of a tie between the
    two nearest candidates (the tie matters only for a pair)"""
    return (c["face"] < margin) | (c["found"] & (c["gap_gate"] < margin)) | (c["paired"] & (c["gap_second"] < margin))


# ------------------------------------------------------------------------------------------------ the weighted system
def _sum(terms):
    """sum over the pairs, (n, m) -> (m,): pairwise along the contiguous axis"""
    return np.ascontiguousarray(terms.T).sum(axis=1) if len(terms) else np.zeros(terms.shape[1], dtype=LD)


def system(src_w, target, paired, kernel):
    """the sums of the paired points.  dict(n_pairs; sums (27,), shadow (27,), moments (16,), moments_shadow (16,): long double; w (n,))"""
    s = np.asarray(src_w, dtype=LD).reshape(-1, 3)[paired]
    t = np.asarray(target, dtype=LD).reshape(-1, 3)[paired]
    k = LD(kernel)
    r = s - t
    r_abs = np.abs(s) + np.abs(t)
    den = k + (r * r).sum(axis=1)
    w = k * k / (den * den)
    z = np.zeros(len(s), dtype=LD)
    o = np.ones(len(s), dtype=LD)
    x, y, zz = s[:, 0], s[:, 1], s[:, 2]
    cols = [np.stack(c, axis=1) for c in ((o, z, z), (z, o, z), (z, z, o), (z, -zz, y), (zz, z, -x), (-y, x, z))] + [r]
    cols_abs = [np.abs(c) for c in cols[:6]] + [r_abs]
    sums = _sum(np.stack([w * (cols[a] * cols[b]).sum(axis=1) for a, b in PAIRS] + [w * (cols[a] * cols[6]).sum(axis=1) for a in range(6)], axis=1))
    shadow = _sum(np.stack([w * (cols_abs[a] * cols_abs[b]).sum(axis=1) for a, b in PAIRS]
                           + [w * (cols_abs[a] * cols_abs[6]).sum(axis=1) for a in range(6)], axis=1))
    cr = np.cross(s, r)
    sa = np.abs(s)
    cr_abs = np.stack([sa[:, 1] * r_abs[:, 2] + sa[:, 2] * r_abs[:, 1], sa[:, 2] * r_abs[:, 0] + sa[:, 0] * r_abs[:, 2],
                       sa[:, 0] * r_abs[:, 1] + sa[:, 1] * r_abs[:, 0]], axis=1)

    def mom(S, R, Cx):
        return [o, S[:, 0], S[:, 1], S[:, 2], S[:, 0] * S[:, 0], S[:, 0] * S[:, 1], S[:, 0] * S[:, 2], S[:, 1] * S[:, 1], S[:, 1] * S[:, 2],
                S[:, 2] * S[:, 2], R[:, 0], R[:, 1], R[:, 2], Cx[:, 0], Cx[:, 1], Cx[:, 2]]
    moments = _sum(np.stack([w * m for m in mom(s, r, cr)], axis=1))
    moments_shadow = _sum(np.stack([w * np.abs(m) for m in mom(sa, r_abs, cr_abs)], axis=1))
    return dict(n_pairs=int(len(s)), sums=sums, shadow=shadow, moments=moments, moments_shadow=moments_shadow, w=w, s=s, t=t)


def sums_from_moments(M):
    """the 27 sums from the 16 moments (the identity the 8-lane kernel relies on)"""
    W, sx, sy, sz, xx, xy, xz, yy, yz, zz_ = M[:10]
    A = np.zeros((6, 6), dtype=LD)
    A[0, 0] = A[1, 1] = A[2, 2] = W
    A[0, 4], A[0, 5], A[1, 3], A[1, 5], A[2, 3], A[2, 4] = sz, -sy, -sz, sx, sy, -sx
    A[3, 3], A[3, 4], A[3, 5], A[4, 4], A[4, 5], A[5, 5] = yy + zz_, -xy, -xz, xx + zz_, -yz, xx + yy
    return np.array([A[a, b] for a, b in PAIRS] + list(M[10:16]), dtype=LD)


def unpack(sums):
    """(JTJ (6, 6), JTr (6,)) of 27 packed sums, dtype kept"""
    sums = np.asarray(sums)
    A = np.zeros((6, 6), dtype=sums.dtype)
    for o, (a, b) in enumerate(PAIRS):
        A[a, b] = A[b, a] = sums[o]
    return A, sums[21:27].copy()


def _full_pivot_solve(A, b):
    """mpmath 6x6: Gaussian elimination with full pivoting (rows and columns); the matrix is regular at the working precision"""
    n = 6
    M = [[A[i, j] for j in range(n)] + [b[i]] for i in range(n)]
    perm = list(range(n))
    for c in range(n):
        pv, pi, pj = -1, c, c
        for i in range(c, n):
            for j in range(c, n):
                if abs(M[i][j]) > pv:
                    pv, pi, pj = abs(M[i][j]), i, j
        if pv == 0:
            raise np.linalg.LinAlgError("singular system")
        M[c], M[pi] = M[pi], M[c]
        for row in M:
            row[c], row[pj] = row[pj], row[c]
        perm[c], perm[pj] = perm[pj], perm[c]
        for i in range(c + 1, n):
            f = M[i][c] / M[c][c]
            for j in range(c, n + 1):
                M[i][j] -= f * M[c][j]
    y = [mp.mpf(0)] * n
    for i in range(n - 1, -1, -1):
        y[i] = (M[i][n] - sum(M[i][j] * y[j] for j in range(i + 1, n))) / M[i][i]
    x = [mp.mpf(0)] * n
    for c in range(n):
        x[perm[c]] = y[c]
    return x


def solve(sysd):
    """dict(dx (6,) long double: the solution at rank 6, the minimum-norm solution below; cond; rank; minnorm; null (6, 6 - rank))
    of a system() result"""
    with mp.workprec(PREC):
        A, g = unpack(sysd["sums"])
        Am = mat_to_mp(A)
        bm = [-to_mp(x) for x in g]
        if sysd["n_pairs"] == 0:
            z = np.zeros(6, dtype=LD)
            return dict(dx=z, cond=float("inf"), rank=0, minnorm=z, null=np.eye(6, dtype=LD))
        # rank: the system about the weighted centroid, unit diagonal
        w, s = sysd["w"], sysd["s"]
        c = (w[:, None] * s).sum(axis=0) / w.sum()
        sc = s - c  # (the weights are those of the residuals: kept)
        z, o = np.zeros(len(s), dtype=LD), np.ones(len(s), dtype=LD)
        cols = [np.stack(q, axis=1) for q in ((o, z, z), (z, o, z), (z, z, o), (z, -sc[:, 2], sc[:, 1]), (sc[:, 2], z, -sc[:, 0]), (-sc[:, 1], sc[:, 0], z))]
        Ac = np.zeros((6, 6), dtype=LD)
        for a, b in PAIRS:
            Ac[a, b] = Ac[b, a] = (w * (cols[a] * cols[b]).sum(axis=1)).sum()
        dg = np.sqrt(np.where(np.diag(Ac) > 0, np.diag(Ac), 1))
        ev = sorted(abs(x) for x in mp.eigsy(mat_to_mp(Ac / np.outer(dg, dg)), eigvals_only=True))
        rank = int(sum(1 for x in ev if x > RANK_TOL * ev[-1]))
        E, Q = mp.eigsy(Am)
        lam = [E[i] for i in range(6)]
        idx = sorted(range(6), key=lambda i: abs(lam[i]))
        cond = float(abs(lam[idx[-1]]) / abs(lam[idx[0]])) if lam[idx[0]] != 0 else float("inf")
        keep, drop = idx[6 - rank:], idx[:6 - rank]
        mn = [mp.mpf(0)] * 6
        for i in keep:
            coef = sum(Q[r, i] * bm[r] for r in range(6)) / lam[i]
            for r in range(6):
                mn[r] += coef * Q[r, i]
        minnorm = np.array([from_mp(x) for x in mn], dtype=LD)
        null = np.array([[from_mp(Q[r, i]) for i in drop] for r in range(6)], dtype=LD).reshape(6, len(drop))
        dx = np.array([from_mp(x) for x in _full_pivot_solve(Am, bm)], dtype=LD) if rank == 6 else minnorm
        return dict(dx=dx, cond=cond, rank=rank, minnorm=minnorm, null=null)


def residual(sums_ref, dx):
    """|JTJ dx + JTr| (2-norm, fp64) of a long double system for somebody's step"""
    A, g = unpack(np.asarray(sums_ref, dtype=LD))
    v = A @ np.asarray(dx, dtype=LD) + g
    return float(np.sqrt((v * v).sum()))


# ------------------------------------------------------------------------------------------------ whole steps
def register(src_sensor, guess, table, max_dist, kernel, steps=1):
    """`steps` Gauss-Newton steps from the fp64 guess.  dict(pose (4, 4) long double = Exp(dx_k) .. Exp(dx_1) as_se3(guess); guess_se3;
    per step a dict(world: the sources the step searched from, corr, sys, sol, exp))"""
    g = as_se3(guess)
    world = apply(g, np.asarray(src_sensor, dtype=np.float64))
    T = g
    out = []
    for _ in range(steps):
        corr = correspondences(world, table, max_dist)
        sysd = system(world, corr["target"], corr["paired"], kernel)
        sol = solve(sysd)
        E = exp_se3(sol["dx"])
        out.append(dict(world=world, corr=corr, sys=sysd, sol=sol, exp=E))
        world = apply(E, world)
        T = mul(E, T)
    return dict(pose=T, guess_se3=g, steps=out)
