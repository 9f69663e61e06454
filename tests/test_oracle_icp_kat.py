"""Known-answer tests that pin the CPU oracle's ICP restatement algebraically (the reference holds no golden
vector for this part - kiss-icp is an absent third-party dependency - so parity there is 'unpinned'; these are the
pins available): exact-transform recovery, identity on a repeated scan, first scan returns the guess, nearest
neighbour against brute force, voxel semantics (first point wins, truncation toward zero, 20-point cap, pruning by
the first point), adaptive threshold state machine."""
import numpy as np

from oracle import cpu as orc


def _room(rng, n):
    L = np.array([40.0, 30.0, 10.0])
    pts = []
    for ax in range(3):
        for side in (0, 1):
            p = rng.uniform(0, 1, (n // 6, 3)) * L
            p[:, ax] = side * L[ax]
            pts.append(p)
    return np.vstack(pts) - L / 2


def test_se3_exp_log_roundtrip_and_reference_values():
    rng = np.random.default_rng(0)
    for _ in range(20):
        xi = rng.normal(0, 0.5, 6)
        T = orc.se3_exp(xi)
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-14
        assert np.abs(orc.se3_log(T) - xi).max() < 1e-12
    # pure translation / tiny rotation branches
    assert np.allclose(orc.se3_exp([1, 2, 3, 0, 0, 0])[:3, 3], [1, 2, 3])
    xi = np.array([0.1, 0.2, 0.3, 1e-9, -2e-9, 1e-9])
    assert np.abs(orc.se3_log(orc.se3_exp(xi)) - xi).max() < 1e-15
    from scipy.linalg import expm
    xi = np.array([0.3, -0.2, 0.5, 0.1, -0.4, 0.25])
    X = np.zeros((4, 4))
    X[:3, 3] = xi[:3]
    w = xi[3:]
    X[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    assert np.abs(expm(X) - orc.se3_exp(xi)).max() < 1e-15
    # 1e-6 <= th < 1e-2, where (1 - cos th) / th^2 used to put 1e-16 / th of |upsilon| into t (4e-11 of it at th = 1e-6; the device has
    # the same formula, so no comparison with it could see that): against the closed forms in mpmath at 50 digits, |upsilon| to 100 m,
    # at the bound tests/test_devmath_probe.py asks of csrc/devmath.h se3_exp (4 x its measured 2 x 2^-52)
    import mpmath as mp
    mp.mp.dps = 50
    worst = 0.0
    for th in [1e-6, 1.1e-6, 2e-6, 5e-6] + [float(a) for a in 10.0 ** np.arange(-6, -2, 0.125)] + [9.99e-3]:
        for un in (0.1, 2.0, 100.0):
            u, w = rng.normal(size=3), rng.normal(size=3)
            xi = np.concatenate([u / np.linalg.norm(u) * un, w / np.linalg.norm(w) * th])
            wm = [mp.mpf(float(v)) for v in xi[3:]]
            t = mp.sqrt(sum(v * v for v in wm))
            K = mp.matrix([[0, -wm[2], wm[1]], [wm[2], 0, -wm[0]], [-wm[1], wm[0], 0]])
            V = mp.eye(3) + (1 - mp.cos(t)) / t ** 2 * K + (t - mp.sin(t)) / t ** 3 * K * K
            R = mp.eye(3) + mp.sin(t) / t * K + (1 - mp.cos(t)) / t ** 2 * K * K
            tv = V * mp.matrix([mp.mpf(float(v)) for v in xi[:3]])
            T = orc.se3_exp(xi)
            worst = max(worst, max(abs(float(tv[i]) - T[i, 3]) for i in range(3)) / un,
                        max(abs(float(R[i, j]) - T[i, j]) for i in range(3) for j in range(3)))
            assert np.abs(orc.se3_log(T) - xi).max() <= 16 * 2.0 ** -52 * un
    assert worst <= 8 * 2.0 ** -52, worst


def test_voxel_downsample_semantics():
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [-0.3, 0.1, 0.1], [0.9, 0.1, 0.1], [1.1, 0.1, 0.1],
                    [-1.1, 0.1, 0.1], [0.15, 0.15, 0.15]])
    out, idx = orc.voxel_downsample(pts, 1.0, return_index=True)
    # (int)(x / size) truncates toward zero: -0.3 and 0.9 share voxel 0 with 0.1 (double-width voxel at the origin)
    assert list(idx) == [0, 4, 5]
    assert np.array_equal(out, pts[[0, 4, 5]])
    assert len(orc.voxel_downsample(np.zeros((0, 3)), 0.5)) == 0
    assert np.array_equal(orc.preprocess(np.array([[0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [70.0, 0, 0.0]]), 70.0, 1.0),
                          np.array([[3.0, 0, 0]]))  # strict inequalities on both ends


def test_map_cap_order_and_prune():
    m = orc.Map(1.0, 10.0, 20)
    rng = np.random.default_rng(1)
    first = np.array([[0.5, 0.5, 0.5]])
    m.add_points(first)
    more = 0.5 + rng.uniform(-0.4, 0.4, (50, 3))
    m.add_points(more)
    assert (m.num_voxels, m.num_points) == (1, 20)
    assert np.array_equal(m.points(), np.vstack([first, more[:19]]))  # first 20 in insertion order
    m.add_points(np.array([[30.5, 0.5, 0.5], [9.6, 0.5, 0.5]]))
    m.prune(np.array([0.0, 0.0, 0.0]))
    # voxel (30,0,0) is gone; voxel (9,0,0): |9.6 - 0|^2 + ... = 92.66 < 100 stays; the cap voxel stays
    assert m.num_voxels == 2
    m.prune(np.array([25.0, 0.0, 0.0]))  # decided by each voxel's FIRST point only
    assert m.num_voxels == 0


def test_nearest_neighbour_against_brute_force():
    rng = np.random.default_rng(3)
    m = orc.Map(0.7, 1e9, 20)
    P = rng.normal(0, 3, (20000, 3))
    m.add_points(P)
    pts = m.points()
    vk = np.trunc(pts / 0.7).astype(int)
    q = rng.normal(0, 2.5, (200, 3))
    _, nc, cand, tgt = m.linear_system(q, 0.5, 0.2, want_targets=True)
    n_ok = 0
    for i in range(len(q)):
        k = np.trunc(q[i] / 0.7).astype(int)
        sel = np.all(np.abs(vk - k) <= 1, axis=1)
        exp = None
        if sel.any():
            d = np.linalg.norm(pts[sel] - q[i], axis=1)
            j = np.argmin(d)
            if d[j] < 0.5:
                exp = pts[sel][j]
        got = None if np.isnan(tgt[i, 0]) else tgt[i]
        assert (exp is None) == (got is None)
        if exp is not None:
            assert np.array_equal(exp, got)
            n_ok += 1
    assert n_ok == nc and n_ok > 100


def test_registration_recovers_known_transform():
    rng = np.random.default_rng(5)
    M = _room(rng, 300000)
    m = orc.Map(0.7, 1e9, 20)
    m.add_points(M)
    # (a) source = map points themselves: the exact transform is a fixed point
    sub = m.points()[::9]
    Tt = orc.se3_exp(np.array([0.2, -0.1, 0.05, 0.01, -0.02, 0.03]))
    body = (np.linalg.inv(Tt) @ np.c_[sub, np.ones(len(sub))].T).T[:, :3]
    out, it, nc, _ = m.register(body, np.eye(4), 6.0, 2 / 3)
    assert np.abs(out - Tt).max() < 1e-4 and it < 60 and nc == len(sub)
    # (b) independent samples of the same surfaces: accuracy at the sampling-texture level
    S = orc.voxel_downsample(orc.voxel_downsample(_room(rng, 60000), 0.35), 1.05)
    body = (np.linalg.inv(Tt) @ np.c_[S, np.ones(len(S))].T).T[:, :3]
    out, it, _, _ = m.register(body, np.eye(4), 6.0, 2 / 3)
    assert np.linalg.norm(out[:3, 3] - Tt[:3, 3]) < 0.03 and orc.rot_angle(np.linalg.inv(Tt) @ out) < 2e-3
    # (c) empty map => the guess (as the SE3d it is turned into on entry: rotation through a unit quaternion); no
    # correspondences => the guess
    g = orc.se3_exp(np.array([1.0, 2.0, 3.0, 0.1, 0.2, 0.3]))
    out, it, _, _ = orc.Map(0.7, 100.0, 20).register(body, g, 6.0, 2 / 3)
    assert np.abs(out - g).max() < 1e-15 and it == 0
    far = body + 1000.0
    out, it, nc, _ = m.register(far, np.eye(4), 6.0, 2 / 3)
    assert np.array_equal(out, np.eye(4)) and it == 1 and nc == 0


def test_pipeline_first_scan_identity_and_threshold_state():
    rng = np.random.default_rng(7)
    scan = _room(rng, 30000)
    t01 = rng.uniform(0, 1, len(scan))
    icp = orc.ICP(100.0, 1.0)
    T0 = icp.register_frame(scan, t01)
    assert np.array_equal(T0, np.eye(4)) and icp.stats[0]["iterations"] == 0  # first scan: pose = guess = I
    T1 = icp.register_frame(scan, t01)  # the same scan again: exact fixed point, one iteration
    assert np.abs(T1 - np.eye(4)).max() < 1e-12 and icp.stats[1]["iterations"] == 1
    assert icp.stats[1]["sigma"] == 2.0 and not icp.has_moved()
    # move by 1 m per scan with an external guess: has_moved flips, sigma leaves 2.0 only once a deviation > 0.1 was seen
    for k in range(1, 4):
        G = np.eye(4)
        G[0, 3] = 1.0 * k
        body = scan - G[:3, 3]
        icp.register_frame(body, t01, guess=G @ orc.se3_exp(np.array([0.15, 0, 0, 0, 0, 0])))
    assert icp.has_moved()
    sig = [s["sigma"] for s in icp.stats]
    assert sig[2] == 2.0 and 0.1 < sig[-1] < 0.6  # sqrt of the mean squared deviation (> min_motion_th) so far


def test_registration_returns_an_orthonormal_pose_whatever_the_guess():
    """kiss-icp's poses are Sophus::SE3d: the 4x4 guess becomes a unit quaternion + translation when it enters the
    registration (pybind `Sophus::SE3d initial_guess(T_guess)`) and the result is the matrix of one.  A guess whose
    rotation block has drifted off SO(3) by 1e-6 comes back orthonormal to rounding - from an empty map and from a
    registration alike (round 2: without this the constant-velocity recursion loses every track around sweep 35-40)."""
    rng = np.random.default_rng(11)
    g = orc.se3_exp(np.array([0.3, -0.2, 0.1, 0.02, 0.01, -0.03]))
    g_bad = g.copy()
    g_bad[:3, :3] += 1e-6 * rng.normal(size=(3, 3))
    M = _room(rng, 100000)
    m = orc.Map(0.7, 1e9, 20)
    m.add_points(M)
    body = (np.linalg.inv(g) @ np.c_[m.points()[::7], np.ones(len(m.points()[::7]))].T).T[:, :3]
    for mp in (orc.Map(0.7, 100.0, 20), m):
        out, _, _, _ = mp.register(body, g_bad, 6.0, 2 / 3)
        R = out[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
        assert np.abs(out - g).max() < 1e-4


import pytest  # noqa: E402


@pytest.mark.parametrize("mode", ["constant_velocity", "external_guess"])
def test_independent_numpy_restatement_agrees_over_free_running_sweeps(mode):
    """oracle/icp_numpy.py - the pipeline restated a second time from SURVEY.md App. A alone (numpy, dict map, brute-force
    27-voxel search, scipy SO(3)) - and the C oracle, both free-running over 60 sweeps of the same synthetic sequence: same
    poses to 1e-9, same integer statistics every sweep (valid / down-sampled / source points, iterations, pairs, candidates
    examined, map size) and the same threshold.  Both guess modes of the reference: its own constant-velocity model
    (kiss.py:102-105) and a caller's guess (ekf_bench.py:533-548: here the ground truth, disturbed).  A divergence here is a
    restatement bug in one of the two (round 1's bare-matrix pose composition would have shown within 40 sweeps)."""
    import ptudes_lab_amd  # noqa: F401
    from oracle import icp_numpy as kn
    from ptudes_lab_amd import synth
    n = 60
    seq = synth.make_sequence(seed=2001, n_scans=n, H=16, W=256, min_range=1.0, max_range=70.0)
    t01 = seq.column_times()
    gt = seq.gt_poses(0.5)
    g0i = np.linalg.inv(gt[0])
    rng = np.random.default_rng(5)
    a = orc.ICP(max_range=70.0, min_range=1.0)
    b = kn.KissICP(max_range=70.0, min_range=1.0)
    worst, moved = 0.0, False
    for k in range(n):
        x = seq.scan(k).astype(np.float64)
        guess = None
        if mode == "external_guess":
            guess = g0i @ gt[k] @ kn.se3_exp(np.concatenate([rng.normal(0, 0.03, 3), rng.normal(0, 0.003, 3)]))
        pa, pb = a.register_frame(x, t01, guess), b.register_frame(x, t01, guess)
        sa, sb = a.stats[-1], b.stats[-1]
        for q in ("n_valid", "n_down", "n_src", "iterations", "n_corr_last", "sum_cand", "map_voxels", "map_points"):
            assert sa[q] == sb[q], (k, q, sa[q], sb[q])
        assert abs(sa["sigma"] - sb["sigma"]) < 1e-9, (k, sa["sigma"], sb["sigma"])
        worst = max(worst, float(np.abs(pa - pb).max()))
        moved = moved or sb["sigma"] != 2.0
    assert worst < 1e-9, worst
    assert moved  # the adaptive threshold left its initial value: that branch was compared too
    assert np.abs(pb[:3, :3] @ pb[:3, :3].T - np.eye(3)).max() < 1e-12


def test_innovation_is_formed_with_the_raw_guess_like_the_reference():
    """kiss.py:116-128: pose_gain = np.linalg.inv(initial_guess) @ new_pose on the guess AS THE CALLER HANDED IT OVER - the
    registration itself works on the Sophus::SE3d of it.  A sheared, scaled caller's guess (rotation block 1e-3 off
    orthonormal) tells the two apart: err_dt / err_drot / the next threshold of the C oracle must follow the numpy restatement,
    which does literally what the reference line does (round 3 formed them with the re-normalised guess)."""
    import ptudes_lab_amd  # noqa: F401
    from oracle import icp_numpy as kn
    from ptudes_lab_amd import synth
    n = 12
    seq = synth.make_sequence(seed=2003, n_scans=n, H=16, W=256, min_range=1.0, max_range=70.0)
    t01 = seq.column_times()
    gt = seq.gt_poses(0.5)
    g0i = np.linalg.inv(gt[0])
    rng = np.random.default_rng(7)
    a = orc.ICP(max_range=70.0, min_range=1.0)
    b = kn.KissICP(max_range=70.0, min_range=1.0)
    differs = 0.0
    for k in range(n):
        x = seq.scan(k).astype(np.float64)
        guess = g0i @ gt[k]
        guess[:3, :3] = guess[:3, :3] @ (np.eye(3) + 1e-3 * rng.normal(size=(3, 3)))  # not a rotation any more
        pa, pb = a.register_frame(x, t01, guess), b.register_frame(x, t01, guess)
        sa, sb = a.stats[-1], b.stats[-1]
        assert abs(sa["err_dt"] - sb["err_dt"]) < 1e-9 and abs(sa["err_drot"] - sb["err_drot"]) < 1e-7, (k, sa, sb)
        assert abs(sa["sigma"] - sb["sigma"]) < 1e-9 and sa["iterations"] == sb["iterations"], (k, sa, sb)
        assert np.abs(pa - pb).max() < 1e-9
        # what round 3 computed: the innovation against the re-normalised guess
        old = np.linalg.inv(kn.as_se3(guess)) @ pb
        differs = max(differs, abs(float(np.linalg.norm(old[:3, 3])) - sb["err_dt"]))
    assert differs > 1e-4  # the case does separate the two definitions

