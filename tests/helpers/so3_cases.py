"""Which branch of the four-case matrix-to-quaternion conversion (scipy's Rotation.from_matrix; csrc/devmath.h R_to_quat) a rotation
takes, computed from the matrices in numpy: tests assert from it that their inputs reach the branches they are there for."""
import numpy as np


def quat_case(R):
    """(n,) for (n, 3, 3) or (n, 9): 0, 1, 2 = that diagonal entry is the largest and not below the trace, 3 = the trace is larger"""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 9)
    d = R[:, [0, 4, 8]]
    tr = d.sum(1)
    return np.where(tr > d.max(1), 3, d.argmax(1))


def raw_w(R):
    """(n,) the w the conversion yields BEFORE normalisation: negative values are what R_to_rotvec has to flip"""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    c = quat_case(R)
    j, k = (c + 1) % 3, (c + 2) % 3
    i = np.arange(len(R))
    return np.where(c == 3, 1.0 + np.trace(R, axis1=1, axis2=2), R[i, k % 3, j % 3] - R[i, j % 3, k % 3])


def quat_to_R(q):
    """(n, 4) xyzw -> (n, 3, 3)"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def ekf_steps_coverage(g):
    """of one tests/golden/ekf_steps_*.npz: (count of each case over the attitudes after every IMU sample, number of updates whose
    attitude error R_est^T R_meas comes out of the conversion with w < 0)"""
    cases = np.bincount(quat_case(quat_to_R(g["nav_after_imu"][:, 3:7])), minlength=4)
    Re = quat_to_R(g["nav_after_imu"][g["upd_idx"], 3:7])
    err = np.einsum("nji,njk->nik", Re, g["upd_pose"][:, :3, :3])
    return cases, int((raw_w(err) < 0).sum())
