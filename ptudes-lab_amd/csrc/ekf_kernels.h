// ekf_kernels.h -- the ptudes 18-state error-state EKF on device (gfx950), fp64.
//
// Replaces reference src/ptudes/ins/es_ekf.py: ESEKF.processImu (:191-237, with _insMech :239-257) and
// ESEKF.processPose (:259-329).  One 384-thread workgroup (6 wavefronts) owns the filter: thread (i,j)
// of the first 324 owns covariance entry P[i][j]; the 18x18 products go through LDS.  A launch consumes
// a whole batch of IMU samples and, optionally, one pose update, so the per-scan EKF work of the
// reference's driver loop (cli/ekf_bench.py:493-563) is a single launch on the handle's stream.
//
// State order (es_ekf.py:65-71): POS 0, VEL 3, PHI 6, BG 9, BA 12, G 15.  Attitude is kept as an xyzw
// quaternion and every use converts through it, as the reference's NavState does (ins/data.py:76-82).
#pragma once
#include "devmath.h"

#define EKF_N 18
#define EKF_POS 0
#define EKF_VEL 3
#define EKF_PHI 6
#define EKF_BG 9
#define EKF_BA 12
#define EKF_G 15
#define EKF_CHUNK 64

struct EkfNav {
    double pos[3], q[4], vel[3], bg[3], ba[3], grav[3];
    double cur_lacc[3], cur_avel[3], cur_ts, cur_dt;
    int initialized, n_updates;
};
struct EkfState {
    EkfNav nav;
    double P[EKF_N * EKF_N];
    double Fx[EKF_N * EKF_N];  // persistent: identity + rewritten blocks (es_ekf.py:142, :216-223)
    double W[EKF_N * EKF_N];   // persistent: zero + rewritten diagonal blocks (es_ekf.py:145, :226-233)
    double pose[16];  // NavState.pose_mat() after the last step (ins/data.py:70-74)
    // Filter history for the fixed-interval smoother (k_ekf_smooth), off while `log` is null.  Phi = product of the Fx of the active
    // samples since the last logged update (identity at init, at a cold start and right after every logged update); every pose
    // update appends one EKF_LOG_STRIDE-double entry while log_count < log_cap, else raises log_overflow and writes nothing.
    double Phi[EKF_N * EKF_N];
    double* log;
    long long log_cap, log_count;
    int log_overflow, log_pad;
    // Knot list of the IMU deskew, off while `knots` is null: EKF_KNOT_STRIDE doubles per knot, (ts, pos[3], q xyzw[4])
    // of the nominal state right after the last pose update (before the first update: after the first IMU sample), then after every
    // later sample whose ts exceeds the previous knot's.  A pose update restarts the list; a knot that does not fit raises
    // knot_overflow (sticky until a cold start) and is dropped.
    double* knots;
    long long knot_cap, knot_count;
    int knot_overflow, knot_pad;
};
#define EKF_KNOT_STRIDE 8
// one log entry (doubles): ts | nav before the update (19: pos, q xyzw, vel, bg, ba, grav) | P before | Phi since the previous
// logged update | nav after (inject + PHI-block projection + reset) | P after; 1011 used, padded to 8 KB
#define EKF_LOG_STRIDE 1024
#define EKF_LOG_TS 0
#define EKF_LOG_NAV_PRED 1
#define EKF_LOG_P_PRED 20
#define EKF_LOG_PHI 344
#define EKF_LOG_NAV_POST 668
#define EKF_LOG_P_POST 687

__device__ __forceinline__ void ekf_nav19(const EkfNav& n, double* o) {
    for (int k = 0; k < 3; ++k) { o[k] = n.pos[k]; o[7 + k] = n.vel[k]; o[10 + k] = n.bg[k]; o[13 + k] = n.ba[k]; o[16 + k] = n.grav[k]; }
    for (int k = 0; k < 4; ++k) o[3 + k] = n.q[k];
}

__device__ __forceinline__ void ekf_knot8(const EkfNav& n, double* o) {
    o[0] = n.cur_ts;
    for (int k = 0; k < 3; ++k) o[1 + k] = n.pos[k];
    for (int k = 0; k < 4; ++k) o[4 + k] = n.q[k];
}

__device__ __forceinline__ void ekf_write_pose(EkfState* e) {
    double R[9];
    quat_to_R(e->nav.q, R);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) e->pose[4 * i + j] = R[3 * i + j];
        e->pose[4 * i + 3] = e->nav.pos[i];
    }
    e->pose[12] = e->pose[13] = e->pose[14] = 0.0;
    e->pose[15] = 1.0;
}

// ESEKF.__init__ (es_ekf.py:73-179)
__global__ void k_ekf_init(EkfState* e, const double* grav, const double* bacc, const double* bgyr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < 3; ++i) { e->nav.pos[i] = 0.0; e->nav.vel[i] = 0.0; e->nav.grav[i] = grav[i]; e->nav.ba[i] = bacc[i]; e->nav.bg[i] = bgyr[i]; }
    e->nav.q[0] = e->nav.q[1] = e->nav.q[2] = 0.0; e->nav.q[3] = 1.0;
    for (int i = 0; i < EKF_N * EKF_N; ++i) { e->P[i] = 0.0; e->Fx[i] = 0.0; e->W[i] = 0.0; }
    for (int i = 0; i < EKF_N; ++i) e->Fx[i * EKF_N + i] = 1.0;
    // initial attitude std = rotation vector of intrinsic-XYZ euler (10, 10, 10) deg (es_ekf.py:104-107)
    const double a = 10.0 * 3.14159265358979323846 / 180.0, cs = cos(a), sn = sin(a);
    const double Rx[9] = {1, 0, 0, 0, cs, -sn, 0, sn, cs}, Ry[9] = {cs, 0, sn, 0, 1, 0, -sn, 0, cs}, Rz[9] = {cs, -sn, 0, sn, cs, 0, 0, 0, 1};
    double R[9], rv[3];
    mat3_mul(Rx, Ry, R);
    mat3_mul(R, Rz, R);
    R_to_rotvec(R, rv);
    for (int i = 0; i < 3; ++i) {
        e->P[(EKF_POS + i) * EKF_N + EKF_POS + i] = 100.0;
        e->P[(EKF_VEL + i) * EKF_N + EKF_VEL + i] = 25.0;
        e->P[(EKF_PHI + i) * EKF_N + EKF_PHI + i] = rv[i] * rv[i];
        e->P[(EKF_BG + i) * EKF_N + EKF_BG + i] = 2.25;
        e->P[(EKF_BA + i) * EKF_N + EKF_BA + i] = 0.25;
        e->P[(EKF_G + i) * EKF_N + EKF_G + i] = 6.25;
    }
    e->nav.cur_ts = 0.0; e->nav.cur_dt = 0.0; e->nav.initialized = 0; e->nav.n_updates = 0;
    // a cold start empties the log (its buffer and capacity stay)
    for (int i = 0; i < EKF_N * EKF_N; ++i) e->Phi[i] = (i % (EKF_N + 1) == 0) ? 1.0 : 0.0;
    e->log_count = 0; e->log_overflow = 0;
    e->knot_count = 0; e->knot_overflow = 0;  // ... and the knot list
    for (int i = 0; i < 3; ++i) { e->nav.cur_lacc[i] = 0.0; e->nav.cur_avel[i] = 0.0; }
    ekf_write_pose(e);
}

__device__ __forceinline__ void set_blk3(double* M, int r, int c, const double* B) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[(r + i) * EKF_N + c + j] = B[3 * i + j];
}
__device__ __forceinline__ void set_diag3(double* M, int r, int c, double v) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[(r + i) * EKF_N + c + j] = (i == j) ? v : 0.0;
}

// One filter step batch.  Order inside a launch: [pose update, if `pose` and update_first] -> IMU samples
// [i0, i1) in order -> [pose update, if `pose` and !update_first].  The sequence runner uses
// update_first = 1 so that one launch per scan does "update with scan k's pose, then predict through the
// IMU samples that precede scan k+1" (reference loop order, cli/ekf_bench.py:493-563).
// imu: rows of 7 doubles (ts, lacc[3], avel[3]).  pose (nullable): 4x4 measurement; meas_cov (nullable): 6x6.
// out_* (nullable): res_poses / res_t / NC-GT row written right after the update (ekf_bench.py:560-563).
// P, Fx and W live in LDS for the whole launch (Fx / W are persistent members in the reference: identity /
// zero plus the blocks each predict rewrites, es_ekf.py:142-145, :216-233).
__device__ __forceinline__ void lds_blk3(double* M, int r, int c, const double* B) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[(r + i) * EKF_N + c + j] = B[3 * i + j];
}
__device__ __forceinline__ void lds_diag3(double* M, int r, int c, double v) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[(r + i) * EKF_N + c + j] = (i == j) ? v : 0.0;
}

// columns of Fx row i that can be non-zero: the diagonal plus the blocks es_ekf.py:216-223 writes
// ((POS,VEL) diag; (VEL,PHI), (VEL,BA), (PHI,PHI) dense 3x3; (PHI,BG) diag)
__device__ __forceinline__ unsigned ekf_row_mask(int i) {
    if (i < 3) return (1u << i) | (1u << (EKF_VEL + i));
    if (i < 6) return (1u << i) | (7u << EKF_PHI) | (7u << EKF_BA);
    if (i < 9) return (7u << EKF_PHI) | (1u << (EKF_BG + i - EKF_PHI));
    return 1u << i;
}

__device__ __forceinline__ void d_ekf_step(EkfState* e, const double* imu, int i0, int i1, const double* pose,
                                           const double* meas_cov, double* out_pose, double* out_t,
                                           double* out_row8, int update_first) {
    // Fx / W are double-buffered: the mechanisation thread writes the blocks of sample j into buffer j & 1 while the
    // covariance products of sample j - 1 still read buffer (j - 1) & 1 (every active sample rewrites all the blocks,
    // the other entries never change, so both buffers always agree outside the blocks in flight)
    __shared__ double sP[EKF_N * EKF_N], sF2[2][EKF_N * EKF_N], sW2[2][EKF_N * EKF_N], sT[EKF_N * EKF_N];
    __shared__ int sAct[2], s_lastbuf;
    __shared__ double sK[EKF_N * 6], sSi[36], sr[6], sdx[EKF_N];
    __shared__ double sM[6][12];
    __shared__ int sPiv;
    __shared__ double sRd[EKF_CHUNK][10];  // per-sample Exp(dtheta) (9) and dt
    __shared__ double sBias[8];
    __shared__ double sPhi[EKF_N * EKF_N];  // the smoother's transition accumulator (only touched while the log is on)
    const int tid = threadIdx.x;
    const int ti = tid / EKF_N, tj = tid % EKF_N;
    const bool cell = tid < EKF_N * EKF_N;
    if (cell) { sP[tid] = e->P[tid]; sF2[0][tid] = sF2[1][tid] = e->Fx[tid]; sW2[0][tid] = sW2[1][tid] = e->W[tid]; }
    double* const lg = e->log;  // uniform: the history log of the smoother, null = off
    long long lcount = 0;
    if (lg) {
        lcount = e->log_count;
        if (cell) sPhi[tid] = e->Phi[tid];
    }
    double phin = 0.0;
    double* const kn = e->knots;  // uniform: the IMU deskew's knot list, null = off
    long long kcount = 0;         // (the mechanisation lane's copy is the one that counts; a pose update resets every copy)
    double klast = 0.0;           // time of the last knot
    if (kn) {
        kcount = e->knot_count;
        if (kcount > 0) klast = kn[EKF_KNOT_STRIDE * (kcount - 1)];
    }
    if (tid == 0) s_lastbuf = 0;
    // the mechanisation (one lane) runs in a wavefront of its own when the launch has one to spare, so that it overlaps
    // the covariance products instead of preceding them
    const int TS = (blockDim.x > EKF_N * EKF_N + 60) ? 384 : 0;
    // the nav state lives in LDS for the whole launch (only thread 0 touches it; written back once at the end)
    __shared__ EkfNav nv;
    if (tid < (int)(sizeof(EkfNav) / 8)) ((double*)&nv)[tid] = ((const double*)&e->nav)[tid];
    __syncthreads();
    const int sel[6] = {EKF_POS, EKF_POS + 1, EKF_POS + 2, EKF_PHI, EKF_PHI + 1, EKF_PHI + 2};
    for (int phase = 0; phase < 3; ++phase) {
        const bool do_update = pose && ((phase == 0 && update_first) || (phase == 2 && !update_first));
        if (phase == 1) {
            // The gyro / accelerometer biases are constant between pose updates, so the per-sample rotation
            // increments Exp((w - b_g) dt) - the only transcendental work of a predict - do not depend on the
            // running state: they are computed for a chunk of samples in parallel, one thread per sample.
            for (int c0 = i0; c0 < i1; c0 += EKF_CHUNK) {
                const int nc = (i1 - c0) < EKF_CHUNK ? (i1 - c0) : EKF_CHUNK;
                if (tid == 0) { for (int k = 0; k < 3; ++k) { sBias[k] = nv.bg[k]; sBias[3 + k] = nv.ba[k]; } sBias[6] = nv.cur_ts; }
                __syncthreads();
                if (tid < nc) {
                    const double* row = imu + 7 * (size_t)(c0 + tid);
                    const double tprev = (tid == 0) ? sBias[6] : imu[7 * (size_t)(c0 + tid - 1)];
                    const double dt = row[0] - tprev;  // es_ekf.py:196
                    double dth[3], Rd[9];
                    for (int k = 0; k < 3; ++k) dth[k] = (row[4 + k] - sBias[k]) * dt;
                    rotvec_to_R(dth, Rd);
                    for (int k = 0; k < 9; ++k) sRd[tid][k] = Rd[k];
                    sRd[tid][9] = dt;
                }
                __syncthreads();
                // Software pipeline over the samples, two barriers per sample: while the mechanisation lane works on sample
                // j (stage 1: _insMech; stage 2: the Fx / W blocks), the 324 cell threads form P = Fx P Fx^T + W of
                // sample j - 1 (stage 1: Fx P; stage 2: (Fx P) Fx^T + W).
                double Rp[9], a[3], Rd[9], dtj = 0.0;
                int act_j = 0;
                for (int j = 0; j <= nc; ++j) {
                    const int bj = j & 1, bp = (j - 1) & 1;
                    const bool prev_active = j >= 1 && sAct[bp] != 0;
                    // ---- stage 1
                    if (tid == TS && j < nc) {  // processImu of sample j: latch + mechanisation (:191-214, _insMech :239-257)
                        const double* row = imu + 7 * (size_t)(c0 + j);
                        nv.cur_dt = sRd[j][9];
                        nv.cur_ts = row[0];
                        for (int k = 0; k < 3; ++k) { nv.cur_lacc[k] = row[1 + k]; nv.cur_avel[k] = row[4 + k]; }
                        if (!nv.initialized) {  // :201-203 the first sample only latches
                            nv.initialized = 1;
                            act_j = 0;
                        } else {
                            act_j = 1;
                            dtj = nv.cur_dt;
                            double Rn[9];
                            quat_to_R(nv.q, Rp);  // nav_prev.att_h
                            for (int k = 0; k < 3; ++k) a[k] = row[1 + k] - nv.ba[k];
                            for (int k = 0; k < 9; ++k) Rd[k] = sRd[j][k];
                            for (int k = 0; k < 3; ++k) {
                                const double ag = (Rp[3 * k] * a[0] + Rp[3 * k + 1] * a[1] + Rp[3 * k + 2] * a[2]) + nv.grav[k];
                                nv.pos[k] = nv.pos[k] + nv.vel[k] * dtj + 0.5 * ag * dtj * dtj;
                                nv.vel[k] = nv.vel[k] + ag * dtj;
                            }
                            mat3_mul(Rp, Rd, Rn);
                            R_to_quat(Rn, nv.q);
                        }
                        sAct[bj] = act_j;
                        if (kn && (kcount == 0 || nv.cur_ts > klast)) {  // the knot of this sample
                            if (kcount < e->knot_cap) {
                                ekf_knot8(nv, kn + EKF_KNOT_STRIDE * kcount);
                                kcount += 1;
                                klast = nv.cur_ts;
                            } else {
                                e->knot_overflow = 1;
                            }
                        }
                    }
                    if (prev_active && cell) {
                        // P = Fx P Fx^T + W (:235), dense like the reference.  Only the structurally non-zero columns of
                        // each Fx row are visited, in ascending order: skipping exact-zero products leaves every
                        // partial sum bit-identical to the dense loop.
                        const double* sF = sF2[bp];
                        double acc = 0.0;
                        for (unsigned m = ekf_row_mask(ti); m; m &= m - 1) {
                            const int k = __ffs(m) - 1;
                            acc += sF[ti * EKF_N + k] * sP[k * EKF_N + tj];
                        }
                        sT[tid] = acc;
                        if (lg) {  // Phi = Fx Phi with the same Fx (written back in stage 2, nobody reads sPhi there)
                            double ph = 0.0;
                            for (unsigned m = ekf_row_mask(ti); m; m &= m - 1) {
                                const int k = __ffs(m) - 1;
                                ph += sF[ti * EKF_N + k] * sPhi[k * EKF_N + tj];
                            }
                            phin = ph;
                        }
                    }
                    __syncthreads();
                    // ---- stage 2
                    if (tid == TS && j < nc && act_j) {  // Fx blocks (:216-223) and W blocks (:226-233) of sample j
                        double* sF = sF2[bj];
                        double* sW = sW2[bj];
                        double K[9], B[9];
                        lds_diag3(sF, EKF_POS, EKF_VEL, dtj);
                        skew(a, K);
                        mat3_mul(Rp, K, B);
                        for (int k = 0; k < 9; ++k) B[k] = -dtj * B[k];
                        lds_blk3(sF, EKF_VEL, EKF_PHI, B);
                        for (int k = 0; k < 9; ++k) B[k] = -dtj * Rp[k];
                        lds_blk3(sF, EKF_VEL, EKF_BA, B);
                        for (int r = 0; r < 3; ++r)
                            for (int cc = 0; cc < 3; ++cc) B[3 * r + cc] = Rd[3 * cc + r];
                        lds_blk3(sF, EKF_PHI, EKF_PHI, B);
                        lds_diag3(sF, EKF_PHI, EKF_BG, -dtj);
                        // the reference's names of the noise terms do not match their use, this copies the use
                        lds_diag3(sW, EKF_VEL, EKF_VEL, dtj * dtj * (0.049 * 0.049));
                        lds_diag3(sW, EKF_PHI, EKF_PHI, dtj * dtj * (0.38 * 0.38));
                        lds_diag3(sW, EKF_BA, EKF_BA, dtj * (0.0043 * 0.0043));
                        lds_diag3(sW, EKF_BG, EKF_BG, dtj * (0.000466 * 0.000466));
                        s_lastbuf = bj;
                    }
                    if (prev_active && cell) {
                        const double* sF = sF2[bp];
                        double acc = 0.0;
                        for (unsigned m = ekf_row_mask(tj); m; m &= m - 1) {
                            const int k = __ffs(m) - 1;
                            acc += sT[ti * EKF_N + k] * sF[tj * EKF_N + k];
                        }
                        sP[tid] = acc + sW2[bp][tid];
                        if (lg) sPhi[tid] = phin;
                    }
                    __syncthreads();
                }
            }
            continue;
        }
        if (!do_update) continue;
        // the smoother's log entry: the state before the update (all writers of nv / sP are behind a barrier here)
        const bool logit = lg && lcount < e->log_cap;
        double* const ent = logit ? lg + (size_t)lcount * EKF_LOG_STRIDE : nullptr;
        if (logit) {
            if (cell) { ent[EKF_LOG_P_PRED + tid] = sP[tid]; ent[EKF_LOG_PHI + tid] = sPhi[tid]; }
            if (tid == 0) { ent[EKF_LOG_TS] = nv.cur_ts; ekf_nav19(nv, ent + EKF_LOG_NAV_PRED); }
        }
        // ---- processPose (:259-329); the error state is zero on entry (reset at :327)
        if (tid == 0) {
            double Rk[9], RkT[9], Rm[9], D[9];
            quat_to_R(nv.q, Rk);
            for (int r = 0; r < 3; ++r)
                for (int cc = 0; cc < 3; ++cc) { RkT[3 * r + cc] = Rk[3 * cc + r]; Rm[3 * r + cc] = pose[4 * r + cc]; }
            for (int k = 0; k < 3; ++k) sr[k] = pose[4 * k + 3] - nv.pos[k];  // :294
            mat3_mul(RkT, Rm, D);
            R_to_rotvec(D, sr + 3);  // :297
        }
        // S = Jp P Jp^T + R (:299) and its inverse by Gauss-Jordan with partial pivoting (np.linalg.inv, :300), held
        // in LDS as the 6 x 12 augmented matrix [S | I]; thread (a, b) owns one entry, every entry sees exactly
        // the operations of the sequential algorithm.
        if (tid < 72) {
            const int a = tid / 12, bb = tid % 12;
            double v;
            if (bb < 6) {
                double rm;
                if (meas_cov) rm = meas_cov[6 * a + bb];
                else rm = (a == bb) ? ((a < 3) ? 0.02 * 0.02 : 0.01 * 0.01) : 0.0;  // :289-292
                v = sP[sel[a] * EKF_N + sel[bb]] + rm;
            } else {
                v = (a == bb - 6) ? 1.0 : 0.0;
            }
            sM[a][bb] = v;
        }
        __syncthreads();
        for (int cI = 0; cI < 6; ++cI) {
            if (tid == 0) {
                int p = cI;
                for (int r = cI + 1; r < 6; ++r)
                    if (fabs(sM[r][cI]) > fabs(sM[p][cI])) p = r;
                sPiv = p;
            }
            __syncthreads();
            const int p = sPiv;
            double mine = 0.0, other = 0.0;
            if (tid < 12 && p != cI) { mine = sM[cI][tid]; other = sM[p][tid]; }
            __syncthreads();
            if (tid < 12 && p != cI) { sM[cI][tid] = other; sM[p][tid] = mine; }
            __syncthreads();
            const double d = sM[cI][cI];
            double pv = 0.0;
            if (tid < 12) pv = sM[cI][tid] / d;
            __syncthreads();
            if (tid < 12) sM[cI][tid] = pv;
            __syncthreads();
            double f = 0.0, prow = 0.0, cur = 0.0;
            const int a = tid / 12, bb = tid % 12;
            if (tid < 72 && a != cI) { f = sM[a][cI]; prow = sM[cI][bb]; cur = sM[a][bb]; }
            __syncthreads();
            if (tid < 72 && a != cI && f != 0.0) sM[a][bb] = cur - f * prow;
            __syncthreads();
        }
        if (tid < 36) sSi[tid] = sM[tid / 6][6 + tid % 6];
        __syncthreads();
        if (tid < EKF_N * 6) {  // K = P Jp^T S^-1 (:300)
            const int i = tid / 6, j = tid % 6;
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc += sP[i * EKF_N + sel[k]] * sSi[6 * k + j];
            sK[tid] = acc;
        }
        __syncthreads();
        if (tid < EKF_N) {  // dx = K r (:301)
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc += sK[tid * 6 + k] * sr[k];
            sdx[tid] = acc;
        }
        // P = (I - K Jp) P (:303): build (I - K Jp) in sT, then multiply
        if (cell) {
            double v = (ti == tj) ? 1.0 : 0.0;
            for (int k = 0; k < 6; ++k)
                if (sel[k] == tj) v -= sK[ti * 6 + k];
            sT[tid] = v;
        }
        __syncthreads();
        double pn = 0.0;
        if (cell)
            for (int k = 0; k < EKF_N; ++k) pn += sT[ti * EKF_N + k] * sP[k * EKF_N + tj];
        __syncthreads();
        if (cell) sP[tid] = pn;
        __syncthreads();
        if (tid == 0) {
            // inject (:314-319)
            double dth[3], R[9], Rd[9], Rn[9];
            for (int k = 0; k < 3; ++k) {
                nv.pos[k] += sdx[EKF_POS + k];
                nv.vel[k] += sdx[EKF_VEL + k];
                dth[k] = sdx[EKF_PHI + k];
                nv.bg[k] += sdx[EKF_BG + k];
                nv.ba[k] += sdx[EKF_BA + k];
                nv.grav[k] += sdx[EKF_G + k];
            }
            quat_to_R(nv.q, R);
            rotvec_to_R(dth, Rd);
            mat3_mul(R, Rd, Rn);
            R_to_quat(Rn, nv.q);
            // covariance projection of the PHI diagonal block only (:322-324): G = I - hat(dth / 2)
            const double h[3] = {0.5 * dth[0], 0.5 * dth[1], 0.5 * dth[2]};
            double Gm[9], GT[9], B[9], C[9];
            skew(h, Gm);
            for (int k = 0; k < 9; ++k) Gm[k] = -Gm[k];
            Gm[0] += 1.0; Gm[4] += 1.0; Gm[8] += 1.0;
            for (int r = 0; r < 3; ++r)
                for (int cc = 0; cc < 3; ++cc) { GT[3 * r + cc] = Gm[3 * cc + r]; B[3 * r + cc] = sP[(EKF_PHI + r) * EKF_N + EKF_PHI + cc]; }
            mat3_mul(Gm, B, C);
            mat3_mul(C, GT, C);
            for (int r = 0; r < 3; ++r)
                for (int cc = 0; cc < 3; ++cc) sP[(EKF_PHI + r) * EKF_N + EKF_PHI + cc] = C[3 * r + cc];
            nv.n_updates += 1;
            // outputs of this update (ekf_bench.py:560-563): nav pose and the last IMU's timestamp
            e->nav = nv;
            ekf_write_pose(e);
            if (out_pose) for (int k = 0; k < 16; ++k) out_pose[k] = e->pose[k];
            if (out_t) *out_t = nv.cur_ts;
            if (out_row8) {  // [t, x, y, z, qx, qy, qz, qw] for the trajectory gather
                out_row8[0] = nv.cur_ts;
                for (int k = 0; k < 3; ++k) out_row8[1 + k] = nv.pos[k];
                for (int k = 0; k < 4; ++k) out_row8[4 + k] = nv.q[k];
            }
            if (kn) ekf_knot8(nv, kn);  // the knot list starts again with the state after the update
        }
        __syncthreads();
        if (kn) { kcount = 1; klast = nv.cur_ts; }
        if (lg) {  // the state after the update; Phi starts again
            if (logit) {
                if (cell) ent[EKF_LOG_P_POST + tid] = sP[tid];
                if (tid == 0) ekf_nav19(nv, ent + EKF_LOG_NAV_POST);
                lcount += 1;
            } else if (tid == 0) {
                e->log_overflow = 1;
            }
            if (cell) sPhi[tid] = (ti == tj) ? 1.0 : 0.0;
        }
    }
    if (cell) { e->P[tid] = sP[tid]; e->Fx[tid] = sF2[s_lastbuf][tid]; e->W[tid] = sW2[s_lastbuf][tid]; }
    if (tid == 0) { e->nav = nv; ekf_write_pose(e); }
    if (lg) {
        if (cell) e->Phi[tid] = sPhi[tid];
        if (tid == 0) e->log_count = lcount;
    }
    if (kn && tid == TS) e->knot_count = kcount;
}

#define EKF_THREADS 448  /* 324 covariance cells (six wavefronts) + a seventh wavefront for the mechanisation lane */
__global__ __launch_bounds__(EKF_THREADS) void k_ekf_step(EkfState* e, const double* imu, int i0, int i1, const double* pose,
                                                  const double* meas_cov, double* out_pose, double* out_t,
                                                  double* out_row8, int update_first) {
    d_ekf_step(e, imu, i0, i1, pose, meas_cov, out_pose, out_t, out_row8, update_first);
}
// One IMU sample (processImu) / one pose measurement (processPose) with the payload passed by value in the kernel
// arguments: no staging copy, so the per-call API neither copies nor synchronises - the call returns once the
// launch is queued, and the state is read back (and the stream drained) only when the caller asks for it.
struct EkfRow7 { double v[7]; };
struct EkfPoseArg { double pose[16]; double cov[36]; int has_cov; };
__global__ __launch_bounds__(384) void k_ekf_imu_value(EkfState* e, EkfRow7 row) {
    __shared__ double srow[7];
    if (threadIdx.x < 7) srow[threadIdx.x] = row.v[threadIdx.x];
    __syncthreads();
    d_ekf_step(e, srow, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
}
__global__ __launch_bounds__(384) void k_ekf_pose_value(EkfState* e, EkfPoseArg a) {
    __shared__ double sp[16 + 36];
    if (threadIdx.x < 16) sp[threadIdx.x] = a.pose[threadIdx.x];
    if (threadIdx.x < 36) sp[16 + threadIdx.x] = a.cov[threadIdx.x];
    __syncthreads();
    d_ekf_step(e, nullptr, 0, 0, sp, a.has_cov ? sp + 16 : nullptr, nullptr, nullptr, nullptr, 0);
}
// S filters in one launch (blockIdx.x = sequence)
#define EKF_MAX_SEQ 64
struct EkfBatchArgs {
    EkfState* e[EKF_MAX_SEQ];
    const double* imu[EKF_MAX_SEQ];
    int i0[EKF_MAX_SEQ], i1[EKF_MAX_SEQ];
    const double* pose[EKF_MAX_SEQ];
    double* out_pose[EKF_MAX_SEQ];
    double* out_t[EKF_MAX_SEQ];
    double* out_row8[EKF_MAX_SEQ];
    int update_first;
};
__global__ __launch_bounds__(384) void kb_ekf_step(EkfBatchArgs a) {
    const int s = blockIdx.x;
    d_ekf_step(a.e[s], a.imu[s], a.i0[s], a.i1[s], a.pose[s], nullptr, a.out_pose[s], a.out_t[s], a.out_row8[s], a.update_first);
}

// ================================================================================================ fixed-interval RTS smoother
// k_ekf_smooth: the Rauch-Tung-Striebel backward pass over one filter's log (EkfState::log), one workgroup per filter, thread (i, j)
// of the first 324 owns entry (i, j) of the 18x18 matrices in LDS.  From x^s_N = x_{N|N}, P^s_N = P_{N|N}, for k = N-2 .. 0
// (entry k: post = x_{k|k}, P_{k|k}; entry k+1: pred = x_{k+1|k}, P_{k+1|k}, Phi = Phi_{k->k+1}):
//   P_{k+1|k} X = Phi P_{k|k}              (Cholesky, right-looking in LDS),  C = X^T
//   e     = x^s_{k+1} [-] x_{k+1|k}        (pos / vel / bg / ba / grav: difference; attitude: Log(R_{k+1|k}^T R^s_{k+1}))
//   x^s_k = x_{k|k} [+] C e                (attitude: R_{k|k} Exp(dphi), the filter's right perturbation)
//   P^s_k = P_{k|k} + C (P^s_{k+1} - P_{k+1|k}) C^T, then (P + P^T) / 2
// The chain is serial per filter; entry k-1 (about 8 KB) is loaded into registers while entry k is computed.
// info[0]: 0 = done, -1 = the log overflowed, -2 = no log, 1 + i = P_pred of entry i is not positive definite (outputs not
// trusted); info[1]: rows written (rows k .. N-1 are valid when the pass stopped early).
struct EkfSmoothJob {
    const EkfState* e;
    double *pose, *t, *nav, *cov;  // [N][16], [N], [N][19], [N][324]
    long long* info;               // [2]
};
#define EKF_SMOOTH_THREADS 384

__device__ __forceinline__ void ekf_smooth_row(const double* xs, double t, const double* Ps, const EkfSmoothJob& J, long long k, int tid) {
    if (tid < 19) J.nav[19 * k + tid] = xs[tid];
    if (tid < EKF_N * EKF_N) J.cov[324 * k + tid] = Ps[tid];
    if (tid == 0) {  // the res_poses form (ekf_write_pose)
        double R[9];
        quat_to_R(xs + 3, R);
        double* o = J.pose + 16 * k;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) o[4 * i + j] = R[3 * i + j];
            o[4 * i + 3] = xs[i];
        }
        o[12] = o[13] = o[14] = 0.0;
        o[15] = 1.0;
        J.t[k] = t;
    }
}

__global__ __launch_bounds__(EKF_SMOOTH_THREADS) void k_ekf_smooth(const EkfSmoothJob* jobs) {
    __shared__ double sPs[EKF_N * EKF_N], sPk[EKF_N * EKF_N], sPp[EKF_N * EKF_N], sPhi[EKF_N * EKF_N];
    __shared__ double sL[EKF_N * EKF_N], sX[EKF_N * EKF_N], sT[EKF_N * EKF_N];
    __shared__ double sxs[19], snk[19], snp[19], se[EKF_N], sdx[EKF_N];
    __shared__ int sbad;
    const EkfSmoothJob J = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    const int ti = tid / EKF_N, tj = tid % EKF_N;
    const bool cell = tid < EKF_N * EKF_N;
    const double* lg = J.e->log;
    const long long N = J.e->log_count;
    if (!lg || J.e->log_overflow) {
        if (tid == 0) { J.info[0] = lg ? -1 : -2; J.info[1] = 0; }
        return;
    }
    if (N <= 0) {
        if (tid == 0) { J.info[0] = 0; J.info[1] = 0; }
        return;
    }
    const double* last = lg + (size_t)(N - 1) * EKF_LOG_STRIDE;
    if (cell) sPs[tid] = last[EKF_LOG_P_POST + tid];
    if (tid < 19) sxs[tid] = last[EKF_LOG_NAV_POST + tid];
    if (tid == 0) sbad = 0;
    __syncthreads();
    ekf_smooth_row(sxs, last[EKF_LOG_TS], sPs, J, N - 1, tid);
    // registers: entry k's post part and entry k + 1's pred part, loaded one step ahead
    double rPk = 0.0, rPp = 0.0, rPhi = 0.0, rnk = 0.0, rnp = 0.0, rt = 0.0;
    auto fetch = [&](long long k) {
        const double* ek = lg + (size_t)k * EKF_LOG_STRIDE;
        const double* e1 = ek + EKF_LOG_STRIDE;
        if (cell) { rPk = ek[EKF_LOG_P_POST + tid]; rPp = e1[EKF_LOG_P_PRED + tid]; rPhi = e1[EKF_LOG_PHI + tid]; }
        if (tid < 19) { rnk = ek[EKF_LOG_NAV_POST + tid]; rnp = e1[EKF_LOG_NAV_PRED + tid]; }
        rt = ek[EKF_LOG_TS];
    };
    if (N >= 2) fetch(N - 2);
    long long k = N - 2;
    for (; k >= 0; --k) {
        if (cell) { sPk[tid] = rPk; sPp[tid] = rPp; sL[tid] = rPp; sPhi[tid] = rPhi; }
        if (tid < 19) { snk[tid] = rnk; snp[tid] = rnp; }
        const double tk = rt;
        __syncthreads();
        if (k >= 1) fetch(k - 1);
        // A = Phi P_{k|k} (into sX, solved in place below)
        if (cell) {
            double acc = 0.0;
            for (int m = 0; m < EKF_N; ++m) acc += sPhi[ti * EKF_N + m] * sPk[m * EKF_N + tj];
            sX[tid] = acc;
        }
        // Cholesky P_{k+1|k} = L L^T, lower triangle of sL
#pragma unroll 1
        for (int j = 0; j < EKF_N; ++j) {
            if (tid == 0) {
                const double d = sL[j * EKF_N + j];
                if (!(d > 0.0)) sbad = 1;
                sL[j * EKF_N + j] = sqrt(d);
            }
            __syncthreads();
            if (tid > j && tid < EKF_N) sL[tid * EKF_N + j] /= sL[j * EKF_N + j];
            __syncthreads();
            if (cell && tj > j && ti >= tj) sL[ti * EKF_N + tj] -= sL[ti * EKF_N + j] * sL[tj * EKF_N + j];
            __syncthreads();
        }
        if (sbad) {
            if (tid == 0) { J.info[0] = 1 + (k + 1); J.info[1] = N - 1 - k; }
            return;
        }
        // L L^T X = A, one column per thread: forward then back substitution
        if (tid < EKF_N) {
            const int c = tid;
#pragma unroll 1
            for (int i = 0; i < EKF_N; ++i) {
                double v = sX[i * EKF_N + c];
                for (int m = 0; m < i; ++m) v -= sL[i * EKF_N + m] * sX[m * EKF_N + c];
                sX[i * EKF_N + c] = v / sL[i * EKF_N + i];
            }
#pragma unroll 1
            for (int i = EKF_N - 1; i >= 0; --i) {
                double v = sX[i * EKF_N + c];
                for (int m = i + 1; m < EKF_N; ++m) v -= sL[m * EKF_N + i] * sX[m * EKF_N + c];
                sX[i * EKF_N + c] = v / sL[i * EKF_N + i];
            }
        }
        if (tid == 0) {  // e = x^s_{k+1} [-] x_{k+1|k} in the state order (POS, VEL, PHI, BG, BA, G)
            double Rp[9], Rs[9], D[9];
            quat_to_R(snp + 3, Rp);
            quat_to_R(sxs + 3, Rs);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    double acc = 0.0;
                    for (int m = 0; m < 3; ++m) acc += Rp[3 * m + r] * Rs[3 * m + c];
                    D[3 * r + c] = acc;
                }
            R_to_rotvec(D, se + EKF_PHI);
            for (int i = 0; i < 3; ++i) {
                se[EKF_POS + i] = sxs[i] - snp[i];
                se[EKF_VEL + i] = sxs[7 + i] - snp[7 + i];
                se[EKF_BG + i] = sxs[10 + i] - snp[10 + i];
                se[EKF_BA + i] = sxs[13 + i] - snp[13 + i];
                se[EKF_G + i] = sxs[16 + i] - snp[16 + i];
            }
        }
        __syncthreads();
        // dx = C e (C = X^T); T = C (P^s_{k+1} - P_{k+1|k})
        if (tid < EKF_N) {
            double acc = 0.0;
            for (int m = 0; m < EKF_N; ++m) acc += sX[m * EKF_N + tid] * se[m];
            sdx[tid] = acc;
        }
        if (cell) {
            double acc = 0.0;
            for (int m = 0; m < EKF_N; ++m) acc += sX[m * EKF_N + ti] * (sPs[m * EKF_N + tj] - sPp[m * EKF_N + tj]);
            sT[tid] = acc;
        }
        __syncthreads();
        // P^s_k = P_{k|k} + T C^T, symmetrised
        double pn = 0.0;
        if (cell) {
            double acc = 0.0;
            for (int m = 0; m < EKF_N; ++m) acc += sT[ti * EKF_N + m] * sX[m * EKF_N + tj];
            pn = sPk[tid] + acc;
        }
        __syncthreads();
        if (cell) sPs[tid] = pn;
        __syncthreads();
        if (cell) pn = 0.5 * (sPs[ti * EKF_N + tj] + sPs[tj * EKF_N + ti]);
        __syncthreads();
        if (cell) sPs[tid] = pn;
        if (tid == 0) {  // x^s_k = x_{k|k} [+] dx
            double R[9], Rd[9], Rn[9];
            for (int i = 0; i < 3; ++i) {
                sxs[i] = snk[i] + sdx[EKF_POS + i];
                sxs[7 + i] = snk[7 + i] + sdx[EKF_VEL + i];
                sxs[10 + i] = snk[10 + i] + sdx[EKF_BG + i];
                sxs[13 + i] = snk[13 + i] + sdx[EKF_BA + i];
                sxs[16 + i] = snk[16 + i] + sdx[EKF_G + i];
            }
            quat_to_R(snk + 3, R);
            rotvec_to_R(sdx + EKF_PHI, Rd);
            mat3_mul(R, Rd, Rn);
            R_to_quat(Rn, sxs + 3);
        }
        __syncthreads();
        ekf_smooth_row(sxs, tk, sPs, J, k, tid);
        __syncthreads();
    }
    if (tid == 0) { J.info[0] = 0; J.info[1] = N; }
}
