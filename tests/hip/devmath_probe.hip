// devmath_probe.hip -- test-only: evaluates the functions of csrc/devmath.h on N inputs, once on the host and once in a kernel
// (one thread per input), so that tests/test_devmath_probe.py can compare both compiles of the same header with a high-precision
// reference.  Not part of the product library: built by tests/helpers/devmath_probe.py into a temporary directory.
//
// Every operation is a struct with NI doubles in, NO doubles out per input; probe_<name>_host / probe_<name>_device (n, in, out)
// return 0 or the failing hipError_t.
#include "../../ptudes-lab_amd/csrc/devmath.h"

namespace {
PTL_HD Rt rt_from12(const double* a) {
    Rt r;
    for (int i = 0; i < 9; ++i) r.R[i] = a[i];
    for (int i = 0; i < 3; ++i) r.t[i] = a[9 + i];
    return r;
}
PTL_HD void rt_to12(const Rt& r, double* o) {
    for (int i = 0; i < 9; ++i) o[i] = r.R[i];
    for (int i = 0; i < 3; ++i) o[9 + i] = r.t[i];
}

struct OpRToQuat   { static constexpr int NI = 9,  NO = 4;  PTL_HD static void f(const double* a, double* o) { R_to_quat(a, o); } };
struct OpQuatToR   { static constexpr int NI = 4,  NO = 9;  PTL_HD static void f(const double* a, double* o) { quat_to_R(a, o); } };
struct OpRotvecToR { static constexpr int NI = 3,  NO = 9;  PTL_HD static void f(const double* a, double* o) { rotvec_to_R(a, o); } };
struct OpRToRotvec { static constexpr int NI = 9,  NO = 3;  PTL_HD static void f(const double* a, double* o) { R_to_rotvec(a, o); } };
struct OpRotAngle  { static constexpr int NI = 9,  NO = 1;  PTL_HD static void f(const double* a, double* o) { o[0] = rot_angle(a); } };
struct OpRtProject { static constexpr int NI = 12, NO = 12; PTL_HD static void f(const double* a, double* o) { rt_to12(rt_project(rt_from12(a)), o); } };
struct OpMat3Polar { static constexpr int NI = 9,  NO = 9;  PTL_HD static void f(const double* a, double* o) { mat3_polar(a, o); } };
struct OpSe3Exp    { static constexpr int NI = 6,  NO = 12; PTL_HD static void f(const double* a, double* o) { rt_to12(se3_exp(a), o); } };
struct OpSe3ExpGn  { static constexpr int NI = 6,  NO = 12; PTL_HD static void f(const double* a, double* o) { rt_to12(se3_exp_gn(a), o); } };
struct OpSe3Log    { static constexpr int NI = 12, NO = 6;  PTL_HD static void f(const double* a, double* o) { se3_log(rt_from12(a), o); } };
struct OpRtInv     { static constexpr int NI = 12, NO = 12; PTL_HD static void f(const double* a, double* o) { rt_to12(rt_inv(rt_from12(a)), o); } };
struct OpRtMul     { static constexpr int NI = 24, NO = 12; PTL_HD static void f(const double* a, double* o) { rt_to12(rt_mul(rt_from12(a), rt_from12(a + 12)), o); } };
// out[16] = 1.0 when mat4_inv reports an invertible matrix
struct OpMat4Inv   { static constexpr int NI = 16, NO = 17; PTL_HD static void f(const double* a, double* o) { o[16] = mat4_inv(a, o) ? 1.0 : 0.0; } };
struct OpSolve6    { static constexpr int NI = 27, NO = 6;  PTL_HD static void f(const double* a, double* o) { solve6_ldlt(a, o); } };

template <class Op>
void run_host(int n, const double* in, double* out) {
    for (int i = 0; i < n; ++i) Op::f(in + (size_t)i * Op::NI, out + (size_t)i * Op::NO);
}

template <class Op>
__global__ void __launch_bounds__(256) k_probe(int n, const double* __restrict__ in, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double a[Op::NI], o[Op::NO];
    for (int k = 0; k < Op::NI; ++k) a[k] = in[(size_t)i * Op::NI + k];
    Op::f(a, o);
    for (int k = 0; k < Op::NO; ++k) out[(size_t)i * Op::NO + k] = o[k];
}

#define PROBE_TRY(call)                  \
    do {                                 \
        rc = (call);                     \
        if (rc != hipSuccess) goto done; \
    } while (0)

template <class Op>
int run_device(int n, const double* in, double* out) {
    if (n <= 0) return 0;
    const size_t bi = (size_t)n * Op::NI * sizeof(double), bo = (size_t)n * Op::NO * sizeof(double);
    double *d_in = nullptr, *d_out = nullptr;
    hipError_t rc;
    PROBE_TRY(hipMalloc((void**)&d_in, bi));
    PROBE_TRY(hipMalloc((void**)&d_out, bo));
    PROBE_TRY(hipMemcpy(d_in, in, bi, hipMemcpyHostToDevice));
    PROBE_TRY(hipMemset(d_out, 0xff, bo));  // NaN pattern: an element no thread wrote cannot pass
    hipLaunchKernelGGL(k_probe<Op>, dim3((n + 255) / 256), dim3(256), 0, 0, n, d_in, d_out);
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    PROBE_TRY(hipMemcpy(out, d_out, bo, hipMemcpyDeviceToHost));
done:
    if (d_in) {
        const hipError_t e = hipFree(d_in);
        if (rc == hipSuccess) rc = e;
    }
    if (d_out) {
        const hipError_t e = hipFree(d_out);
        if (rc == hipSuccess) rc = e;
    }
    return (int)rc;
}
}  // namespace

#define PROBE_EXPORT(name, Op)                                                                                                \
    extern "C" int probe_##name##_host(int n, const double* in, double* out) { run_host<Op>(n, in, out); return 0; }          \
    extern "C" int probe_##name##_device(int n, const double* in, double* out) { return run_device<Op>(n, in, out); }         \
    extern "C" int probe_##name##_ni() { return Op::NI; }                                                                     \
    extern "C" int probe_##name##_no() { return Op::NO; }

PROBE_EXPORT(R_to_quat, OpRToQuat)
PROBE_EXPORT(quat_to_R, OpQuatToR)
PROBE_EXPORT(rotvec_to_R, OpRotvecToR)
PROBE_EXPORT(R_to_rotvec, OpRToRotvec)
PROBE_EXPORT(rot_angle, OpRotAngle)
PROBE_EXPORT(rt_project, OpRtProject)
PROBE_EXPORT(mat3_polar, OpMat3Polar)
PROBE_EXPORT(se3_exp, OpSe3Exp)
PROBE_EXPORT(se3_exp_gn, OpSe3ExpGn)
PROBE_EXPORT(se3_log, OpSe3Log)
PROBE_EXPORT(rt_inv, OpRtInv)
PROBE_EXPORT(rt_mul, OpRtMul)
PROBE_EXPORT(mat4_inv, OpMat4Inv)
PROBE_EXPORT(solve6_ldlt, OpSolve6)
