// top2_probe.hip -- test-only: evaluates top2_update() of csrc/top2.h on N inputs, once on the host and once in a kernel (one
// thread per input), so that tests/test_top2_probe.py can hold both compiles against the sequential three-branch rule the
// function replaces.  Not part of the product library: built by tests/helpers/top2_probe.py into a temporary directory.
//
// One input: the incoming state (11 doubles: bd, b2d, sd, border, b2o, bp xyz, b2p xyz - ids as doubles, exact below 2^32) and
// W slots of 6 doubles (position xyz, d2, id, active != 0); one output: the state in the same layout.
// probe_<name>_host / probe_<name>_device (n, in, out) return 0 or the failing hipError_t.
#include "../../ptudes-lab_amd/csrc/top2.h"

namespace {
constexpr int NSTATE = 11;

template <int W>
struct OpTop2 {
    static constexpr int NI = NSTATE + 6 * W, NO = NSTATE;
    PTL_HD static void f(const double* a, double* o) {
        Top2 s{a[0], a[1], a[2], (unsigned)a[3], (unsigned)a[4], V3{a[5], a[6], a[7]}, V3{a[8], a[9], a[10]}};
        Top2Cand c[W];
        for (int j = 0; j < W; ++j) {
            const double* e = a + NSTATE + 6 * j;
            c[j] = Top2Cand{V3{e[0], e[1], e[2]}, e[3], (unsigned)e[4], e[5] != 0.0};
        }
        s = top2_update(s, c);
        o[0] = s.bd; o[1] = s.b2d; o[2] = s.sd; o[3] = (double)s.border; o[4] = (double)s.b2o;
        o[5] = s.bp.x; o[6] = s.bp.y; o[7] = s.bp.z; o[8] = s.b2p.x; o[9] = s.b2p.y; o[10] = s.b2p.z;
    }
};

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

// the widths scan_voxelsL calls it at: 4 voxels x 3 chunks (first round), 2 x 3 (survivor rounds), 1 (the loop over base)
PROBE_EXPORT(top2_w12, OpTop2<12>)
PROBE_EXPORT(top2_w6, OpTop2<6>)
PROBE_EXPORT(top2_w1, OpTop2<1>)
