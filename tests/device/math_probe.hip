// math_probe.hip — test infrastructure, not shipped: every device math primitive of emei_amd/csrc/emei_device.h behind an
// elementwise kernel, so that tests/test_gpu_device_math.py can run the code the env kernels really execute (the asm LDS
// read, the magic-number rounding, the hardware seeds, the ballot-guarded cold paths) on its own against exact references.
//
// Built by emei_amd/csrc/Makefile (target `probe`, the flags of the product) into tests/device/libemei_math_probe.so; never
// linked into libemei_hip.so.  The kernels use the primitives the way the product does: 256-thread blocks, the table staged
// into LDS by every thread before any early return, trig_ctx_init, and thread i handles element i — the position of a value
// in the input array is the lane it runs in (the lane-independence tests rely on that).
//
// Launchers: raw device pointers, n, a stream; they return hipGetLastError() of the launch (0 = hipSuccess).
#include "../../emei_amd/csrc/emei_device.h"

using namespace emei;

#define PROBE_API extern "C" __attribute__((visibility("default")))

namespace {

__device__ __forceinline__ int64_t probe_index() { return (int64_t)blockIdx.x * kBlock + threadIdx.x; }

inline dim3 probe_grid(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// ---- trigonometry ------------------------------------------------------------------------------------------------------
// the two-phase table path of the substep: begin -> pin(a, b) -> dependent work -> end(a, b, s, c) -> post (float32's repair)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_sincos_two_phase(const SinCosEntry* __restrict__ tab, double rot_c, double rot_s,
                                                             const T* __restrict__ x, T* __restrict__ s, T* __restrict__ c, int64_t n) {
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, tab, rot_c, rot_s);
    TrigCtx t;
    trig_ctx_init(t, trig_s);
    const int64_t i = probe_index();
    if (i >= n) return;
    const T xi = x[i];
    auto p = sincos_begin_ctx(t, xi);
    T a = xi * T(0.5), b = xi + T(1);
    sincos_pin(p, a, b);
    const T d0 = fma_r(a, b, a), d1 = fma_r(a, a, -b);  // stands for the dynamics that hide the read's latency
    T sn, cs;
    sincos_end_ctx(p, d0, d1, sn, cs);
    sincos_post_ctx(xi, sn, cs);
    s[i] = sn, c[i] = cs;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_sincos_ctx(const SinCosEntry* __restrict__ tab, double rot_c, double rot_s,
                                                       const T* __restrict__ x, T* __restrict__ s, T* __restrict__ c, int64_t n) {
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, tab, rot_c, rot_s);
    TrigCtx t;
    trig_ctx_init(t, trig_s);
    const int64_t i = probe_index();
    if (i >= n) return;
    T sn, cs;
    sincos_ctx(t, x[i], sn, cs);
    s[i] = sn, c[i] = cs;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_sincos_r(const T* __restrict__ x, T* __restrict__ s, T* __restrict__ c, int64_t n) {
    const int64_t i = probe_index();
    if (i >= n) return;
    T sn, cs;
    sincos_r(x[i], sn, cs);
    s[i] = sn, c[i] = cs;
}

__global__ __launch_bounds__(kBlock) void k_trig_reduce_large(const double* __restrict__ x, double* __restrict__ r, int64_t n) {
    const int64_t i = probe_index();
    if (i >= n) return;
    r[i] = trig_reduce_large(x[i]);
}

// ---- reciprocals ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_recip(const T* __restrict__ d, T* __restrict__ rcp, T* __restrict__ rcp1, T* __restrict__ rsq,
                                                  int64_t n) {
    const int64_t i = probe_index();
    if (i >= n) return;
    const T v = d[i];
    rcp[i] = rcp_r(v), rcp1[i] = rcp1_r(v), rsq[i] = rsqrt_r(v);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_div(const T* __restrict__ num, const T* __restrict__ den, T* __restrict__ q, int64_t n) {
    const int64_t i = probe_index();
    if (i >= n) return;
    q[i] = div_r(num[i], den[i]);
}

// ---- angle wrap: wrap_pi and the pymod_pos form it replaces -------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_wrap(const T* __restrict__ theta, T* __restrict__ wrapped, T* __restrict__ pymod, int64_t n) {
    const int64_t i = probe_index();
    if (i >= n) return;
    const T th = theta[i];
    const T pi = T(3.141592653589793);
    wrapped[i] = wrap_pi(th);
    pymod[i] = pymod_pos(th + pi, T(2) * pi, T(1.0 / (2 * 3.141592653589793))) - pi;
}

// ---- random numbers ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_boxmuller(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, float* __restrict__ z0,
                                                      float* __restrict__ z1, int64_t n) {
    const int64_t i = probe_index();
    if (i >= n) return;
    float u, v;
    boxmuller(a[i], b[i], u, v);
    z0[i] = u, z1[i] = v;
}

__global__ __launch_bounds__(kBlock) void k_u01(const uint32_t* __restrict__ r, float* __restrict__ out, int64_t n) {
    const int64_t i = probe_index();
    if (i >= n) return;
    out[i] = u01(r[i]);
}

// the seed is a kernel argument (wave-uniform), as KEYS_IN_PLACE requires
template <bool KEYS_IN_PLACE>
__global__ __launch_bounds__(kBlock) void k_philox(uint64_t seed, const uint64_t* __restrict__ env, const uint32_t* __restrict__ episode,
                                                   const uint32_t* __restrict__ block, uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = probe_index();
    if (i >= n) return;
    const u32x4 r = philox4x32_10<KEYS_IN_PLACE>(seed, env[i], episode[i], block[i]);
    out[4 * i + 0] = r.v[0], out[4 * i + 1] = r.v[1], out[4 * i + 2] = r.v[2], out[4 * i + 3] = r.v[3];
}

}  // namespace

#define PROBE_LAUNCH(kernel, ...)                                            \
    do {                                                                     \
        if (n < 0) return (int)hipErrorInvalidValue;                         \
        if (n == 0) return (int)hipSuccess;                                  \
        kernel<<<probe_grid(n), dim3(kBlock), 0, stream>>>(__VA_ARGS__, n);  \
        return (int)hipGetLastError();                                       \
    } while (0)

PROBE_API int emei_probe_abi_version() { return 1; }

PROBE_API int emei_probe_sincos_two_phase_f64(const void* tab, double rot_c, double rot_s, const double* x, double* s, double* c, int64_t n,
                                              hipStream_t stream) {
    PROBE_LAUNCH(k_sincos_two_phase<double>, (const SinCosEntry*)tab, rot_c, rot_s, x, s, c);
}
PROBE_API int emei_probe_sincos_two_phase_f32(const void* tab, double rot_c, double rot_s, const float* x, float* s, float* c, int64_t n,
                                              hipStream_t stream) {
    PROBE_LAUNCH(k_sincos_two_phase<float>, (const SinCosEntry*)tab, rot_c, rot_s, x, s, c);
}
PROBE_API int emei_probe_sincos_ctx_f64(const void* tab, double rot_c, double rot_s, const double* x, double* s, double* c, int64_t n,
                                        hipStream_t stream) {
    PROBE_LAUNCH(k_sincos_ctx<double>, (const SinCosEntry*)tab, rot_c, rot_s, x, s, c);
}
PROBE_API int emei_probe_sincos_ctx_f32(const void* tab, double rot_c, double rot_s, const float* x, float* s, float* c, int64_t n,
                                        hipStream_t stream) {
    PROBE_LAUNCH(k_sincos_ctx<float>, (const SinCosEntry*)tab, rot_c, rot_s, x, s, c);
}
PROBE_API int emei_probe_sincos_r_f64(const double* x, double* s, double* c, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_sincos_r<double>, x, s, c);
}
PROBE_API int emei_probe_sincos_r_f32(const float* x, float* s, float* c, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_sincos_r<float>, x, s, c);
}
PROBE_API int emei_probe_trig_reduce_large(const double* x, double* r, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_trig_reduce_large, x, r);
}
PROBE_API int emei_probe_recip_f64(const double* d, double* rcp, double* rcp1, double* rsq, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_recip<double>, d, rcp, rcp1, rsq);
}
PROBE_API int emei_probe_recip_f32(const float* d, float* rcp, float* rcp1, float* rsq, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_recip<float>, d, rcp, rcp1, rsq);
}
PROBE_API int emei_probe_div_f64(const double* num, const double* den, double* q, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_div<double>, num, den, q);
}
PROBE_API int emei_probe_div_f32(const float* num, const float* den, float* q, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_div<float>, num, den, q);
}
PROBE_API int emei_probe_wrap_f64(const double* theta, double* wrapped, double* pymod, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_wrap<double>, theta, wrapped, pymod);
}
PROBE_API int emei_probe_wrap_f32(const float* theta, float* wrapped, float* pymod, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_wrap<float>, theta, wrapped, pymod);
}
PROBE_API int emei_probe_boxmuller(const uint32_t* a, const uint32_t* b, float* z0, float* z1, int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_boxmuller, a, b, z0, z1);
}
PROBE_API int emei_probe_u01(const uint32_t* r, float* out, int64_t n, hipStream_t stream) { PROBE_LAUNCH(k_u01, r, out); }
PROBE_API int emei_probe_philox(uint64_t seed, const uint64_t* env, const uint32_t* episode, const uint32_t* block, uint32_t* out, int64_t n,
                                hipStream_t stream) {
    PROBE_LAUNCH(k_philox<false>, seed, env, episode, block, out);
}
PROBE_API int emei_probe_philox_keys_in_place(uint64_t seed, const uint64_t* env, const uint32_t* episode, const uint32_t* block, uint32_t* out,
                                              int64_t n, hipStream_t stream) {
    PROBE_LAUNCH(k_philox<true>, seed, env, episode, block, out);
}
