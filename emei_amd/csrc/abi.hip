// abi.hip — the extern "C" boundary of libemei_hip.so (declared in include/emei_hip.h).
// Host code only: argument checks, handle bookkeeping, launch dispatch.  No call in a launch path
// allocates, frees or synchronises (HIP-graph capturable).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <new>

#include "launch.h"
#include "body_kernels.h"
#include "cheetah_model.h"
#include "hopper_model.h"
#include "dpend_model.h"

using namespace emei;

struct emei_env {
    emei_config cfg;
    int obs_dim, act_dim, state_dim;
    size_t real_size;
    void* state;
    int32_t* steps;
    uint32_t* episode;
    unsigned long long* done_mask;
    void* frozen_state;
    int32_t* frozen_steps;
    uint32_t* frozen_episode;
    uint64_t frozen_seed;          // key of the reset generator at emei_freeze (restored by emei_unfreeze)
    unsigned long long* cap_hits;  // device counter: Newton solves that ended at the iteration cap (emei_get_solver_cap_hits)
    uint32_t* work;                // body_kernels.h:WorkQueue words of the chunked body rollout (2 + waves of the shard)
    int resident_waves;            // waves of this handle's body rollout kernel the device holds at once (0: not a body / unknown)
    bool has_state, frozen;
    int last_kernel;  // enum emei_kernel_id of the last emei_step / emei_rollout
    uint32_t* host_flag = nullptr;  // emei_step_host: page-locked completion word (allocated on first use) ...
    uint32_t flag_seq = 0;          // ... and the value the next launch stores into it
    PendParams pend;
    const void* trig;
    ObsPeers peers;  // emei_set_obs_peers
};

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(EMEI_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

extern "C" EMEI_API const char* emei_last_error(void) { return g_err; }
extern "C" EMEI_API int emei_abi_version(void) { return EMEI_ABI_VERSION; }

extern "C" EMEI_API int emei_env_dims(int env_id, int* obs_dim, int* act_dim, int* state_dim) {
    int od, ad, sd;
    switch (env_id) {
        case EMEI_CARTPOLE_SWINGUP:
        case EMEI_CARTPOLE_BALANCING: od = 4, ad = 0, sd = 4; break;
        case EMEI_IP_REBOUND_BALANCING:
        case EMEI_IP_BOUNDARY_BALANCING:
        case EMEI_IP_REBOUND_SWINGUP:
        case EMEI_IP_BOUNDARY_SWINGUP: od = 4, ad = 1, sd = 4; break;
        case EMEI_HALFCHEETAH_RUNNING: od = 18, ad = 6, sd = 18; break;
        case EMEI_IDP_REBOUND_BALANCING:
        case EMEI_IDP_BOUNDARY_BALANCING:
        case EMEI_IDP_REBOUND_SWINGUP:
        case EMEI_IDP_BOUNDARY_SWINGUP: od = 6, ad = 1, sd = 6; break;
        case EMEI_HOPPER_RUNNING: od = 12, ad = 3, sd = 12; break;
        default: return fail(EMEI_ERR_INVALID, "unknown env_id %d", env_id);
    }
    if (obs_dim) *obs_dim = od;
    if (act_dim) *act_dim = ad;
    if (state_dim) *state_dim = sd;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_model_constants(int env_id, double* out, int capacity) {
    if (!out || capacity < 0) return fail(EMEI_ERR_INVALID, "emei_model_constants: bad argument");
    double buf[256];
    int n;
    switch (env_id) {
        case EMEI_IP_REBOUND_BALANCING:
        case EMEI_IP_BOUNDARY_BALANCING:
        case EMEI_IP_REBOUND_SWINGUP:
        case EMEI_IP_BOUNDARY_SWINGUP: n = ip_xml_constants(buf); break;
        case EMEI_IDP_REBOUND_BALANCING:
        case EMEI_IDP_BOUNDARY_BALANCING:
        case EMEI_IDP_REBOUND_SWINGUP:
        case EMEI_IDP_BOUNDARY_SWINGUP: n = dpend::xml_constants(buf); break;
        case EMEI_HALFCHEETAH_RUNNING: n = cheetah::xml_constants(buf); break;
        case EMEI_HOPPER_RUNNING: n = hopper::xml_constants(buf); break;
        case EMEI_CARTPOLE_SWINGUP:
        case EMEI_CARTPOLE_BALANCING: return fail(EMEI_ERR_UNSUPPORTED, "emei_model_constants: CartPole has no model file (cartpole.py:22-27)");
        default: return fail(EMEI_ERR_INVALID, "unknown env_id %d", env_id);
    }
    if (n > capacity) return fail(EMEI_ERR_INVALID, "emei_model_constants: %d values, capacity %d", n, capacity);
    memcpy(out, buf, n * sizeof(double));
    return n;
}

extern "C" EMEI_API int emei_model_invweights(int env_id, double* out, int capacity) {
    if (!out || capacity < 0) return fail(EMEI_ERR_INVALID, "emei_model_invweights: bad argument");
    double buf[32];
    int n;
    switch (env_id) {
        case EMEI_IP_REBOUND_BALANCING:
        case EMEI_IP_BOUNDARY_BALANCING:
        case EMEI_IP_REBOUND_SWINGUP:
        case EMEI_IP_BOUNDARY_SWINGUP: {
            constexpr IpModel m = ip_make_model(false);
            buf[0] = m.invw, buf[1] = m.invw_hinge, n = 2;
            break;
        }
        case EMEI_IDP_REBOUND_BALANCING:
        case EMEI_IDP_BOUNDARY_BALANCING:
        case EMEI_IDP_REBOUND_SWINGUP:
        case EMEI_IDP_BOUNDARY_SWINGUP: buf[0] = dpend::make_model(false, 0.002).invw, n = 1; break;
        case EMEI_HALFCHEETAH_RUNNING: n = cheetah::xml_invweights(buf); break;
        case EMEI_HOPPER_RUNNING: n = hopper::xml_invweights(buf); break;
        case EMEI_CARTPOLE_SWINGUP:
        case EMEI_CARTPOLE_BALANCING: return fail(EMEI_ERR_UNSUPPORTED, "emei_model_invweights: CartPole has no constraint rows");
        default: return fail(EMEI_ERR_INVALID, "unknown env_id %d", env_id);
    }
    if (n > capacity) return fail(EMEI_ERR_INVALID, "emei_model_invweights: %d values, capacity %d", n, capacity);
    memcpy(out, buf, n * sizeof(double));
    return n;
}

// ---------------------------------------------------------------------------------------------
// {sin, cos}(k * 2pi/256), k = 0..255, correctly rounded from long double, one copy per device.
// Allocated on the first emei_create / stateless call for that device (never inside a hot launch
// path of an existing handle).
#include <cstddef>
#include <mutex>
namespace emei {
const void* emei_trig_table(int device) {
    static std::mutex mu;
    static void* tabs[64] = {nullptr};
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tabs[device]) {
        SinCosEntry host[kTrigTableSize];
        for (int k = 0; k < kTrigTableSize; ++k) {
            const long double a = 2.0L * 3.141592653589793238462643383279502884L * k / kTrigTableSize;
            host[k].s = (double)sinl(a), host[k].c = (double)cosl(a);
        }
        int prev = 0;
        (void)hipGetDevice(&prev);
        void* d = nullptr;
        if (hipSetDevice(device) == hipSuccess && hipMalloc(&d, sizeof(host)) == hipSuccess &&
            hipMemcpy(d, host, sizeof(host), hipMemcpyHostToDevice) == hipSuccess)
            tabs[device] = d;
        (void)hipSetDevice(prev);
    }
    return tabs[device];
}
}  // namespace emei

static const void* current_device_trig() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    return emei_trig_table(dev);
}

static bool is_pend(int env_id) { return env_id >= EMEI_CARTPOLE_SWINGUP && env_id <= EMEI_IP_BOUNDARY_SWINGUP; }
static bool is_ip(int env_id) { return env_id >= EMEI_IP_REBOUND_BALANCING && env_id <= EMEI_IP_BOUNDARY_SWINGUP; }
// The classic-control envs ignore `integrator` like the reference (base_control.py:73) and have no
// observation noise; an InvertedPendulum with a non-default integrator or observation noise leaves
// the staged 4-state kernel for the generic Body rollout (ipend_model.h).
static bool steps_as_body(const emei_config& c) {
    if (!is_pend(c.env_id)) return true;
    bool obs_noise = false;
    for (int i = 0; i < EMEI_MAX_STATE_DIM; ++i) obs_noise |= c.obs_sigma[i] != 0.f;
    return is_ip(c.env_id) && (c.integrator != EMEI_INTEG_EULER || obs_noise);
}
static bool is_body(int env_id) { return env_id >= EMEI_HALFCHEETAH_RUNNING && env_id <= EMEI_HOPPER_RUNNING; }
static bool is_idp(int env_id) {
    return env_id == EMEI_IDP_REBOUND_BALANCING || env_id == EMEI_IDP_BOUNDARY_BALANCING || env_id == EMEI_IDP_REBOUND_SWINGUP ||
           env_id == EMEI_IDP_BOUNDARY_SWINGUP;
}

// ---------------------------------------------------------------------------------------------
// Host twin of the InvertedPendulum constants for the launch descriptors: every number comes from pendulum_envs.h:
// ip_make_model (the one typed copy of emei/envs/mujoco/assets/inverted_pendulum.xml on the kernel side).
static PendParams pend_params(int env_id, double dt, const float* init_sigma = nullptr, int noise_shared = 0) {
    PendParams p;
    memset(&p, 0, sizeof(p));
    p.dt = dt;
    p.dt32 = (float)dt;
    for (int i = 0; i < 4; ++i) p.init_sigma[i] = init_sigma ? init_sigma[i] : 0.f;
    p.noise_shared = noise_shared;
    const bool swingup = env_id == EMEI_IP_REBOUND_SWINGUP || env_id == EMEI_IP_BOUNDARY_SWINGUP;
    const IpModel x = ip_make_model(swingup);
    p.M11 = x.M11, p.M22 = x.M22, p.mpr = x.mpr, p.mgr = x.mp * x.gravity * x.r;
    p.gear = x.gear, p.ctrl_lo = x.ctrl_lo, p.ctrl_hi = x.ctrl_hi, p.x_lo = x.x_lo, p.x_hi = x.x_hi;
    p.phi_off = x.phi_off, p.sin_off = x.sin_off, p.cos_off = x.cos_off;  // _update_model: pole body turned by pi about y
    p.invw = x.invw;                                                      // dof_invweight0 of the slider at qpos0
    p.tc = x.solref_tc < 2 * dt ? 2 * dt : x.solref_tc;                   // solref timeconst with MuJoCo's refsafe clamp
    p.dampratio = 1.0, p.dmin = x.dmin, p.dmax = x.dmax, p.width = x.width;
    p.limK = 1.0 / (p.dmax * p.dmax * p.tc * p.tc * p.dampratio * p.dampratio), p.limB = 2.0 / (p.dmax * p.tc);
    return p;
}

// ---------------------------------------------------------------------------------------------
extern "C" EMEI_API int emei_create(const emei_config* cfg, emei_env** out) {
    if (!cfg || !out) return fail(EMEI_ERR_INVALID, "emei_create: null argument");
    // older callers pass a shorter struct: every tail field has an all-zero default
    const uint32_t size_v2a = (uint32_t)offsetof(emei_config, env_param_mask);  // 328: before env_params existed
    const uint32_t size_v5 = (uint32_t)offsetof(emei_config, ode_method);       // 400: before ode_method / rollout_chunk_steps
    if (cfg->struct_size != sizeof(emei_config) && cfg->struct_size != size_v5 && cfg->struct_size != size_v2a &&
        cfg->struct_size != EMEI_CONFIG_SIZE_V1)
        return fail(EMEI_ERR_INVALID, "emei_create: emei_config size %u, library expects %zu (or the older sizes %u / %u / %u)",
                    cfg->struct_size, sizeof(emei_config), size_v5, size_v2a, EMEI_CONFIG_SIZE_V1);
    emei_config c2;  // the caller's struct, widened to this library's layout
    memset(&c2, 0, sizeof(c2));
    memcpy(&c2, cfg, cfg->struct_size);
    if (cfg->struct_size == EMEI_CONFIG_SIZE_V1)
        for (int i = 0; i < EMEI_MAX_STATE_DIM; ++i) c2.init_sigma[i] = (float)c2.init_noise;
    c2.struct_size = sizeof(emei_config);
    cfg = &c2;
    if (cfg->integrator < EMEI_INTEG_EULER || cfg->integrator > EMEI_INTEG_RK4)
        return fail(EMEI_ERR_UNSUPPORTED, "emei_create: integrator=%d", cfg->integrator);  // mujoco_env.py:78-79
    if (cfg->noise_layout != EMEI_NOISE_IID && cfg->noise_layout != EMEI_NOISE_SHARED)
        return fail(EMEI_ERR_INVALID, "emei_create: noise_layout=%d", cfg->noise_layout);
    for (int i = 0; i < EMEI_MAX_STATE_DIM; ++i)
        if (!(cfg->init_sigma[i] >= 0) || !(cfg->obs_sigma[i] >= 0))
            return fail(EMEI_ERR_INVALID, "emei_create: noise sigmas must be >= 0");
    if (cfg->ode_method != EMEI_ODE_EULER && cfg->ode_method != EMEI_ODE_RK4)
        return fail(EMEI_ERR_UNSUPPORTED, "emei_create: ode_method=%d", cfg->ode_method);  // base_control.py:171-172
    if (cfg->ode_method != EMEI_ODE_EULER && cfg->env_id != EMEI_CARTPOLE_SWINGUP && cfg->env_id != EMEI_CARTPOLE_BALANCING)
        return fail(EMEI_ERR_INVALID, "emei_create: ode_method is ODE_approximation's switch (classic control); env_id %d is integrated "
                    "according to `integrator`", cfg->env_id);
    if (cfg->rollout_chunk_steps < -1 && (cfg->rollout_chunk_steps > -101 || cfg->rollout_chunk_steps < -1506 ||
                                          -cfg->rollout_chunk_steps % 100 < 1 || -cfg->rollout_chunk_steps % 100 > 6)) return fail(EMEI_ERR_INVALID, "emei_create: rollout_chunk_steps=%d", cfg->rollout_chunk_steps);
    if (cfg->solver != EMEI_SOLVER_NEWTON && cfg->solver != EMEI_SOLVER_SWEEP1) return fail(EMEI_ERR_INVALID, "emei_create: solver=%u", cfg->solver);
    if (cfg->env_param_mask >> EMEI_MAX_ENV_PARAMS) return fail(EMEI_ERR_INVALID, "emei_create: env_param_mask=0x%x", cfg->env_param_mask);
    if (cfg->env_param_mask != 0 && cfg->env_id != EMEI_HALFCHEETAH_RUNNING && cfg->env_id != EMEI_HOPPER_RUNNING)
        return fail(EMEI_ERR_UNSUPPORTED, "emei_create: env_id %d takes no reward / health parameters", cfg->env_id);
    if (cfg->env_id == EMEI_HALFCHEETAH_RUNNING && (cfg->env_param_mask >> 2))
        return fail(EMEI_ERR_INVALID, "emei_create: HalfCheetahRunning has only the two reward weights");
    int od, ad, sd;
    if (emei_env_dims(cfg->env_id, &od, &ad, &sd) != EMEI_OK) return EMEI_ERR_INVALID;
    // the kernels index envs with uint32_t lane indices and int32 done lists: n_envs < 2^31
    if (cfg->n_envs <= 0 || cfg->n_envs >= (int64_t)1 << 31)
        return fail(EMEI_ERR_INVALID, "emei_create: n_envs=%lld out of range", (long long)cfg->n_envs);
    if (cfg->freq_rate < 1) return fail(EMEI_ERR_INVALID, "emei_create: freq_rate=%d < 1", cfg->freq_rate);
    if (!(cfg->real_time_scale > 0)) return fail(EMEI_ERR_INVALID, "emei_create: real_time_scale must be > 0");
    if (cfg->precision != EMEI_PRECISION_REF && cfg->precision != EMEI_PRECISION_F32)
        return fail(EMEI_ERR_INVALID, "emei_create: precision=%d", cfg->precision);
    if (cfg->max_episode_steps < 0) return fail(EMEI_ERR_INVALID, "emei_create: max_episode_steps < 0");
    int prev_device = 0;
    HIP_TRY(hipGetDevice(&prev_device));
    HIP_TRY(hipSetDevice(cfg->device));
    struct RestoreDevice {  // emei_create leaves the caller's current device as it found it
        int d;
        ~RestoreDevice() { (void)hipSetDevice(d); }
    } restore{prev_device};

    emei_env* h = new (std::nothrow) emei_env();
    if (!h) return fail(EMEI_ERR_INVALID, "emei_create: out of host memory");
    memset(h, 0, sizeof(*h));
    h->cfg = *cfg;
    h->obs_dim = od, h->act_dim = ad, h->state_dim = sd;
    h->real_size = cfg->precision == EMEI_PRECISION_F32 ? sizeof(float) : sizeof(double);
    const size_t n = (size_t)cfg->n_envs, n_words = (n + kWave - 1) / kWave;
    const size_t state_bytes = n * sd * h->real_size;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc(&h->state, state_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&h->steps, n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->episode, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->done_mask, n_words * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&h->frozen_state, state_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&h->frozen_steps, n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->frozen_episode, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->cap_hits, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(h->cap_hits, 0, sizeof(unsigned long long));
    if (e == hipSuccess && steps_as_body(*cfg)) {
        // (2 + waves words of the queue; a second `waves` words are scratch of probe builds: body_kernels.h, EMEI_CLOCK_HIST_CORR)
        e = hipMalloc((void**)&h->work, (2 + 2 * n_words) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(h->work, 0, (2 + 2 * n_words) * sizeof(uint32_t));
    }
    if (e == hipSuccess) e = hipMemset(h->done_mask, 0, n_words * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(h->steps, 0, n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->episode, 0, n * sizeof(uint32_t));
    if (e != hipSuccess) {
        emei_destroy(h);
        return fail(EMEI_ERR_HIP, "emei_create: allocation failed: %s", hipGetErrorString(e));
    }
    if (is_pend(cfg->env_id))
        h->pend = pend_params(cfg->env_id, cfg->real_time_scale, cfg->init_sigma, cfg->noise_layout);
    h->trig = emei_trig_table(cfg->device);
    if (!h->trig) {
        emei_destroy(h);
        return fail(EMEI_ERR_HIP, "emei_create: could not build the trig table on device %d", cfg->device);
    }
    if (steps_as_body(*cfg)) {  // occupancy of the rollout kernel: the automatic chunking policy (body_kernels.h:WorkQueue)
        BodyLaunch L;
        L.op = OP_OCCUPANCY, L.env_id = cfg->env_id, L.precision = cfg->precision, L.integrator = cfg->integrator;
        L.solver = (int)cfg->solver, L.selected = &h->resident_waves;
        if (body_launch(L) != EMEI_OK) h->resident_waves = 0;  // unknown: the automatic policy then stays with one-piece launches
    }
    *out = h;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_destroy(emei_env* h) {
    if (!h) return EMEI_OK;
    (void)hipFree(h->state);
    (void)hipFree(h->steps);
    (void)hipFree(h->episode);
    (void)hipFree(h->done_mask);
    (void)hipFree(h->frozen_state);
    (void)hipFree(h->frozen_steps);
    (void)hipFree(h->frozen_episode);
    (void)hipFree(h->cap_hits);
    (void)hipFree(h->work);
    if (h->host_flag) (void)hipHostFree(h->host_flag);
    delete h;
    return EMEI_OK;
}

// One handle <-> one device: every launch of a handle goes to the CALLER's current device, so a handle used
// while another device is current would touch memory of the wrong GPU.  Refused up front.
static int wrong_device(const emei_env* h, const char* fn) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return fail(EMEI_ERR_HIP, "%s: hipGetDevice failed", fn);
    if (dev != h->cfg.device)
        return fail(EMEI_ERR_INVALID, "%s: the handle belongs to device %d but device %d is current", fn, h->cfg.device, dev);
    return EMEI_OK;
}
#define EMEI_ON_DEVICE(h, fn)                                  \
    do {                                                        \
        if (int rc_ = wrong_device((h), (fn))) return rc_;      \
    } while (0)

// The handle's part of a launch descriptor, laid under the call's own fields in `L` (L.n != 0: a count of the call's own)
static void handle_fields(const emei_env* h, void* stream, LaunchCommon& L) {
    L.env_id = h->cfg.env_id;
    L.precision = h->cfg.precision;
    L.state = h->state;
    L.steps = h->steps;
    L.episode = h->episode;
    L.done_mask = h->done_mask;
    if (L.n == 0) L.n = h->cfg.n_envs;
    L.freq_rate = h->cfg.freq_rate;
    L.max_episode_steps = h->cfg.max_episode_steps;
    L.seed = h->cfg.seed;
    L.env_offset = h->cfg.env_index_offset;
    L.trig = h->trig;
    L.stream = (hipStream_t)stream;
}

static PendLaunch pend_base(emei_env* h, void* stream, const LaunchCommon& call = LaunchCommon()) {
    PendLaunch L;
    static_cast<LaunchCommon&>(L) = call;
    handle_fields(h, stream, L);
    L.ode_method = h->cfg.ode_method;
    L.p = h->pend;
    L.peers = h->peers;
    return L;
}

static BodyLaunch body_base(emei_env* h, void* stream, const LaunchCommon& call = LaunchCommon()) {
    BodyLaunch L;
    static_cast<LaunchCommon&>(L) = call;
    handle_fields(h, stream, L);
    L.dt = h->cfg.real_time_scale;
    L.integrator = h->cfg.integrator;
    L.solver = (int)h->cfg.solver;
    memcpy(L.noise.init, h->cfg.init_sigma, sizeof(L.noise.init));
    memcpy(L.noise.obs, h->cfg.obs_sigma, sizeof(L.noise.obs));
    L.noise.shared = h->cfg.noise_layout == EMEI_NOISE_SHARED;
    L.env_params.mask = h->cfg.env_param_mask;
    memcpy(L.env_params.v, h->cfg.env_params, sizeof(L.env_params.v));
    L.cap_hits = h->cap_hits;
    L.work = h->work, L.chunk_steps = h->cfg.rollout_chunk_steps, L.resident_waves = h->resident_waves;
    return L;
}

// THE family launch: every launch on a handle but emei_step_host's goes through here.  `call` holds the op and the call's own
// fields (launch.h: LaunchOp), action_dtype the dtype of the actions a 4-state kernel reads or writes.  The ops that step or plan go
// to the family emei_rollout runs for this handle (steps_as_body); reset, get_obs and init_obs touch the state alone and stay with
// the env's own family, which for an InvertedPendulum on the body kernels is the other one.  The ops that step the handle report
// their kernel (emei_last_rollout_kernel); the queries leave the handle as it is.
static int launch(emei_env* h, const LaunchCommon& call, void* stream, int action_dtype = 0) {
    const int op = call.op;
    const bool state_only = op == OP_RESET || op == OP_GET_OBS || op == OP_INIT_OBS;
    const bool steps = op == OP_ROLLOUT || op == OP_MPC_MPPI || op == OP_MPC_CEM || op == OP_MPC_POLICY || op == OP_POLICY ||
                       op == OP_POLICY_NOISY || op == OP_POLICY_DEEP;
    int* const selected = steps ? &h->last_kernel : nullptr;
    const bool on_body = state_only ? !is_pend(h->cfg.env_id) : steps_as_body(h->cfg);
    if (!on_body) {
        PendLaunch L = pend_base(h, stream, call);
        L.action_dtype = action_dtype, L.selected = selected;
        return pend_launch(L);
    }
    BodyLaunch L = body_base(h, stream, call);
    L.selected = selected;
    return body_launch(L);
}

// the tail of the entry points that launch: `rc` as the launches left it
static int launched(const char* fn, int rc) {
    return rc == EMEI_OK ? rc : fail(rc, "%s: launch failed (%s)", fn, hipGetErrorString(hipGetLastError()));
}

static int check_flags(const char* fn, uint32_t flags) {
    if (flags & ~EMEI_FLAG_AUTO_RESET) return fail(EMEI_ERR_INVALID, "%s: unknown flags 0x%x", fn, flags);
    return EMEI_OK;
}

extern "C" EMEI_API int emei_reset(emei_env* h, uint64_t seed, void* stream) {
    if (!h) return fail(EMEI_ERR_INVALID, "emei_reset: null handle");
    EMEI_ON_DEVICE(h, "emei_reset");
    h->cfg.seed = seed;
    LaunchCommon c;
    c.op = OP_RESET;
    const int rc = launch(h, c, stream);
    if (rc != EMEI_OK) return fail(rc, "emei_reset: launch failed");
    h->has_state = true;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_set_seed(emei_env* h, uint64_t seed) {
    if (!h) return fail(EMEI_ERR_INVALID, "emei_set_seed: null handle");
    h->cfg.seed = seed;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_last_rollout_kernel(emei_env* h) {
    if (!h) return fail(EMEI_ERR_INVALID, "emei_last_rollout_kernel: null handle");
    return h->last_kernel;
}

extern "C" EMEI_API int emei_set_state(emei_env* h, const double* state_aos, int reset_counters, void* stream) {
    if (!h || !state_aos) return fail(EMEI_ERR_INVALID, "emei_set_state: null argument");
    EMEI_ON_DEVICE(h, "emei_set_state");
    int rc = launch_state_unpack(state_aos, h->state, h->cfg.precision, h->cfg.n_envs, h->state_dim, (hipStream_t)stream);
    if (rc != EMEI_OK) return fail(rc, "emei_set_state: launch failed");
    if (reset_counters) {
        HIP_TRY(hipMemsetAsync(h->steps, 0, (size_t)h->cfg.n_envs * sizeof(int32_t), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(h->episode, 0, (size_t)h->cfg.n_envs * sizeof(uint32_t), (hipStream_t)stream));
    }
    h->has_state = true;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_get_state(emei_env* h, double* state_aos, void* stream) {
    if (!h || !state_aos) return fail(EMEI_ERR_INVALID, "emei_get_state: null argument");
    EMEI_ON_DEVICE(h, "emei_get_state");
    if (!h->has_state) return fail(EMEI_ERR_STATE, "emei_get_state: call reset before using the state");
    int rc = launch_state_pack(h->state, state_aos, h->cfg.precision, h->cfg.n_envs, h->state_dim, (hipStream_t)stream);
    return rc == EMEI_OK ? rc : fail(rc, "emei_get_state: launch failed");
}

extern "C" EMEI_API int emei_get_obs(emei_env* h, double* obs_aos, void* stream) {
    if (!h || !obs_aos) return fail(EMEI_ERR_INVALID, "emei_get_obs: null argument");
    EMEI_ON_DEVICE(h, "emei_get_obs");
    if (!h->has_state) return fail(EMEI_ERR_STATE, "emei_get_obs: call reset before using the state");
    LaunchCommon c;
    c.op = OP_GET_OBS, c.obs_f64 = obs_aos;
    const int rc = launch(h, c, stream);
    return rc == EMEI_OK ? rc : fail(rc, "emei_get_obs: launch failed");
}

extern "C" EMEI_API int emei_freeze(emei_env* h, void* stream) {
    if (!h) return fail(EMEI_ERR_INVALID, "emei_freeze: null handle");
    EMEI_ON_DEVICE(h, "emei_freeze");
    if (!h->has_state) return fail(EMEI_ERR_STATE, "emei_freeze: no state to freeze (call reset first)");
    const size_t n = (size_t)h->cfg.n_envs;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->frozen_state, h->state, n * h->state_dim * h->real_size, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->frozen_steps, h->steps, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->frozen_episode, h->episode, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    h->frozen_seed = h->cfg.seed;  // a reset(seed=) between freeze and unfreeze must not re-key the restored episodes
    h->frozen = true;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_unfreeze(emei_env* h, void* stream) {
    if (!h) return fail(EMEI_ERR_INVALID, "emei_unfreeze: null handle");
    EMEI_ON_DEVICE(h, "emei_unfreeze");
    if (!h->frozen) return fail(EMEI_ERR_STATE, "emei_unfreeze: env has not been frozen");
    const size_t n = (size_t)h->cfg.n_envs;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->state, h->frozen_state, n * h->state_dim * h->real_size, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->steps, h->frozen_steps, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->episode, h->frozen_episode, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    h->cfg.seed = h->frozen_seed;
    h->frozen = false;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_get_solver_cap_hits(emei_env* h, uint64_t* count_out, void* stream) {
    if (!h || !count_out) return fail(EMEI_ERR_INVALID, "emei_get_solver_cap_hits: null argument");
    EMEI_ON_DEVICE(h, "emei_get_solver_cap_hits");
    HIP_TRY(hipMemcpyAsync(count_out, h->cap_hits, sizeof(uint64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return EMEI_OK;
}

extern "C" EMEI_API int emei_get_rollout_faults(emei_env* h, uint64_t* count_out, void* stream) {
    if (!h || !count_out) return fail(EMEI_ERR_INVALID, "emei_get_rollout_faults: null argument");
    EMEI_ON_DEVICE(h, "emei_get_rollout_faults");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(count_out, 0, sizeof(uint64_t), s));
    if (h->work) HIP_TRY(hipMemcpyAsync(count_out, h->work + WorkQueue::kFaults, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));  // little endian
    return EMEI_OK;
}

extern "C" EMEI_API int emei_set_obs_peers(emei_env* h, int n_peers, void* const* peer_obs, int64_t row_envs, int64_t col_offset, int32_t max_steps) {
    if (!h) return fail(EMEI_ERR_INVALID, "emei_set_obs_peers: null handle");
    if (n_peers == 0) {
        h->peers = ObsPeers();
        return EMEI_OK;
    }
    if (n_peers < 0 || n_peers > EMEI_MAX_OBS_PEERS) return fail(EMEI_ERR_INVALID, "emei_set_obs_peers: n_peers=%d outside 0..%d", n_peers, EMEI_MAX_OBS_PEERS);
    if (!peer_obs) return fail(EMEI_ERR_INVALID, "emei_set_obs_peers: null pointer list");
    if (max_steps < 1) return fail(EMEI_ERR_INVALID, "emei_set_obs_peers: max_steps=%d < 1", max_steps);
    if (col_offset < 0 || row_envs < col_offset + h->cfg.n_envs)
        return fail(EMEI_ERR_INVALID, "emei_set_obs_peers: columns [%lld, %lld) do not fit a row of %lld envs", (long long)col_offset,
                    (long long)(col_offset + h->cfg.n_envs), (long long)row_envs);
    if (steps_as_body(h->cfg) || h->obs_dim != 4 || h->cfg.env_id > EMEI_CARTPOLE_BALANCING)
        return fail(EMEI_ERR_UNSUPPORTED, "emei_set_obs_peers: built for the CartPole family (env_id %d)", h->cfg.env_id);
    ObsPeers P;
    for (int p = 0; p < n_peers; ++p) {
        if (!peer_obs[p] || ((uintptr_t)peer_obs[p] & 15u)) return fail(EMEI_ERR_INVALID, "emei_set_obs_peers: peer %d is null or not 16-byte aligned", p);
        P.obs[p] = peer_obs[p];
    }
    P.row_envs = row_envs, P.col = col_offset, P.count = n_peers, P.max_steps = max_steps;
    h->peers = P;
    return EMEI_OK;
}

// Device memory another process of this node can map (hipIpc): see include/emei_hip.h
static_assert(sizeof(hipIpcMemHandle_t) == sizeof(emei_ipc_handle), "hipIpcMemHandle_t is 64 opaque bytes");
struct DeviceScope {  // the calls below act on the caller's device and leave the current device as they found it
    int prev = -1;
    hipError_t err;
    explicit DeviceScope(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) err = hipSetDevice(device);
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

extern "C" EMEI_API int emei_peer_buffer_create(int device, uint64_t bytes, void** dev_ptr_out, emei_ipc_handle* handle_out) {
    if (!dev_ptr_out || !handle_out || bytes == 0) return fail(EMEI_ERR_INVALID, "emei_peer_buffer_create: bad argument");
    DeviceScope scope(device);
    HIP_TRY(scope.err);
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    hipIpcMemHandle_t hnd;
    hipError_t e = hipIpcGetMemHandle(&hnd, p);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(EMEI_ERR_HIP, "hipIpcGetMemHandle: %s (HSA_ENABLE_IPC_MODE_LEGACY=0 is needed where the host driver only has dmabuf IPC)", hipGetErrorString(e));
    }
    memcpy(handle_out->bytes, &hnd, sizeof(hnd));
    *dev_ptr_out = p;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_peer_buffer_open(int device, const emei_ipc_handle* handle, void** dev_ptr_out) {
    if (!handle || !dev_ptr_out) return fail(EMEI_ERR_INVALID, "emei_peer_buffer_open: null argument");
    DeviceScope scope(device);
    HIP_TRY(scope.err);
    hipIpcMemHandle_t hnd;
    memcpy(&hnd, handle->bytes, sizeof(hnd));
    void* p = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&p, hnd, hipIpcMemLazyEnablePeerAccess));
    *dev_ptr_out = p;
    return EMEI_OK;
}

extern "C" EMEI_API int emei_peer_buffer_close(int device, void* dev_ptr) {
    if (!dev_ptr) return fail(EMEI_ERR_INVALID, "emei_peer_buffer_close: null pointer");
    DeviceScope scope(device);
    HIP_TRY(scope.err);
    HIP_TRY(hipIpcCloseMemHandle(dev_ptr));
    return EMEI_OK;
}

extern "C" EMEI_API int emei_peer_buffer_destroy(int device, void* dev_ptr) {
    if (!dev_ptr) return fail(EMEI_ERR_INVALID, "emei_peer_buffer_destroy: null pointer");
    DeviceScope scope(device);
    HIP_TRY(scope.err);
    HIP_TRY(hipFree(dev_ptr));
    return EMEI_OK;
}

static int check_action_dtype(const emei_env* h, int action_dtype) {
    if (action_dtype < EMEI_ACT_U8 || action_dtype > EMEI_ACT_F32) return fail(EMEI_ERR_INVALID, "bad action_dtype %d", action_dtype);
    int od, ad, sd;
    emei_env_dims(h->cfg.env_id, &od, &ad, &sd);
    if (ad > 0 && action_dtype != EMEI_ACT_F32)
        return fail(EMEI_ERR_INVALID, "continuous-action envs take float32 actions [n,%d]", ad);
    if (ad == 0 && action_dtype == EMEI_ACT_F32)
        return fail(EMEI_ERR_INVALID, "discrete-action envs take uint8/int32/int64 actions [n]");
    return EMEI_OK;
}

extern "C" EMEI_API int emei_rollout(emei_env* h, int32_t n_steps, const void* actions, int action_dtype, float* obs_out,
                            float* reward_out, uint8_t* done_out, uint32_t flags, void* stream) {
    if (!h || !actions) return fail(EMEI_ERR_INVALID, "emei_rollout: null argument");
    EMEI_ON_DEVICE(h, "emei_rollout");
    if (n_steps < 1) return fail(EMEI_ERR_INVALID, "emei_rollout: n_steps=%d < 1", n_steps);
    if (!h->has_state) return fail(EMEI_ERR_STATE, "Call reset before using step method.");  // base_control.py:67
    if (int rc = check_flags("emei_rollout", flags)) return rc;
    if (check_action_dtype(h, action_dtype) != EMEI_OK) return EMEI_ERR_INVALID;
    if (h->peers.count > 0 && n_steps > h->peers.max_steps)
        return fail(EMEI_ERR_INVALID, "emei_rollout: n_steps=%d but the registered observation peers hold %d rows (emei_set_obs_peers)", n_steps,
                    h->peers.max_steps);
    if (h->peers.count > 0 && steps_as_body(h->cfg))
        return fail(EMEI_ERR_UNSUPPORTED, "emei_rollout: observation peers are set (emei_set_obs_peers), which the body kernels do not serve");
    LaunchCommon c;
    c.op = OP_ROLLOUT;
    c.actions = actions;
    c.obs_out = obs_out, c.reward_out = reward_out, c.done_out = done_out;
    c.n_steps = n_steps;
    c.flags = flags;
    const int rc = launch(h, c, stream, action_dtype);
    if (rc == EMEI_ERR_UNSUPPORTED && h->peers.count > 0)
        return fail(rc, "emei_rollout: observation peers are set (emei_set_obs_peers), which only the staged kernel of the CartPole family "
                        "serves: n_envs a multiple of 64, n_steps >= 16, all three outputs, 16-byte aligned buffers (n_envs=%lld, n_steps=%d)",
                    (long long)h->cfg.n_envs, n_steps);
    return launched("emei_rollout", rc);
}

extern "C" EMEI_API int emei_step_host(emei_env* h, const void* actions_host, int action_dtype, double* obs64_host, float* obs32_host,
                                       float* reward_host, uint8_t* done_host, uint32_t flags, void* stream) {
    if (!h || !actions_host || !obs64_host || !obs32_host || !reward_host || !done_host)
        return fail(EMEI_ERR_INVALID, "emei_step_host: null argument");
    EMEI_ON_DEVICE(h, "emei_step_host");
    if (!h->has_state) return fail(EMEI_ERR_STATE, "Call reset before using step method.");  // base_control.py:67
    if (int rc = check_flags("emei_step_host", flags)) return rc;
    if (check_action_dtype(h, action_dtype) != EMEI_OK) return EMEI_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (!steps_as_body(h->cfg) && h->cfg.n_envs == 1) {
        // ONE launch: the generic rollout kernel also writes the float64 observation and ends with a completion word
        if (!h->host_flag) {
            HIP_TRY(hipHostMalloc((void**)&h->host_flag, 64, hipHostMallocDefault));
            *h->host_flag = 0;
        }
        PendLaunch L = pend_base(h, stream);
        L.op = OP_ROLLOUT;
        L.actions = actions_host;
        L.action_dtype = action_dtype;
        L.obs_out = obs32_host, L.reward_out = reward_host, L.done_out = done_host, L.obs_f64 = obs64_host;
        L.n_steps = 1;
        L.flags = flags;
        L.selected = &h->last_kernel;
        L.host_flag = h->host_flag;
        L.flag_value = ++h->flag_seq;
        if (L.flag_value == 0) L.flag_value = ++h->flag_seq;  // 0 is the word's initial content
        int rc = pend_launch(L);
        if (rc != EMEI_OK) return launched("emei_step_host", rc);
        // poll the word (the kernel's last store, system scope); a launch that does not finish within ~5 ms is handed to the
        // runtime's own wait, which also surfaces a device fault
        volatile uint32_t* flag = h->host_flag;
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int spin = 0;; ++spin) {
            if (*flag == L.flag_value) {
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                return EMEI_OK;
            }
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#else
            __asm__ __volatile__("" ::: "memory");
#endif
            if ((spin & 1023) == 1023) {  // the bound is wall time (a pause is 40-140 cycles depending on the part), checked every 1024 spins
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec) > 5000000ll) break;
            }
        }
        HIP_TRY(hipStreamSynchronize(s));
        return *flag == L.flag_value ? EMEI_OK : fail(EMEI_ERR_HIP, "emei_step_host: the kernel finished without its completion word");
    }
    int rc = emei_rollout(h, 1, actions_host, action_dtype, obs32_host, reward_host, done_host, flags, stream);
    if (rc != EMEI_OK) return rc;
    rc = emei_get_obs(h, obs64_host, stream);
    if (rc != EMEI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return EMEI_OK;
}

extern "C" EMEI_API int emei_step(emei_env* h, const void* actions, int action_dtype, float* obs_out, float* reward_out,
                         uint8_t* done_out, uint32_t flags, void* stream) {
    return emei_rollout(h, 1, actions, action_dtype, obs_out, reward_out, done_out, flags, stream);
}

// ---------------------------------------------------------------------------------------------
// The planner entry points refuse in one order: the scalars (without a handle and before any HIP call), the handle, what needs the
// handle, the call's own pointers, the device, the state.  The refusals more than one of them makes:
// (`count`: what the call names its lanes-per-env argument)
static int check_plan_scalars(const char* fn, int32_t horizon, int32_t n_candidates, double discount, const char* count = "n_candidates") {
    if (horizon < 1) return fail(EMEI_ERR_INVALID, "%s: horizon=%d < 1", fn, horizon);
    if (n_candidates < 1) return fail(EMEI_ERR_INVALID, "%s: %s=%d < 1", fn, count, n_candidates);
    if (!(discount > 0.0 && discount <= 1.0)) return fail(EMEI_ERR_INVALID, "%s: discount=%g is outside (0, 1]", fn, discount);
    return EMEI_OK;
}

static int check_temperature(const char* fn, double temperature) {
    if (!(std::isfinite(temperature) && temperature > 0.0))
        return fail(EMEI_ERR_INVALID, "%s: temperature=%g must be finite and > 0", fn, temperature);
    return EMEI_OK;
}

// one lane per candidate, 32-bit lane indices (as emei_create's bound on n_envs)
static int check_plan_lanes(const char* fn, const emei_env* h, int32_t n_candidates) {
    const int64_t nk = h->cfg.n_envs * (int64_t)n_candidates;
    if (nk > INT32_MAX) return fail(EMEI_ERR_INVALID, "%s: n_envs * n_candidates = %lld exceeds 2^31 - 1", fn, (long long)nk);
    return EMEI_OK;
}

// of the *_workspace_bytes functions -> n_envs * n_candidates, or the refusal's (negative) code
static int64_t check_plan_shape(const char* fn, int64_t n_envs, int32_t n_candidates) {
    if (n_envs < 1 || n_envs > INT32_MAX) return fail(EMEI_ERR_INVALID, "%s: n_envs=%lld", fn, (long long)n_envs);
    if (n_candidates < 1) return fail(EMEI_ERR_INVALID, "%s: n_candidates=%d < 1", fn, n_candidates);
    const int64_t nk = n_envs * (int64_t)n_candidates;
    if (nk > INT32_MAX) return fail(EMEI_ERR_INVALID, "%s: n_envs * n_candidates = %lld exceeds 2^31 - 1", fn, (long long)nk);
    return nk;
}

// The workspace of the drawn plans starts with one PlanPartial per (wave, env) segment of the plan kernel: at most waves + envs of
// them (emei_device.h:plan_reduce_wave).  emei_plan_mppi / emei_plan_cem keep nk float64 returns / weights behind them.
static int64_t plan_partials_bytes(int64_t n_envs, int64_t nk) {
    static_assert(sizeof(PlanPartial) % 16 == 0, "the returns behind the partials stay 16-byte aligned");
    return (int64_t)sizeof(PlanPartial) * ((nk + kWave - 1) / kWave + n_envs);
}
static double* plan_returns(const emei_env* h, int32_t n_candidates, void* workspace) {
    return (double*)((char*)workspace + plan_partials_bytes(h->cfg.n_envs, h->cfg.n_envs * (int64_t)n_candidates));
}

// The *_value twins of the four open-loop plan calls share their plain call's body: `with_value` adds the terminal value's refusals
// between the scalars and the handle (check_plan_value) and sends the first launch to OP_PLAN_VALUE.  The struct helpers are the
// deep policy calls' (below).
static int check_policy_deep_struct(const char* fn, const char* arg, const emei_policy_deep* policy, bool with_out_mode = true);
static int check_policy_deep_weights(const char* fn, const char* arg, const emei_policy_deep* policy);
static PolicyDeepArgs policy_value_args(const emei_policy_deep* value);

// NULL value, value.struct_size, .hidden1, .hidden2, .reserved; a NULL handle; NULL value w1 .. b3
static int check_plan_value(const char* fn, const emei_env* h, const emei_policy_deep* value) {
    if (int rc = check_policy_deep_struct(fn, "value", value, false)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    return check_policy_deep_weights(fn, "value", value);
}

// what every OP_PLAN / OP_PLAN_VALUE call sets alike (launch.h: PlanMode); value: the checked terminal value, or null for OP_PLAN
static LaunchCommon plan_call(int mode, const double* start_rows, int32_t horizon, int32_t n_candidates, double discount,
                              const emei_policy_deep* value) {
    LaunchCommon c;
    c.op = value ? OP_PLAN_VALUE : OP_PLAN, c.n_steps = horizon;
    c.plan.mode = mode, c.plan.start_rows = start_rows, c.plan.n_candidates = n_candidates, c.plan.discount = discount;
    c.policy_value = policy_value_args(value);
    return c;
}

static int evaluate_sequences(const char* fn, bool with_value, emei_env* h, int32_t horizon, int32_t n_candidates, const void* actions,
                              int action_dtype, double discount, const emei_policy_deep* value, const double* start_state,
                              double* return_out, int32_t* length_out, float* final_obs_out, void* stream) {
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (with_value)
        if (int rc = check_plan_value(fn, h, value)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (!actions || !return_out || !length_out) return fail(EMEI_ERR_INVALID, "%s: null argument", fn);
    if (int rc = check_plan_lanes(fn, h, n_candidates)) return rc;
    if (check_action_dtype(h, action_dtype) != EMEI_OK) return EMEI_ERR_INVALID;
    EMEI_ON_DEVICE(h, fn);
    if (!start_state && !h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    LaunchCommon c = plan_call(PLAN_GIVEN, start_state, horizon, n_candidates, discount, value);
    c.plan.return_out = return_out, c.plan.length_out = length_out;
    c.actions = actions, c.obs_out = final_obs_out;
    return launched(fn, launch(h, c, stream, action_dtype));
}
extern "C" EMEI_API int emei_evaluate_sequences(emei_env* h, int32_t horizon, int32_t n_candidates, const void* actions, int action_dtype,
                                                double discount, const double* start_state, double* return_out, int32_t* length_out,
                                                float* final_obs_out, void* stream) {
    return evaluate_sequences("emei_evaluate_sequences", false, h, horizon, n_candidates, actions, action_dtype, discount, nullptr,
                              start_state, return_out, length_out, final_obs_out, stream);
}
extern "C" EMEI_API int emei_evaluate_sequences_value(emei_env* h, int32_t horizon, int32_t n_candidates, const void* actions,
                                                      int action_dtype, double discount, const emei_policy_deep* value,
                                                      const double* start_state, double* return_out, int32_t* length_out,
                                                      float* final_obs_out, void* stream) {
    return evaluate_sequences("emei_evaluate_sequences_value", true, h, horizon, n_candidates, actions, action_dtype, discount, value,
                              start_state, return_out, length_out, final_obs_out, stream);
}

// ---------------------------------------------------------------------------------------------
// emei_plan_shooting / emei_sample_candidates
extern "C" EMEI_API int64_t emei_plan_shooting_workspace_bytes(int64_t n_envs, int32_t n_candidates) {
    const int64_t nk = check_plan_shape("emei_plan_shooting_workspace_bytes", n_envs, n_candidates);
    return nk < 0 ? nk : plan_partials_bytes(n_envs, nk);
}

// the env's ctrlrange from the kernels' own model constants (the Python classes' action_space bounds)
static void ctrl_range(int env_id, float& lo, float& hi) {
    if (is_ip(env_id)) lo = (float)ip_make_model(false).ctrl_lo, hi = (float)ip_make_model(false).ctrl_hi;
    else if (env_id == EMEI_HALFCHEETAH_RUNNING) lo = (float)cheetah::kCtrlLo, hi = (float)cheetah::kCtrlHi;
    else if (env_id == EMEI_HOPPER_RUNNING) lo = (float)hopper::kCtrlLo, hi = (float)hopper::kCtrlHi;
    else if (is_body(env_id)) lo = (float)dpend::kXml.ctrl_lo, hi = (float)dpend::kXml.ctrl_hi;
    else lo = 0.f, hi = 1.f;  // discrete: unused
}

// What the calls that draw candidates refuse alike, from the handle on.  sigma_counts: the call draws around a nominal under the
// scalar `sigma` (which a continuous env then reads).  A call that emits actions checks their dtype next (check_action_dtype).
static int check_candidates(const char* fn, const emei_env* h, int32_t horizon, int32_t n_candidates, bool sigma_counts, double sigma) {
    if (horizon < 1) return fail(EMEI_ERR_INVALID, "%s: horizon=%d < 1", fn, horizon);
    if (n_candidates < 1) return fail(EMEI_ERR_INVALID, "%s: n_candidates=%d < 1", fn, n_candidates);
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (sigma_counts && h->act_dim > 0 && !(std::isfinite(sigma) && sigma > 0.0))
        return fail(EMEI_ERR_INVALID, "%s: sigma=%g with a nominal sequence must be finite and > 0", fn, sigma);
    if (int rc = check_plan_lanes(fn, h, n_candidates)) return rc;
    if ((int64_t)horizon * (h->act_dim > 0 ? h->act_dim : 1) > INT32_MAX)  // 32-bit word index of the candidate's stream
        return fail(EMEI_ERR_INVALID, "%s: horizon * act_dim exceeds 2^31 - 1", fn);
    return EMEI_OK;
}

// the candidate rule of a checked call; `sigma` is read only where check_candidates' sigma_counts held
static CandidateSpec candidate_spec(const emei_env* h, uint64_t seed, const float* nominal, double sigma) {
    CandidateSpec sp{};
    sp.seed = seed, sp.env_offset = h->cfg.env_index_offset, sp.nominal = nominal, sp.sigma = (float)sigma;
    ctrl_range(h->cfg.env_id, sp.lo, sp.hi);
    return sp;
}

extern "C" EMEI_API int emei_sample_candidates(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal,
                                               double sigma, void* actions_out, int action_dtype, void* stream) {
    const char* fn = "emei_sample_candidates";
    if (int rc = check_candidates(fn, h, horizon, n_candidates, nominal != nullptr, sigma)) return rc;
    if (check_action_dtype(h, action_dtype) != EMEI_OK) return EMEI_ERR_INVALID;
    if (!actions_out) return fail(EMEI_ERR_INVALID, "%s: null argument", fn);
    EMEI_ON_DEVICE(h, fn);
    const int rc = launch_sample_candidates(candidate_spec(h, seed, nominal, sigma), h->cfg.n_envs, n_candidates, horizon, h->act_dim,
                                            actions_out, action_dtype, (hipStream_t)stream);
    return launched(fn, rc);
}

// with_value: the value plan kernels keep every return (one instantiation serves the three planners), so the workspace is
// emei_plan_value_workspace_bytes' and the returns lie behind the partials as emei_plan_mppi's do
static int plan_shooting(const char* fn, bool with_value, emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed,
                         const float* nominal, double sigma, double discount, const emei_policy_deep* value, const double* start_state,
                         void* workspace, void* best_action_out, int action_dtype, void* best_sequence_out, double* best_return_out,
                         int32_t* best_index_out, int32_t* best_length_out, void* stream) {
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (with_value)
        if (int rc = check_plan_value(fn, h, value)) return rc;
    if (int rc = check_candidates(fn, h, horizon, n_candidates, nominal != nullptr, sigma)) return rc;
    if (check_action_dtype(h, action_dtype) != EMEI_OK) return EMEI_ERR_INVALID;
    if (!workspace || !best_action_out || !best_return_out || !best_index_out) return fail(EMEI_ERR_INVALID, "%s: null argument", fn);
    EMEI_ON_DEVICE(h, fn);
    if (!start_state && !h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    LaunchCommon c = plan_call(with_value ? PLAN_DRAWN_KEEP : PLAN_DRAWN, start_state, horizon, n_candidates, discount, value);
    PlanLaunch& p = c.plan;
    p.cand = candidate_spec(h, seed, nominal, sigma), p.partials = workspace;
    if (with_value) p.return_out = plan_returns(h, n_candidates, workspace);
    int rc = launch(h, c, stream);
    if (rc == EMEI_OK)
        rc = launch_plan_finish(workspace, p.cand, h->cfg.n_envs, n_candidates, horizon, h->act_dim, best_action_out, action_dtype,
                                best_sequence_out, best_return_out, best_index_out, best_length_out, (hipStream_t)stream);
    return launched(fn, rc);
}
extern "C" EMEI_API int emei_plan_shooting(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal,
                                           double sigma, double discount, const double* start_state, void* workspace,
                                           void* best_action_out, int action_dtype, void* best_sequence_out, double* best_return_out,
                                           int32_t* best_index_out, int32_t* best_length_out, void* stream) {
    return plan_shooting("emei_plan_shooting", false, h, horizon, n_candidates, seed, nominal, sigma, discount, nullptr, start_state,
                         workspace, best_action_out, action_dtype, best_sequence_out, best_return_out, best_index_out, best_length_out,
                         stream);
}
extern "C" EMEI_API int emei_plan_shooting_value(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal,
                                                 double sigma, double discount, const emei_policy_deep* value, const double* start_state,
                                                 void* workspace, void* best_action_out, int action_dtype, void* best_sequence_out,
                                                 double* best_return_out, int32_t* best_index_out, int32_t* best_length_out, void* stream) {
    return plan_shooting("emei_plan_shooting_value", true, h, horizon, n_candidates, seed, nominal, sigma, discount, value, start_state,
                         workspace, best_action_out, action_dtype, best_sequence_out, best_return_out, best_index_out, best_length_out,
                         stream);
}

// ---------------------------------------------------------------------------------------------
// emei_plan_mppi: the plan kernel of emei_plan_shooting with every return kept, then the weighted mean of the redrawn candidates.
// Workspace: emei_plan_shooting's partials (a multiple of 16 bytes), then n_envs * n_candidates float64 returns / weights.
static int64_t keep_workspace_bytes(const char* fn, int64_t n_envs, int32_t n_candidates) {  // also emei_plan_cem's
    const int64_t nk = check_plan_shape(fn, n_envs, n_candidates);
    return nk < 0 ? nk : plan_partials_bytes(n_envs, nk) + (int64_t)sizeof(double) * nk;
}
extern "C" EMEI_API int64_t emei_plan_mppi_workspace_bytes(int64_t n_envs, int32_t n_candidates) {
    return keep_workspace_bytes("emei_plan_mppi_workspace_bytes", n_envs, n_candidates);
}

static int plan_mppi(const char* fn, bool with_value, emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed,
                     const float* nominal, double sigma, double discount, const emei_policy_deep* value, double temperature,
                     const double* start_state, void* workspace, float* nominal_out, double* best_return_out, int32_t* best_index_out,
                     double* ess_out, void* stream) {
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (int rc = check_temperature(fn, temperature)) return rc;
    if (with_value)
        if (int rc = check_plan_value(fn, h, value)) return rc;
    if (int rc = check_candidates(fn, h, horizon, n_candidates, nominal != nullptr, sigma)) return rc;
    if (!workspace) return fail(EMEI_ERR_INVALID, "%s: null workspace", fn);
    if (!nominal_out) return fail(EMEI_ERR_INVALID, "%s: null nominal_out", fn);
    EMEI_ON_DEVICE(h, fn);
    if (!start_state && !h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    LaunchCommon c = plan_call(PLAN_DRAWN_KEEP, start_state, horizon, n_candidates, discount, value);
    PlanLaunch& p = c.plan;
    p.cand = candidate_spec(h, seed, nominal, sigma), p.partials = workspace, p.return_out = plan_returns(h, n_candidates, workspace);
    int rc = launch(h, c, stream);
    if (rc == EMEI_OK)
        rc = launch_plan_mppi_finish(workspace, p.return_out, p.cand, h->cfg.n_envs, n_candidates, horizon, h->act_dim, temperature, nominal_out,
                                     best_return_out, best_index_out, ess_out, (hipStream_t)stream);
    return launched(fn, rc);
}
extern "C" EMEI_API int emei_plan_mppi(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal, double sigma,
                                       double discount, double temperature, const double* start_state, void* workspace,
                                       float* nominal_out, double* best_return_out, int32_t* best_index_out, double* ess_out,
                                       void* stream) {
    return plan_mppi("emei_plan_mppi", false, h, horizon, n_candidates, seed, nominal, sigma, discount, nullptr, temperature, start_state,
                     workspace, nominal_out, best_return_out, best_index_out, ess_out, stream);
}
extern "C" EMEI_API int emei_plan_mppi_value(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal,
                                             double sigma, double discount, const emei_policy_deep* value, double temperature,
                                             const double* start_state, void* workspace, float* nominal_out, double* best_return_out,
                                             int32_t* best_index_out, double* ess_out, void* stream) {
    return plan_mppi("emei_plan_mppi_value", true, h, horizon, n_candidates, seed, nominal, sigma, discount, value, temperature,
                     start_state, workspace, nominal_out, best_return_out, best_index_out, ess_out, stream);
}

// emei_sample_candidates_sigma: emei_sample_candidates' Gaussian mode with the sigma read per entry (there is no scalar to check)
extern "C" EMEI_API int emei_sample_candidates_sigma(emei_env* h, int32_t horizon, int32_t n_candidates, uint64_t seed, const float* nominal,
                                                     const float* sigma_map, void* actions_out, int action_dtype, void* stream) {
    const char* fn = "emei_sample_candidates_sigma";
    if (int rc = check_candidates(fn, h, horizon, n_candidates, false, 0.0)) return rc;
    if (check_action_dtype(h, action_dtype) != EMEI_OK) return EMEI_ERR_INVALID;
    if (h->act_dim == 0) return fail(EMEI_ERR_INVALID, "%s: a discrete env takes no sigma_map", fn);
    if (!nominal || !sigma_map) return fail(EMEI_ERR_INVALID, "%s: null nominal or sigma_map", fn);
    if (!actions_out) return fail(EMEI_ERR_INVALID, "%s: null argument", fn);
    EMEI_ON_DEVICE(h, fn);
    const int rc = launch_sample_candidates_sigma(CandidateSpecMap(candidate_spec(h, seed, nominal, 0.0), sigma_map), h->cfg.n_envs,
                                                  n_candidates, horizon, h->act_dim, actions_out, (hipStream_t)stream);
    return launched(fn, rc);
}

// ---------------------------------------------------------------------------------------------
// emei_plan_cem: emei_plan_mppi's first launch (with a sigma_map: its CandidateSpecMap instantiation), then the elite set and its
// moments.  Workspace: emei_plan_mppi's layout — the selection's counters live in LDS.
extern "C" EMEI_API int64_t emei_plan_cem_workspace_bytes(int64_t n_envs, int32_t n_candidates) {
    return keep_workspace_bytes("emei_plan_cem_workspace_bytes", n_envs, n_candidates);
}

static int plan_cem(const char* fn, bool with_value, emei_env* h, int32_t horizon, int32_t n_candidates, int32_t n_elites, uint64_t seed,
                    const float* nominal, double sigma, const float* sigma_map, double discount, const emei_policy_deep* value,
                    const double* start_state, void* workspace, float* mean_out, float* std_out, double* best_return_out,
                    int32_t* best_index_out, double* elite_return_out, void* stream) {
    // n_elites is refused after horizon and n_candidates, before discount
    if (horizon >= 1 && n_candidates >= 1 && (n_elites < 1 || n_elites > n_candidates))
        return fail(EMEI_ERR_INVALID, "%s: n_elites=%d is outside [1, n_candidates=%d]", fn, n_elites, n_candidates);
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (with_value)
        if (int rc = check_plan_value(fn, h, value)) return rc;
    // with a sigma_map the scalar is ignored
    if (int rc = check_candidates(fn, h, horizon, n_candidates, nominal && !sigma_map, sigma)) return rc;
    if (sigma_map && !nominal) return fail(EMEI_ERR_INVALID, "%s: a sigma_map needs a nominal", fn);
    if (h->act_dim == 0 && (sigma_map || std_out))
        return fail(EMEI_ERR_INVALID, "%s: a discrete env takes no sigma_map and has no std_out", fn);
    if (!workspace) return fail(EMEI_ERR_INVALID, "%s: null workspace", fn);
    if (!mean_out) return fail(EMEI_ERR_INVALID, "%s: null mean_out", fn);
    EMEI_ON_DEVICE(h, fn);
    if (!start_state && !h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    LaunchCommon c = plan_call(PLAN_DRAWN_KEEP, start_state, horizon, n_candidates, discount, value);
    PlanLaunch& p = c.plan;
    p.cand = candidate_spec(h, seed, nominal, sigma), p.sigma_map = sigma_map;
    p.partials = workspace, p.return_out = plan_returns(h, n_candidates, workspace);
    int rc = launch(h, c, stream);
    if (rc == EMEI_OK)
        rc = launch_plan_cem_finish(workspace, p.return_out, p.cand, sigma_map, h->cfg.n_envs, n_candidates, n_elites, horizon, h->act_dim, mean_out,
                                    std_out, best_return_out, best_index_out, elite_return_out, (hipStream_t)stream);
    return launched(fn, rc);
}
extern "C" EMEI_API int emei_plan_cem(emei_env* h, int32_t horizon, int32_t n_candidates, int32_t n_elites, uint64_t seed,
                                      const float* nominal, double sigma, const float* sigma_map, double discount,
                                      const double* start_state, void* workspace, float* mean_out, float* std_out,
                                      double* best_return_out, int32_t* best_index_out, double* elite_return_out, void* stream) {
    return plan_cem("emei_plan_cem", false, h, horizon, n_candidates, n_elites, seed, nominal, sigma, sigma_map, discount, nullptr,
                    start_state, workspace, mean_out, std_out, best_return_out, best_index_out, elite_return_out, stream);
}
extern "C" EMEI_API int emei_plan_cem_value(emei_env* h, int32_t horizon, int32_t n_candidates, int32_t n_elites, uint64_t seed,
                                            const float* nominal, double sigma, const float* sigma_map, double discount,
                                            const emei_policy_deep* value, const double* start_state, void* workspace, float* mean_out,
                                            float* std_out, double* best_return_out, int32_t* best_index_out, double* elite_return_out,
                                            void* stream) {
    return plan_cem("emei_plan_cem_value", true, h, horizon, n_candidates, n_elites, seed, nominal, sigma, sigma_map, discount, value,
                    start_state, workspace, mean_out, std_out, best_return_out, best_index_out, elite_return_out, stream);
}
// one size for the three value planners: the shooting variant keeps every return as well
extern "C" EMEI_API int64_t emei_plan_value_workspace_bytes(int64_t n_envs, int32_t n_candidates) {
    return keep_workspace_bytes("emei_plan_value_workspace_bytes", n_envs, n_candidates);
}

// ---------------------------------------------------------------------------------------------
// The handles the fused controllers refuse (after the state check): the 4-state kernels have pend_mpc_*_kernel, and of the handles
// that step on the body kernels the InvertedDoublePendulum has body_mpc_*_kernel (body_mpc_kernels.h: Body::kFusedMpc), whose plan
// steps the model without observation noise.
static int check_mpc_handle(const char* fn, const emei_env* h) {
    if (steps_as_body(h->cfg)) {
        if (!is_idp(h->cfg.env_id))
            return fail(EMEI_ERR_UNSUPPORTED, "%s: this handle steps on the body kernels (a multi-body env, or an InvertedPendulum with "
                                              "a non-euler integrator or observation noise); the fused controller serves the 4-state kernels only",
                        fn);
        for (int i = 0; i < EMEI_MAX_STATE_DIM; ++i)
            if (h->cfg.obs_sigma[i] != 0.f)
                return fail(EMEI_ERR_UNSUPPORTED, "%s: this InvertedDoublePendulum handle has observation noise (obs_sigma[%d]=%g), which the "
                                                  "fused controller does not serve: its plan steps the model without it",
                            fn, i, (double)h->cfg.obs_sigma[i]);
    }
    if (h->peers.count > 0)
        return fail(EMEI_ERR_UNSUPPORTED, "%s: observation peers are set (emei_set_obs_peers), which this kernel does not serve", fn);
    return EMEI_OK;
}

// The launch of a fused controller (emei_mpc_mppi / emei_mpc_cem / emei_mpc_policy; actions_out in action_dtype), then the done mask
// packed by a small second launch: the kernel leaves env i's last done code in word 0 of its workspace row of n_candidates doubles.
static int launch_controller(const char* fn, emei_env* h, const LaunchCommon& c, int action_dtype, void* stream) {
    int rc = launch(h, c, stream, action_dtype);
    if (rc == EMEI_OK) rc = launch_mpc_done_pack(c.plan.return_out, c.plan.n_candidates, h->cfg.n_envs, h->done_mask, (hipStream_t)stream);
    return launched(fn, rc);
}

// What emei_mpc_mppi and emei_mpc_cem refuse alike about the nominal they keep in LDS ...
static int check_nominal_update(const char* fn, float refill, float nominal_lo, float nominal_hi) {
    if (!std::isfinite(refill)) return fail(EMEI_ERR_INVALID, "%s: refill=%g must be finite", fn, (double)refill);
    if (!(nominal_lo <= nominal_hi))  // also refuses a NaN bound
        return fail(EMEI_ERR_INVALID, "%s: nominal_lo=%g, nominal_hi=%g: need nominal_lo <= nominal_hi", fn, (double)nominal_lo,
                    (double)nominal_hi);
    return EMEI_OK;
}
static int check_mpc_horizon(const char* fn, int32_t horizon, const char* in_lds) {
    if (horizon > EMEI_MPC_MAX_HORIZON)
        return fail(EMEI_ERR_INVALID, "%s: horizon=%d exceeds EMEI_MPC_MAX_HORIZON=%d (%s in LDS)", fn, horizon, EMEI_MPC_MAX_HORIZON, in_lds);
    return EMEI_OK;
}
// ... and everything from the handle on.  They always plan around a nominal, so sigma always counts (the nominal's own NULL check
// comes a few refusals later).
static int check_nominal_controller(const char* fn, emei_env* h, int32_t horizon, int32_t n_candidates, double sigma, int action_dtype,
                                    uint32_t flags, const float* nominal, const void* workspace, const void* actions_out) {
    if (int rc = check_candidates(fn, h, horizon, n_candidates, true, sigma)) return rc;
    if (check_action_dtype(h, action_dtype) != EMEI_OK) return EMEI_ERR_INVALID;
    if (int rc = check_flags(fn, flags)) return rc;
    if (!nominal) return fail(EMEI_ERR_INVALID, "%s: null nominal", fn);
    if (!workspace) return fail(EMEI_ERR_INVALID, "%s: null workspace", fn);
    if (!actions_out) return fail(EMEI_ERR_INVALID, "%s: null actions_out", fn);
    EMEI_ON_DEVICE(h, fn);
    if (!h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    return check_mpc_handle(fn, h);
}
// the fields both give their kernel alike; `c` arrives with the op and the planner's own part of c.mpc
static int launch_nominal_controller(const char* fn, emei_env* h, LaunchCommon& c, int32_t n_steps, int32_t horizon, int32_t n_candidates,
                                     uint64_t seed, float* nominal, double sigma, double discount, float refill, float nominal_lo,
                                     float nominal_hi, void* workspace, void* actions_out, int action_dtype, float* obs_out, float* reward_out,
                                     uint8_t* done_out, double* plan_return_out, uint32_t flags, void* stream) {
    c.n_steps = n_steps, c.flags = flags;
    c.obs_out = obs_out, c.reward_out = reward_out, c.done_out = done_out;
    c.plan.n_candidates = n_candidates, c.plan.discount = discount, c.plan.return_out = (double*)workspace;
    c.plan.cand = candidate_spec(h, seed, nullptr, sigma);  // the kernel keeps the nominal (CEM: the mean and the sigma) in LDS
    c.mpc.horizon = horizon, c.mpc.nominal = nominal, c.mpc.actions_out = actions_out, c.mpc.plan_return_out = plan_return_out;
    c.mpc.refill = refill, c.mpc.nominal_lo = nominal_lo, c.mpc.nominal_hi = nominal_hi;
    return launch_controller(fn, h, c, action_dtype, stream);
}

// ---------------------------------------------------------------------------------------------
// emei_mpc_mppi: n_steps control steps of "emei_plan_mppi, act, emei_step, shift" in one kernel of one wave per env
// (pendulum_kernels.h:pend_mpc_mppi_kernel; the InvertedDoublePendulum: body_mpc_kernels.h:body_mpc_mppi_kernel), then the done mask
// packed by a small second launch.
extern "C" EMEI_API int64_t emei_mpc_mppi_workspace_bytes(int64_t n_envs, int32_t n_candidates) {
    const int64_t nk = check_plan_shape("emei_mpc_mppi_workspace_bytes", n_envs, n_candidates);
    return nk < 0 ? nk : (int64_t)sizeof(double) * nk;  // every candidate's return, then its weight
}

extern "C" EMEI_API int emei_mpc_mppi(emei_env* h, int32_t n_steps, int32_t horizon, int32_t n_candidates, uint64_t seed, float* nominal,
                                      double sigma, double discount, double temperature, float refill, float nominal_lo,
                                      float nominal_hi, void* workspace, void* actions_out, int action_dtype, float* obs_out,
                                      float* reward_out, uint8_t* done_out, double* plan_return_out, double* ess_out, uint32_t flags,
                                      void* stream) {
    const char* fn = "emei_mpc_mppi";
    if (n_steps < 1) return fail(EMEI_ERR_INVALID, "%s: n_steps=%d < 1", fn, n_steps);
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (int rc = check_temperature(fn, temperature)) return rc;
    if (int rc = check_nominal_update(fn, refill, nominal_lo, nominal_hi)) return rc;
    if (int rc = check_mpc_horizon(fn, horizon, "the nominal lives")) return rc;
    if (int rc = check_nominal_controller(fn, h, horizon, n_candidates, sigma, action_dtype, flags, nominal, workspace, actions_out)) return rc;
    LaunchCommon c;
    c.op = OP_MPC_MPPI;
    c.mpc.ess_out = ess_out, c.mpc.temperature = temperature;
    return launch_nominal_controller(fn, h, c, n_steps, horizon, n_candidates, seed, nominal, sigma, discount, refill, nominal_lo, nominal_hi,
                                     workspace, actions_out, action_dtype, obs_out, reward_out, done_out, plan_return_out, flags, stream);
}

// ---------------------------------------------------------------------------------------------
// emei_mpc_cem: n_steps control steps of "`iterations` times emei_plan_cem in place, act, emei_step, shift" in one kernel of one wave
// per env (pendulum_kernels.h:pend_mpc_cem_kernel; the InvertedDoublePendulum: body_mpc_kernels.h:body_mpc_cem_kernel), then
// emei_mpc_mppi's done-mask launch.
extern "C" EMEI_API int64_t emei_mpc_cem_workspace_bytes(int64_t n_envs, int32_t n_candidates) {
    const int64_t nk = check_plan_shape("emei_mpc_cem_workspace_bytes", n_envs, n_candidates);
    return nk < 0 ? nk : (int64_t)sizeof(double) * nk;  // every candidate's return, then its membership flag
}

extern "C" EMEI_API int emei_mpc_cem(emei_env* h, int32_t n_steps, int32_t horizon, int32_t n_candidates, int32_t n_elites,
                                     int32_t iterations, uint64_t seed, float* nominal, double sigma, double sigma_min, double discount,
                                     float refill, float nominal_lo, float nominal_hi, void* workspace, void* actions_out,
                                     int action_dtype, float* obs_out, float* reward_out, uint8_t* done_out, double* plan_return_out,
                                     double* elite_return_out, uint32_t flags, void* stream) {
    const char* fn = "emei_mpc_cem";
    if (n_steps < 1) return fail(EMEI_ERR_INVALID, "%s: n_steps=%d < 1", fn, n_steps);
    // n_elites is refused after horizon and n_candidates, before discount (as emei_plan_cem)
    if (horizon >= 1 && n_candidates >= 1 && (n_elites < 1 || n_elites > n_candidates))
        return fail(EMEI_ERR_INVALID, "%s: n_elites=%d is outside [1, n_candidates=%d]", fn, n_elites, n_candidates);
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (iterations < 1) return fail(EMEI_ERR_INVALID, "%s: iterations=%d < 1", fn, iterations);
    if (int rc = check_nominal_update(fn, refill, nominal_lo, nominal_hi)) return rc;
    if (!(std::isfinite(sigma_min) && sigma_min >= 0.0))
        return fail(EMEI_ERR_INVALID, "%s: sigma_min=%g must be finite and >= 0", fn, sigma_min);
    if (int rc = check_mpc_horizon(fn, horizon, "the mean and the sigma live")) return rc;
    // every control step starts from the scalar sigma
    if (int rc = check_nominal_controller(fn, h, horizon, n_candidates, sigma, action_dtype, flags, nominal, workspace, actions_out)) return rc;
    LaunchCommon c;
    c.op = OP_MPC_CEM;
    c.mpc.elite_return_out = elite_return_out;
    c.mpc.n_elites = n_elites, c.mpc.iterations = iterations, c.mpc.sigma_min = (float)sigma_min;
    return launch_nominal_controller(fn, h, c, n_steps, horizon, n_candidates, seed, nominal, sigma, discount, refill, nominal_lo, nominal_hi,
                                     workspace, actions_out, action_dtype, obs_out, reward_out, done_out, plan_return_out, flags, stream);
}

// ---------------------------------------------------------------------------------------------
// What emei_rollout_policy and emei_evaluate_policies refuse alike about their struct emei_policy argument `arg`: the struct's own
// fields before the handle is looked at, the weight pointers after it.
static int check_policy_struct(const char* fn, const char* arg, const emei_policy* policy) {
    if (!policy) return fail(EMEI_ERR_INVALID, "%s: null %s", fn, arg);
    if (policy->struct_size != sizeof(emei_policy))
        return fail(EMEI_ERR_INVALID, "%s: %s.struct_size=%u != sizeof(emei_policy)=%zu", fn, arg, policy->struct_size, sizeof(emei_policy));
    if (policy->hidden < 0 || policy->hidden > EMEI_POLICY_MAX_HIDDEN)
        return fail(EMEI_ERR_INVALID, "%s: %s.hidden=%d is outside [0, EMEI_POLICY_MAX_HIDDEN=%d]", fn, arg, policy->hidden, EMEI_POLICY_MAX_HIDDEN);
    if (policy->out_mode != EMEI_POLICY_OUT_CLIP && policy->out_mode != EMEI_POLICY_OUT_TANH)
        return fail(EMEI_ERR_INVALID, "%s: unknown %s.out_mode=%d", fn, arg, policy->out_mode);
    if (policy->reserved != 0) return fail(EMEI_ERR_INVALID, "%s: %s.reserved=%d must be 0", fn, arg, policy->reserved);
    return EMEI_OK;
}
static int check_policy_weights(const char* fn, const char* arg, const emei_policy* policy) {
    if (!policy->w2 || !policy->b2) return fail(EMEI_ERR_INVALID, "%s: null %s.%s", fn, arg, !policy->w2 ? "w2" : "b2");
    if (policy->hidden > 0 && (!policy->w1 || !policy->b1))
        return fail(EMEI_ERR_INVALID, "%s: null %s.%s with hidden=%d", fn, arg, !policy->w1 ? "w1" : "b1", policy->hidden);
    return EMEI_OK;
}
// the kernel-argument form of a checked struct emei_policy (the caller adds actions_out / action_dtype where its kernel reads them)
static PolicyArgs policy_args(const emei_env* h, const emei_policy* policy) {
    PolicyArgs pa{};
    pa.w1 = policy->w1, pa.b1 = policy->b1, pa.w2 = policy->w2, pa.b2 = policy->b2;
    pa.hidden = policy->hidden, pa.out_mode = policy->out_mode;
    ctrl_range(h->cfg.env_id, pa.lo, pa.hi);
    return pa;
}

// ---------------------------------------------------------------------------------------------
// What emei_rollout_policy_noisy refuses about its struct emei_policy_noise before the handle is looked at.
static int check_policy_noise(const char* fn, const emei_policy_noise* nz) {
    if (!nz) return fail(EMEI_ERR_INVALID, "%s: null noise", fn);
    if (nz->struct_size != sizeof(emei_policy_noise))
        return fail(EMEI_ERR_INVALID, "%s: noise.struct_size=%u != sizeof(emei_policy_noise)=%zu", fn, nz->struct_size, sizeof(emei_policy_noise));
    if (nz->mode < EMEI_POLICY_NOISE_GAUSS || nz->mode > EMEI_POLICY_NOISE_EPS_GREEDY)
        return fail(EMEI_ERR_INVALID, "%s: unknown noise.mode=%d", fn, nz->mode);
    if (nz->reserved != 0) return fail(EMEI_ERR_INVALID, "%s: noise.reserved=%d must be 0", fn, nz->reserved);
    if (nz->mode == EMEI_POLICY_NOISE_GAUSS && !nz->std && !(std::isfinite(nz->sigma) && nz->sigma >= 0.0))
        return fail(EMEI_ERR_INVALID, "%s: noise.sigma=%g must be finite and >= 0 (noise.std is null)", fn, nz->sigma);
    if (nz->mode == EMEI_POLICY_NOISE_EPS_GREEDY && !(nz->sigma >= 0.0 && nz->sigma <= 1.0))
        return fail(EMEI_ERR_INVALID, "%s: noise.sigma=%g (epsilon) is outside [0, 1]", fn, nz->sigma);
    if (nz->mode == EMEI_POLICY_NOISE_GAUSS_HEAD) {
        if (!(nz->log_std_min <= nz->log_std_max))
            return fail(EMEI_ERR_INVALID, "%s: noise.log_std_min=%g > noise.log_std_max=%g (or a NaN)", fn, (double)nz->log_std_min,
                        (double)nz->log_std_max);
        if (!nz->ws || !nz->bs) return fail(EMEI_ERR_INVALID, "%s: null noise.%s", fn, !nz->ws ? "ws" : "bs");
    }
    return EMEI_OK;
}
// ... and once the handle is known: the noise's kind against the env's
static int check_noise_kind(const char* fn, const emei_env* h, const emei_policy_noise* noise) {
    if ((h->act_dim > 0) == (noise->mode == EMEI_POLICY_NOISE_EPS_GREEDY))
        return fail(EMEI_ERR_INVALID, "%s: noise.mode=%d: the Gaussian modes are for the continuous envs, EMEI_POLICY_NOISE_EPS_GREEDY for "
                                      "the discrete ones", fn, noise->mode);
    return EMEI_OK;
}
// the kernel-argument form of a checked struct emei_policy_noise; null: no noise, all zero
static PolicyNoiseArgs policy_noise_args(const emei_policy_noise* noise) {
    PolicyNoiseArgs na{};
    if (!noise) return na;
    na.seed = noise->seed, na.mode = noise->mode, na.sigma = (float)noise->sigma;
    if (noise->mode == EMEI_POLICY_NOISE_GAUSS) na.std = noise->std;
    if (noise->mode == EMEI_POLICY_NOISE_GAUSS_HEAD)
        na.ws = noise->ws, na.bs = noise->bs, na.log_std_min = noise->log_std_min, na.log_std_max = noise->log_std_max;
    return na;
}

// the dtype of the actions a policy call emits (`out`: the name of its argument)
static int check_policy_action_dtype(const char* fn, const emei_env* h, int action_dtype, const char* out) {
    if (action_dtype < EMEI_ACT_U8 || action_dtype > EMEI_ACT_F32 || (h->act_dim > 0) != (action_dtype == EMEI_ACT_F32))
        return fail(EMEI_ERR_INVALID, "%s: action_dtype=%d: %s is uint8 / int32 / int64 for the discrete envs, float32 for the "
                                      "continuous ones", fn, action_dtype, out);
    return EMEI_OK;
}

// What the three policy rollouts refuse alike once their network's weights are checked (noise null: a deterministic launch) ...
static int check_policy_rollout(const char* fn, emei_env* h, int action_dtype, uint32_t flags, const emei_policy_noise* noise) {
    if (int rc = check_policy_action_dtype(fn, h, action_dtype, "actions_out")) return rc;
    if (int rc = check_flags(fn, flags)) return rc;
    if (noise)
        if (int rc = check_noise_kind(fn, h, noise)) return rc;
    EMEI_ON_DEVICE(h, fn);
    if (!h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    if (h->peers.count > 0)
        return fail(EMEI_ERR_UNSUPPORTED, "%s: observation peers are set (emei_set_obs_peers), which this kernel does not serve", fn);
    return EMEI_OK;
}
// ... and their launch; `c` arrives with the op and the network.  The kernel leaves the done mask itself.
static int launch_policy_rollout(const char* fn, emei_env* h, LaunchCommon& c, int32_t n_steps, const emei_policy_noise* noise, int action_dtype,
                                 float* obs_out, float* reward_out, uint8_t* done_out, uint32_t flags, void* stream) {
    c.n_steps = n_steps, c.flags = flags;
    c.obs_out = obs_out, c.reward_out = reward_out, c.done_out = done_out;
    c.policy_noise = policy_noise_args(noise);
    return launched(fn, launch(h, c, stream, action_dtype));
}

// emei_rollout_policy / emei_rollout_policy_noisy (`noisy`: the latter, with `noise` checked in its place of the header's order):
// n_steps of "observe, evaluate the policy, emei_step" in one launch of the family's policy rollout kernel
// (pendulum_kernels.h:pend_policy_rollout_kernel, body_kernels.h:body_policy_rollout_kernel, or their noisy twins).
static int rollout_policy(const char* fn, bool noisy, emei_env* h, int32_t n_steps, const emei_policy* policy, const emei_policy_noise* noise,
                          void* actions_out, int action_dtype, float* obs_out, float* reward_out, uint8_t* done_out, uint32_t flags,
                          void* stream) {
    if (n_steps < 1) return fail(EMEI_ERR_INVALID, "%s: n_steps=%d < 1", fn, n_steps);
    if (int rc = check_policy_struct(fn, "policy", policy)) return rc;
    if (noisy)
        if (int rc = check_policy_noise(fn, noise)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (int rc = check_policy_weights(fn, "policy", policy)) return rc;
    if (int rc = check_policy_rollout(fn, h, action_dtype, flags, noisy ? noise : nullptr)) return rc;
    LaunchCommon c;
    c.op = noisy ? OP_POLICY_NOISY : OP_POLICY;
    c.policy = policy_args(h, policy);
    c.policy.actions_out = actions_out, c.policy.action_dtype = action_dtype;
    return launch_policy_rollout(fn, h, c, n_steps, noisy ? noise : nullptr, action_dtype, obs_out, reward_out, done_out, flags, stream);
}
extern "C" EMEI_API int emei_rollout_policy(emei_env* h, int32_t n_steps, const emei_policy* policy, void* actions_out, int action_dtype,
                                            float* obs_out, float* reward_out, uint8_t* done_out, uint32_t flags, void* stream) {
    return rollout_policy("emei_rollout_policy", false, h, n_steps, policy, nullptr, actions_out, action_dtype, obs_out, reward_out, done_out,
                          flags, stream);
}
extern "C" EMEI_API int emei_rollout_policy_noisy(emei_env* h, int32_t n_steps, const emei_policy* policy, const emei_policy_noise* noise,
                                                  void* actions_out, int action_dtype, float* obs_out, float* reward_out, uint8_t* done_out,
                                                  uint32_t flags, void* stream) {
    return rollout_policy("emei_rollout_policy_noisy", true, h, n_steps, policy, noise, actions_out, action_dtype, obs_out, reward_out,
                          done_out, flags, stream);
}

// ---------------------------------------------------------------------------------------------
// emei_evaluate_policies: emei_evaluate_sequences' query with the candidates replaced by a population of feedback policies, one
// launch of the family's policy evaluation kernel (pendulum_kernels.h:pend_policy_eval_kernel, body_kernels.h:body_policy_eval_kernel)
// through the plan-launch descriptor; nothing of the handle is written (h->last_kernel included).
// What it and its deep twin refuse alike once the weights are checked: one lane per (policy, env) pair with 32-bit indices, one grid
// dimension of ceil(n_envs / block) blocks per policy ...
static int check_population(const char* fn, emei_env* h, int32_t n_policies, int block, const double* start_state, const double* return_out) {
    if (!return_out) return fail(EMEI_ERR_INVALID, "%s: null return_out", fn);
    const int64_t np = h->cfg.n_envs * (int64_t)n_policies;
    if (np > INT32_MAX) return fail(EMEI_ERR_INVALID, "%s: n_envs * n_policies = %lld exceeds 2^31 - 1", fn, (long long)np);
    const int64_t blocks = (h->cfg.n_envs + block - 1) / block * (int64_t)n_policies;
    if (blocks > INT32_MAX) return fail(EMEI_ERR_INVALID, "%s: n_policies=%d needs %lld blocks, more than 2^31 - 1", fn, n_policies, (long long)blocks);
    EMEI_ON_DEVICE(h, fn);
    if (!start_state && !h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    return EMEI_OK;
}
// ... and their launch; `c` arrives with the op and the stacked networks
static int launch_population(const char* fn, emei_env* h, LaunchCommon& c, int32_t horizon, int32_t n_policies, double discount,
                             const double* start_state, double* return_out, int32_t* length_out, float* final_obs_out, void* stream) {
    c.plan.mode = PLAN_GIVEN, c.plan.start_rows = start_state, c.plan.n_candidates = n_policies, c.plan.discount = discount;
    c.plan.return_out = return_out, c.plan.length_out = length_out;
    c.n_steps = horizon, c.obs_out = final_obs_out;
    return launched(fn, launch(h, c, stream));
}

extern "C" EMEI_API int emei_evaluate_policies(emei_env* h, int32_t horizon, int32_t n_policies, const emei_policy* stacked, double discount,
                                               const double* start_state, double* return_out, int32_t* length_out, float* final_obs_out,
                                               void* stream) {
    const char* fn = "emei_evaluate_policies";
    if (int rc = check_plan_scalars(fn, horizon, n_policies, discount, "n_policies")) return rc;
    if (int rc = check_policy_struct(fn, "stacked", stacked)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (int rc = check_policy_weights(fn, "stacked", stacked)) return rc;
    if (int rc = check_population(fn, h, n_policies, kBlock, start_state, return_out)) return rc;
    LaunchCommon c;
    c.op = OP_POLICY_EVAL, c.policy = policy_args(h, stacked);
    return launch_population(fn, h, c, horizon, n_policies, discount, start_state, return_out, length_out, final_obs_out, stream);
}

// ---------------------------------------------------------------------------------------------
// emei_plan_policy: shooting and MPPI over closed-loop rollouts of one feedback policy under exploration noise.  First launch: the
// family's policy plan kernel (pendulum_kernels.h:pend_policy_plan_kernel, body_kernels.h:body_policy_plan_kernel) through the
// plan-launch descriptor, as PLAN_DRAWN_KEEP with the policy in the place of the draws; second launch: plan_policy_finish_kernel.
// Workspace: emei_plan_shooting's partials (a multiple of 16 bytes), then n_envs * n_candidates float64 returns (unused when the
// caller gives return_out: the kernel then writes there), then kPlanPolicyMaxAct float32 slots per candidate, of which the actions of
// step 0 take [n_envs * n_candidates, act_dim].  Nothing of the handle is written (h->last_kernel included).
extern "C" EMEI_API int64_t emei_plan_policy_workspace_bytes(int64_t n_envs, int32_t n_candidates) {
    const int64_t nk = check_plan_shape("emei_plan_policy_workspace_bytes", n_envs, n_candidates);
    return nk < 0 ? nk : plan_partials_bytes(n_envs, nk) + (int64_t)(sizeof(double) + kPlanPolicyMaxAct * sizeof(float)) * nk;
}
struct PlanPolicyWorkspace {
    void* partials;
    double* returns;
    float* first_actions;
};
static PlanPolicyWorkspace plan_policy_workspace(const emei_env* h, int32_t n_candidates, void* workspace) {
    double* returns = plan_returns(h, n_candidates, workspace);
    return {workspace, returns, (float*)(returns + h->cfg.n_envs * (int64_t)n_candidates)};
}

// What emei_plan_policy and its deep twin refuse alike once the weights are checked ...
static int check_plan_policy(const char* fn, emei_env* h, int32_t n_candidates, int action_dtype, const void* workspace,
                             const void* best_action_out, const emei_policy_noise* noise, const double* start_state) {
    if (int rc = check_plan_lanes(fn, h, n_candidates)) return rc;
    if (int rc = check_policy_action_dtype(fn, h, action_dtype, "best_action_out")) return rc;
    if (!workspace) return fail(EMEI_ERR_INVALID, "%s: null workspace", fn);
    if (!best_action_out) return fail(EMEI_ERR_INVALID, "%s: null best_action_out", fn);
    if (int rc = check_noise_kind(fn, h, noise)) return rc;
    EMEI_ON_DEVICE(h, fn);
    if (!start_state && !h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    return EMEI_OK;
}
// ... and their two launches; `c` arrives with the op and the networks
static int launch_plan_policy(const char* fn, emei_env* h, LaunchCommon& c, int32_t horizon, int32_t n_candidates,
                              const emei_policy_noise* noise, double discount, double temperature, const double* start_state, void* workspace,
                              void* best_action_out, int action_dtype, float* mean_action_out, double* best_return_out,
                              int32_t* best_index_out, int32_t* best_length_out, double* return_out, double* ess_out, void* stream) {
    const PlanPolicyWorkspace ws = plan_policy_workspace(h, n_candidates, workspace);
    PlanLaunch& p = c.plan;
    p.mode = PLAN_DRAWN_KEEP, p.start_rows = start_state, p.n_candidates = n_candidates, p.discount = discount;
    p.partials = ws.partials, p.return_out = return_out ? return_out : ws.returns, p.first_actions = ws.first_actions;
    c.policy_noise = policy_noise_args(noise);
    c.n_steps = horizon;
    int rc = launch(h, c, stream);
    if (rc == EMEI_OK)
        rc = launch_plan_policy_finish(ws.partials, p.return_out, p.first_actions, h->cfg.n_envs, n_candidates, h->act_dim, temperature,
                                       best_action_out, action_dtype, mean_action_out, best_return_out, best_index_out, best_length_out,
                                       ess_out, (hipStream_t)stream);
    return launched(fn, rc);
}

extern "C" EMEI_API int emei_plan_policy(emei_env* h, int32_t horizon, int32_t n_candidates, const emei_policy* policy,
                                         const emei_policy_noise* noise, double discount, double temperature, const double* start_state,
                                         void* workspace, void* best_action_out, int action_dtype, float* mean_action_out,
                                         double* best_return_out, int32_t* best_index_out, int32_t* best_length_out, double* return_out,
                                         double* ess_out, void* stream) {
    const char* fn = "emei_plan_policy";
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (mean_action_out || ess_out)
        if (int rc = check_temperature(fn, temperature)) return rc;
    if (int rc = check_policy_struct(fn, "policy", policy)) return rc;
    if (int rc = check_policy_noise(fn, noise)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (int rc = check_policy_weights(fn, "policy", policy)) return rc;
    if (int rc = check_plan_policy(fn, h, n_candidates, action_dtype, workspace, best_action_out, noise, start_state)) return rc;
    LaunchCommon c;
    c.op = OP_POLICY_PLAN;
    c.policy = policy_args(h, policy);
    c.policy.action_dtype = action_dtype;
    return launch_plan_policy(fn, h, c, horizon, n_candidates, noise, discount, temperature, start_state, workspace, best_action_out,
                              action_dtype, mean_action_out, best_return_out, best_index_out, best_length_out, return_out, ess_out, stream);
}

// ---------------------------------------------------------------------------------------------
// emei_mpc_policy: n_steps control steps of "emei_plan_policy under the key seed + t * seed_stride, act, emei_step" in one kernel of one
// wave per env (pendulum_kernels.h:pend_mpc_policy_kernel; the InvertedDoublePendulum: body_mpc_kernels.h:body_mpc_policy_kernel), then
// emei_mpc_mppi's done-mask launch.  Workspace: every candidate's float64 return, [n_envs, n_candidates] — word 0 of env i's row is
// where the kernel leaves the env's last done code — then one float32 first-action slot per candidate.
extern "C" EMEI_API int64_t emei_mpc_policy_workspace_bytes(int64_t n_envs, int32_t n_candidates) {
    const int64_t nk = check_plan_shape("emei_mpc_policy_workspace_bytes", n_envs, n_candidates);
    return nk < 0 ? nk : ((int64_t)(sizeof(double) + sizeof(float)) * nk + 7) / 8 * 8;
}

extern "C" EMEI_API int emei_mpc_policy(emei_env* h, int32_t n_steps, int32_t horizon, int32_t n_candidates, const emei_policy* policy,
                                        const emei_policy_noise* noise, uint64_t seed_stride, int32_t act_mode, double discount,
                                        double temperature, void* workspace, void* actions_out, int action_dtype, float* obs_out,
                                        float* reward_out, uint8_t* done_out, double* plan_return_out, int32_t* plan_index_out,
                                        double* ess_out, uint32_t flags, void* stream) {
    const char* fn = "emei_mpc_policy";
    if (n_steps < 1) return fail(EMEI_ERR_INVALID, "%s: n_steps=%d < 1", fn, n_steps);
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (act_mode != EMEI_MPC_POLICY_ACT_BEST && act_mode != EMEI_MPC_POLICY_ACT_MEAN)
        return fail(EMEI_ERR_INVALID, "%s: unknown act_mode=%d", fn, act_mode);
    const bool weighted = act_mode == EMEI_MPC_POLICY_ACT_MEAN || ess_out;
    if (weighted)
        if (int rc = check_temperature(fn, temperature)) return rc;
    if (int rc = check_policy_struct(fn, "policy", policy)) return rc;
    if (int rc = check_policy_noise(fn, noise)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (int rc = check_policy_weights(fn, "policy", policy)) return rc;
    if (int rc = check_plan_lanes(fn, h, n_candidates)) return rc;
    if (int rc = check_policy_action_dtype(fn, h, action_dtype, "actions_out")) return rc;
    if (int rc = check_flags(fn, flags)) return rc;
    if (!workspace) return fail(EMEI_ERR_INVALID, "%s: null workspace", fn);
    if (!actions_out) return fail(EMEI_ERR_INVALID, "%s: null actions_out", fn);
    if (int rc = check_noise_kind(fn, h, noise)) return rc;
    EMEI_ON_DEVICE(h, fn);
    if (!h->has_state) return fail(EMEI_ERR_STATE, "%s: call reset before using the state", fn);
    if (int rc = check_mpc_handle(fn, h)) return rc;
    LaunchCommon c;
    c.op = OP_MPC_POLICY;
    c.n_steps = n_steps, c.flags = flags;
    c.obs_out = obs_out, c.reward_out = reward_out, c.done_out = done_out;
    c.plan.n_candidates = n_candidates, c.plan.discount = discount, c.plan.return_out = (double*)workspace;
    c.mpc.horizon = horizon, c.mpc.actions_out = actions_out;
    c.mpc.plan_return_out = plan_return_out, c.mpc.plan_index_out = plan_index_out, c.mpc.ess_out = ess_out;
    c.mpc.temperature = weighted ? temperature : 1.0, c.mpc.act_mode = act_mode, c.mpc.seed_stride = seed_stride;
    c.policy = policy_args(h, policy);
    c.policy.action_dtype = action_dtype;
    c.policy_noise = policy_noise_args(noise);
    return launch_controller(fn, h, c, action_dtype, stream);
}

// ---------------------------------------------------------------------------------------------
// emei_rollout_policy_deep / emei_evaluate_policies_deep / emei_plan_policy_deep: the policy calls above for struct emei_policy_deep
// (two hidden layers), on kernels of their own (pend_policy_*_deep_kernel / body_policy_*_deep_kernel).  The refusals mirror
// check_policy_struct / check_policy_weights.
// with_out_mode false: the terminal value network of emei_plan_policy_deep, whose out_mode is ignored
static int check_policy_deep_struct(const char* fn, const char* arg, const emei_policy_deep* policy, bool with_out_mode) {
    if (!policy) return fail(EMEI_ERR_INVALID, "%s: null %s", fn, arg);
    if (policy->struct_size != sizeof(emei_policy_deep))
        return fail(EMEI_ERR_INVALID, "%s: %s.struct_size=%u != sizeof(emei_policy_deep)=%zu", fn, arg, policy->struct_size,
                    sizeof(emei_policy_deep));
    if (policy->hidden1 < 1 || policy->hidden1 > EMEI_POLICY_DEEP_MAX_HIDDEN)
        return fail(EMEI_ERR_INVALID, "%s: %s.hidden1=%d is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=%d]", fn, arg, policy->hidden1,
                    EMEI_POLICY_DEEP_MAX_HIDDEN);
    if (policy->hidden2 < 1 || policy->hidden2 > EMEI_POLICY_DEEP_MAX_HIDDEN)
        return fail(EMEI_ERR_INVALID, "%s: %s.hidden2=%d is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=%d]", fn, arg, policy->hidden2,
                    EMEI_POLICY_DEEP_MAX_HIDDEN);
    if (with_out_mode && policy->out_mode != EMEI_POLICY_OUT_CLIP && policy->out_mode != EMEI_POLICY_OUT_TANH)
        return fail(EMEI_ERR_INVALID, "%s: unknown %s.out_mode=%d", fn, arg, policy->out_mode);
    if (policy->reserved != 0) return fail(EMEI_ERR_INVALID, "%s: %s.reserved=%lld must be 0", fn, arg, (long long)policy->reserved);
    return EMEI_OK;
}
static int check_policy_deep_weights(const char* fn, const char* arg, const emei_policy_deep* policy) {
    const float* const ptr[6] = {policy->w1, policy->b1, policy->w2, policy->b2, policy->w3, policy->b3};
    static const char* const name[6] = {"w1", "b1", "w2", "b2", "w3", "b3"};
    for (int k = 0; k < 6; ++k)
        if (!ptr[k]) return fail(EMEI_ERR_INVALID, "%s: null %s.%s", fn, arg, name[k]);
    return EMEI_OK;
}
// the kernel-argument form of a checked struct emei_policy_deep (noisy = 0; the caller adds what its kernel reads beyond the network)
static PolicyDeepArgs policy_deep_args(const emei_env* h, const emei_policy_deep* policy) {
    PolicyDeepArgs pa{};
    pa.w1 = policy->w1, pa.b1 = policy->b1, pa.w2 = policy->w2, pa.b2 = policy->b2, pa.w3 = policy->w3, pa.b3 = policy->b3;
    pa.hidden1 = policy->hidden1, pa.hidden2 = policy->hidden2, pa.out_mode = policy->out_mode;
    ctrl_range(h->cfg.env_id, pa.lo, pa.hi);
    return pa;
}
// ... and of the terminal value network: the weights and the widths alone; null: w1 null, no terminal value
static PolicyDeepArgs policy_value_args(const emei_policy_deep* value) {
    PolicyDeepArgs va{};
    if (!value) return va;
    va.w1 = value->w1, va.b1 = value->b1, va.w2 = value->w2, va.b2 = value->b2, va.w3 = value->w3, va.b3 = value->b3;
    va.hidden1 = value->hidden1, va.hidden2 = value->hidden2;
    return va;
}

extern "C" EMEI_API int emei_rollout_policy_deep(emei_env* h, int32_t n_steps, const emei_policy_deep* policy, const emei_policy_noise* noise,
                                                 void* actions_out, int action_dtype, float* obs_out, float* reward_out, uint8_t* done_out,
                                                 uint32_t flags, void* stream) {
    const char* fn = "emei_rollout_policy_deep";
    if (n_steps < 1) return fail(EMEI_ERR_INVALID, "%s: n_steps=%d < 1", fn, n_steps);
    if (int rc = check_policy_deep_struct(fn, "policy", policy)) return rc;
    if (noise)
        if (int rc = check_policy_noise(fn, noise)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (int rc = check_policy_deep_weights(fn, "policy", policy)) return rc;
    if (int rc = check_policy_rollout(fn, h, action_dtype, flags, noise)) return rc;
    LaunchCommon c;
    c.op = OP_POLICY_DEEP;
    c.policy_deep = policy_deep_args(h, policy);
    c.policy_deep.actions_out = actions_out, c.policy_deep.action_dtype = action_dtype, c.policy_deep.noisy = noise ? 1 : 0;
    return launch_policy_rollout(fn, h, c, n_steps, noise, action_dtype, obs_out, reward_out, done_out, flags, stream);
}

extern "C" EMEI_API int emei_evaluate_policies_deep(emei_env* h, int32_t horizon, int32_t n_policies, const emei_policy_deep* stacked,
                                                    double discount, const double* start_state, double* return_out, int32_t* length_out,
                                                    float* final_obs_out, void* stream) {
    const char* fn = "emei_evaluate_policies_deep";
    if (int rc = check_plan_scalars(fn, horizon, n_policies, discount, "n_policies")) return rc;
    if (int rc = check_policy_deep_struct(fn, "stacked", stacked)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (int rc = check_policy_deep_weights(fn, "stacked", stacked)) return rc;
    if (int rc = check_population(fn, h, n_policies, kWave, start_state, return_out)) return rc;  // one-wave blocks
    LaunchCommon c;
    c.op = OP_POLICY_EVAL_DEEP, c.policy_deep = policy_deep_args(h, stacked);  // noisy = 0: scored without exploration noise
    return launch_population(fn, h, c, horizon, n_policies, discount, start_state, return_out, length_out, final_obs_out, stream);
}

// emei_plan_policy_deep: emei_plan_policy for struct emei_policy_deep, with an optional terminal value network.  First launch: the
// family's deep policy plan kernel (pendulum_kernels.h:pend_policy_plan_deep_kernel, body_kernels.h:body_policy_plan_deep_kernel),
// one-wave blocks over the same lanes j = i * n_candidates + k; second launch: plan_policy_finish_kernel, as it is.  The workspace
// is emei_plan_policy's, laid out as there.  Nothing of the handle is written (h->last_kernel included).
extern "C" EMEI_API int emei_plan_policy_deep(emei_env* h, int32_t horizon, int32_t n_candidates, const emei_policy_deep* policy,
                                              const emei_policy_noise* noise, const emei_policy_deep* value, double discount,
                                              double temperature, const double* start_state, void* workspace, void* best_action_out,
                                              int action_dtype, float* mean_action_out, double* best_return_out, int32_t* best_index_out,
                                              int32_t* best_length_out, double* return_out, double* ess_out, void* stream) {
    const char* fn = "emei_plan_policy_deep";
    if (int rc = check_plan_scalars(fn, horizon, n_candidates, discount)) return rc;
    if (mean_action_out || ess_out)
        if (int rc = check_temperature(fn, temperature)) return rc;
    if (int rc = check_policy_deep_struct(fn, "policy", policy)) return rc;
    if (int rc = check_policy_noise(fn, noise)) return rc;
    if (value)
        if (int rc = check_policy_deep_struct(fn, "value", value, false)) return rc;
    if (!h) return fail(EMEI_ERR_INVALID, "%s: null handle", fn);
    if (int rc = check_policy_deep_weights(fn, "policy", policy)) return rc;
    if (value)
        if (int rc = check_policy_deep_weights(fn, "value", value)) return rc;
    if (int rc = check_plan_policy(fn, h, n_candidates, action_dtype, workspace, best_action_out, noise, start_state)) return rc;
    LaunchCommon c;
    c.op = OP_POLICY_PLAN_DEEP;
    c.policy_deep = policy_deep_args(h, policy);
    c.policy_deep.action_dtype = action_dtype, c.policy_deep.noisy = 1;
    c.policy_value = policy_value_args(value);
    return launch_plan_policy(fn, h, c, horizon, n_candidates, noise, discount, temperature, start_state, workspace, best_action_out,
                              action_dtype, mean_action_out, best_return_out, best_index_out, best_length_out, return_out, ess_out, stream);
}

extern "C" EMEI_API int emei_compact_done(emei_env* h, int32_t* idx_out, int32_t* count_out, void* stream) {
    if (!h || !idx_out || !count_out) return fail(EMEI_ERR_INVALID, "emei_compact_done: null argument");
    EMEI_ON_DEVICE(h, "emei_compact_done");
    int rc = launch_compact_done(h->done_mask, h->cfg.n_envs, idx_out, count_out, (hipStream_t)stream);
    return rc == EMEI_OK ? rc : fail(rc, "emei_compact_done: launch failed");
}

extern "C" EMEI_API int emei_get_counters(emei_env* h, int32_t* steps_out, uint32_t* episode_out, void* stream) {
    if (!h) return fail(EMEI_ERR_INVALID, "emei_get_counters: null handle");
    EMEI_ON_DEVICE(h, "emei_get_counters");
    const size_t n = (size_t)h->cfg.n_envs;
    hipStream_t s = (hipStream_t)stream;
    if (steps_out) HIP_TRY(hipMemcpyAsync(steps_out, h->steps, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (episode_out) HIP_TRY(hipMemcpyAsync(episode_out, h->episode, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return EMEI_OK;
}

extern "C" EMEI_API int emei_episode_init_obs(emei_env* h, int64_t count, const int64_t* env_index, const uint32_t* episode,
                                              float* obs_out, void* stream) {
    if (!h || !env_index || !episode || !obs_out) return fail(EMEI_ERR_INVALID, "emei_episode_init_obs: null argument");
    EMEI_ON_DEVICE(h, "emei_episode_init_obs");
    if (count <= 0) return fail(EMEI_ERR_INVALID, "emei_episode_init_obs: count=%lld", (long long)count);
    LaunchCommon c;
    c.op = OP_INIT_OBS;
    c.n = count;
    c.env_index = env_index;
    c.episode_in = episode;
    c.obs_out = obs_out;
    const int rc = launch(h, c, stream);
    return rc == EMEI_OK ? rc : fail(rc, "emei_episode_init_obs: launch failed");
}

// ---------------------------------------------------------------------------------------------
static int fill_env_params(int env_id, uint32_t mask, const double* params, EnvParams& ep, const char* fn) {
    if (mask == 0) return EMEI_OK;
    if (!params || (mask >> EMEI_MAX_ENV_PARAMS)) return fail(EMEI_ERR_INVALID, "%s: bad env_param_mask 0x%x / params", fn, mask);
    if (env_id != EMEI_HALFCHEETAH_RUNNING && env_id != EMEI_HOPPER_RUNNING)
        return fail(EMEI_ERR_UNSUPPORTED, "%s: env_id %d takes no reward / health parameters", fn, env_id);
    ep.mask = mask;
    memcpy(ep.v, params, sizeof(ep.v));
    return EMEI_OK;
}

static bool bad_io(int io_dtype) { return io_dtype != EMEI_IO_F32 && io_dtype != EMEI_IO_F64; }
static bool misaligned16(const void* p) { return ((uintptr_t)p & 15u) != 0; }
// the descriptor of a 4-state kernel launched without a handle, on the caller's current device: rows `obs` of io_dtype
static PendLaunch pend_stateless(int op, int env_id, int precision, int64_t n, int io_dtype, const void* obs, double dt, void* stream) {
    PendLaunch L;
    L.op = op;
    L.env_id = env_id;
    L.precision = precision;
    L.obs_in = obs;
    L.io_f64 = io_dtype == EMEI_IO_F64;
    L.n = n;
    L.p = pend_params(env_id, dt);
    L.trig = current_device_trig();
    L.stream = (hipStream_t)stream;
    return L;
}

extern "C" EMEI_API int emei_reward_io(int env_id, int64_t n, int io_dtype, const void* obs, const void* pre_obs, const void* action,
                              double real_time_scale, int32_t freq_rate, uint32_t env_param_mask, const double* env_params,
                              uint32_t flags, void* reward_out, void* stream) {
    if (n <= 0 || !obs || !reward_out) return fail(EMEI_ERR_INVALID, "emei_reward: bad argument");
    if (bad_io(io_dtype)) return fail(EMEI_ERR_INVALID, "emei_reward: io_dtype=%d", io_dtype);
    if (flags & ~EMEI_REWARD_BATCH_CTRL_COST) return fail(EMEI_ERR_INVALID, "emei_reward: unknown flags 0x%x", flags);
    if ((flags & EMEI_REWARD_BATCH_CTRL_COST) && env_id != EMEI_HALFCHEETAH_RUNNING && env_id != EMEI_HOPPER_RUNNING)
        return fail(EMEI_ERR_UNSUPPORTED, "emei_reward: env_id %d has no control-cost term to sum over the batch", env_id);
    if (is_pend(env_id)) {
        if (misaligned16(obs)) return fail(EMEI_ERR_INVALID, "emei_reward: obs must be 16-byte aligned");
        // evaluated in float64 whatever the row dtype
        PendLaunch L = pend_stateless(OP_REWARD_TERMINAL, env_id, EMEI_PRECISION_REF, n, io_dtype, obs, real_time_scale > 0 ? real_time_scale : 0.02, stream);
        L.reward_out = (float*)reward_out;
        int rc = pend_launch(L);
        return rc == EMEI_OK ? rc : fail(rc, "emei_reward: launch failed");
    }
    if (is_body(env_id)) {
        if ((env_id == EMEI_HALFCHEETAH_RUNNING || env_id == EMEI_HOPPER_RUNNING) && (!pre_obs || !action))
            return fail(EMEI_ERR_INVALID, "emei_reward: this env's reward needs pre_obs and action");
        if (!(real_time_scale > 0) || freq_rate < 1) return fail(EMEI_ERR_INVALID, "emei_reward: bad dt/freq_rate");
        BodyLaunch L;
        if (int rc_ = fill_env_params(env_id, env_param_mask, env_params, L.env_params, "emei_reward")) return rc_;
        L.op = OP_REWARD;
        L.env_id = env_id;
        L.precision = EMEI_PRECISION_REF;
        L.obs_in = obs, L.pre_obs_in = pre_obs, L.actions = action;
        L.io_f64 = io_dtype == EMEI_IO_F64;
        L.reward_out = (float*)reward_out;
        L.n = n;
        L.freq_rate = freq_rate;
        L.dt = real_time_scale;
        L.stream = (hipStream_t)stream;
        if (flags & EMEI_REWARD_BATCH_CTRL_COST)  // 8 B for the whole-batch sum, allocated and freed in stream order
            HIP_TRY(hipMallocAsync((void**)&L.batch_cost_scratch, sizeof(double), L.stream));
        int rc = body_launch(L);
        if (L.batch_cost_scratch) (void)hipFreeAsync(L.batch_cost_scratch, L.stream);
        return rc == EMEI_OK ? rc : fail(rc, "emei_reward: launch failed");
    }
    return fail(EMEI_ERR_INVALID, "emei_reward: unknown env_id %d", env_id);
}

extern "C" EMEI_API int emei_reward_ex(int env_id, int64_t n, const float* obs, const float* pre_obs, const float* action,
                              double real_time_scale, int32_t freq_rate, uint32_t env_param_mask, const double* env_params,
                              float* reward_out, void* stream) {
    return emei_reward_io(env_id, n, EMEI_IO_F32, obs, pre_obs, action, real_time_scale, freq_rate, env_param_mask, env_params, 0u,
                          reward_out, stream);
}

extern "C" EMEI_API int emei_reward(int env_id, int64_t n, const float* obs, const float* pre_obs, const float* action,
                           double real_time_scale, int32_t freq_rate, float* reward_out, void* stream) {
    return emei_reward_io(env_id, n, EMEI_IO_F32, obs, pre_obs, action, real_time_scale, freq_rate, 0u, nullptr, 0u, reward_out, stream);
}

extern "C" EMEI_API int emei_terminal_io(int env_id, int64_t n, int io_dtype, const void* obs, uint32_t env_param_mask,
                                const double* env_params, uint8_t* terminal_out, void* stream) {
    if (n <= 0 || !obs || !terminal_out) return fail(EMEI_ERR_INVALID, "emei_terminal: bad argument");
    if (bad_io(io_dtype)) return fail(EMEI_ERR_INVALID, "emei_terminal: io_dtype=%d", io_dtype);
    if (is_pend(env_id)) {
        if (misaligned16(obs)) return fail(EMEI_ERR_INVALID, "emei_terminal: obs must be 16-byte aligned");
        PendLaunch L = pend_stateless(OP_REWARD_TERMINAL, env_id, EMEI_PRECISION_REF, n, io_dtype, obs, 0.02, stream);
        L.done_out = terminal_out;
        int rc = pend_launch(L);
        return rc == EMEI_OK ? rc : fail(rc, "emei_terminal: launch failed");
    }
    if (is_body(env_id)) {
        BodyLaunch L;
        if (int rc_ = fill_env_params(env_id, env_param_mask, env_params, L.env_params, "emei_terminal")) return rc_;
        L.op = OP_TERMINAL;
        L.env_id = env_id;
        L.precision = EMEI_PRECISION_REF;
        L.obs_in = obs;
        L.io_f64 = io_dtype == EMEI_IO_F64;
        L.done_out = terminal_out;
        L.n = n;
        L.stream = (hipStream_t)stream;
        int rc = body_launch(L);
        return rc == EMEI_OK ? rc : fail(rc, "emei_terminal: launch failed");
    }
    return fail(EMEI_ERR_INVALID, "emei_terminal: unknown env_id %d", env_id);
}

extern "C" EMEI_API int emei_terminal_ex(int env_id, int64_t n, const float* obs, uint32_t env_param_mask,
                                const double* env_params, uint8_t* terminal_out, void* stream) {
    return emei_terminal_io(env_id, n, EMEI_IO_F32, obs, env_param_mask, env_params, terminal_out, stream);
}

extern "C" EMEI_API int emei_terminal(int env_id, int64_t n, const float* obs, uint8_t* terminal_out, void* stream) {
    return emei_terminal_io(env_id, n, EMEI_IO_F32, obs, 0u, nullptr, terminal_out, stream);
}

extern "C" EMEI_API int emei_next_obs_io(int env_id, int64_t n, int io_dtype, const void* obs, const void* actions, int action_dtype,
                                double real_time_scale, int32_t freq_rate, int32_t precision, int32_t integrator,
                                void* next_obs_out, void* stream) {
    if (n <= 0 || !obs || !actions || !next_obs_out) return fail(EMEI_ERR_INVALID, "emei_next_obs: bad argument");
    if (bad_io(io_dtype)) return fail(EMEI_ERR_INVALID, "emei_next_obs: io_dtype=%d", io_dtype);
    if (!(real_time_scale > 0) || freq_rate < 1) return fail(EMEI_ERR_INVALID, "emei_next_obs: bad dt/freq_rate");
    if (action_dtype < EMEI_ACT_U8 || action_dtype > EMEI_ACT_F32) return fail(EMEI_ERR_INVALID, "bad action_dtype");
    if (precision != EMEI_PRECISION_REF && precision != EMEI_PRECISION_F32) return fail(EMEI_ERR_INVALID, "emei_next_obs: precision=%d", precision);
    const int ode_method = (integrator & EMEI_NEXT_OBS_ODE_RK4) ? EMEI_ODE_RK4 : EMEI_ODE_EULER;  // classic control only
    integrator &= ~EMEI_NEXT_OBS_ODE_RK4;
    if (integrator < EMEI_INTEG_EULER || integrator > EMEI_INTEG_RK4)
        return fail(EMEI_ERR_UNSUPPORTED, "emei_next_obs: integrator=%d", integrator);
    int od, ad, sd;
    if (emei_env_dims(env_id, &od, &ad, &sd) != EMEI_OK) return EMEI_ERR_INVALID;
    const bool ip_as_body = is_ip(env_id) && integrator != EMEI_INTEG_EULER;
    if (is_pend(env_id) && !ip_as_body) {
        if (misaligned16(obs) || misaligned16(next_obs_out)) return fail(EMEI_ERR_INVALID, "emei_next_obs: obs / next_obs_out must be 16-byte aligned");
        PendLaunch L = pend_stateless(OP_NEXT_OBS, env_id, precision, n, io_dtype, obs, real_time_scale, stream);
        L.ode_method = ode_method;
        L.actions = actions;
        L.action_dtype = action_dtype;
        L.obs_out = (float*)next_obs_out;
        L.freq_rate = freq_rate;
        int rc = pend_launch(L);
        return rc == EMEI_OK ? rc : fail(rc, "emei_next_obs: launch failed");
    }
    if (action_dtype != EMEI_ACT_F32) return fail(EMEI_ERR_INVALID, "continuous-action envs take float32 actions [n,%d]", ad);
    BodyLaunch L;
    L.op = OP_NEXT_OBS;
    L.env_id = env_id;
    L.precision = precision;
    L.obs_in = obs;
    L.io_f64 = io_dtype == EMEI_IO_F64;
    L.actions = actions;
    L.obs_out = (float*)next_obs_out;
    L.n = n;
    L.freq_rate = freq_rate;
    L.dt = real_time_scale;
    L.integrator = integrator;
    L.trig = current_device_trig();
    L.stream = (hipStream_t)stream;
    int rc = body_launch(L);
    if (rc == EMEI_ERR_UNSUPPORTED)
        return fail(rc, "emei_next_obs: the observation of env_id %d does not determine its state", env_id);  // core.py:190-193
    return rc == EMEI_OK ? rc : fail(rc, "emei_next_obs: launch failed");
}

extern "C" EMEI_API int emei_next_obs_ex(int env_id, int64_t n, const float* obs, const void* actions, int action_dtype,
                                double real_time_scale, int32_t freq_rate, int32_t precision, int32_t integrator,
                                float* next_obs_out, void* stream) {
    return emei_next_obs_io(env_id, n, EMEI_IO_F32, obs, actions, action_dtype, real_time_scale, freq_rate, precision, integrator,
                            next_obs_out, stream);
}

extern "C" EMEI_API int emei_next_obs(int env_id, int64_t n, const float* obs, const void* actions, int action_dtype,
                             double real_time_scale, int32_t freq_rate, int32_t precision, float* next_obs_out,
                             void* stream) {
    return emei_next_obs_io(env_id, n, EMEI_IO_F32, obs, actions, action_dtype, real_time_scale, freq_rate, precision, EMEI_INTEG_EULER,
                            next_obs_out, stream);
}
