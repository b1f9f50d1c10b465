// launch.h — host-side launch descriptors shared between the ABI layer and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pendulum_envs.h"

namespace emei {

// What a launch does.  One vocabulary for both kernel families (pend_launch: the 4-state kernels, NO = 4; body_launch: the body
// kernels); an op only one family serves falls into the other's `default:` refusal.  The fields each op reads beyond the handle's
// own (LaunchCommon; n_steps = the horizon wherever `plan` is read):
enum LaunchOp {
    // emei_rollout: actions [n_steps, n(, NA)], obs_out / reward_out / done_out or null, flags; *selected = the rollout kernel's id.
    // 4-state, n_steps = 1 (emei_step_host): obs_f64 also takes the float64 observation of the post-step state, host_flag the
    // completion word; peers.count > 0 -> the staged peers kernel or EMEI_ERR_UNSUPPORTED
    OP_ROLLOUT = 0,
    OP_RESET,     // emei_reset: seed
    OP_GET_OBS,   // emei_get_obs: obs_f64 [n, NO]
    OP_INIT_OBS,  // emei_episode_init_obs: n = the count, env_index, episode_in, obs_out
    OP_NEXT_OBS,  // emei_next_obs_io, no handle: obs_in, actions, obs_out in io_f64's dtype
    // emei_evaluate_sequences and the first launch of emei_plan_shooting / _mppi / _cem: `plan` (PlanMode), actions (PLAN_GIVEN),
    // obs_out = final_obs [n * K, NO] or null
    OP_PLAN,
    // emei_evaluate_sequences_value / emei_plan_shooting_value / _mppi_value / _cem_value: OP_PLAN's fields with the terminal value
    // network in `policy_value` (w1 non-null; out_mode, lo, hi and noisy unused) on the one-wave plan kernels; every mode keeps its
    // returns in plan.return_out (PLAN_DRAWN included)
    OP_PLAN_VALUE,
    // emei_mpc_mppi: n_steps control steps of MPPI with plan.n_candidates candidates over mpc.horizon steps under plan.discount;
    // plan.cand carries the call's seed, sigma and the ctrlrange (its nominal is unused: the kernel keeps mpc.nominal in LDS), `seed`
    // the handle's reset key; plan.return_out = the workspace [n * K]; mpc.actions_out, obs_out / reward_out / done_out and flags as
    // OP_ROLLOUT's; mpc.plan_return_out, mpc.ess_out, mpc.temperature, mpc.refill, mpc.nominal_lo / _hi
    OP_MPC_MPPI,
    // emei_mpc_cem: OP_MPC_MPPI's fields with the cross-entropy method as the planner — mpc.iterations refits to the mpc.n_elites best
    // candidates per control step, plan.cand.sigma the width every control step starts from, mpc.sigma_min the floor of the refitted
    // one; mpc.elite_return_out takes ess_out's place, temperature is unused
    OP_MPC_CEM,
    // emei_rollout_policy: OP_ROLLOUT's fields without `actions`; the weights, the ctrlrange and actions_out (4-state: in
    // policy.action_dtype; body: float32) travel in `policy`
    OP_POLICY,
    OP_POLICY_NOISY,  // emei_rollout_policy_noisy: OP_POLICY's fields and the noise of the call in `policy_noise`
    // emei_evaluate_policies: `policy` holds the STACKED weights (member p at p * its size; actions_out unused), `plan` what PLAN_GIVEN
    // takes with n_candidates = the number of policies and return_out / length_out [P, n] policy-major; obs_out = final_obs [P, n, NO]
    // or null
    OP_POLICY_EVAL,
    // emei_rollout_policy_deep: OP_POLICY_NOISY's fields with the two-hidden-layer network in `policy_deep` (policy_deep.noisy: whether
    // `policy_noise` is the call's noise or unused)
    OP_POLICY_DEEP,
    OP_POLICY_EVAL_DEEP,  // emei_evaluate_policies_deep: OP_POLICY_EVAL's fields with the STACKED networks in `policy_deep`
    // emei_plan_policy: `policy` and `policy_noise` as OP_POLICY_NOISY takes them (actions_out unused), `plan` what PLAN_DRAWN_KEEP
    // takes (cand unused: the candidates are the policy's noisy rollouts) plus plan.first_actions
    OP_POLICY_PLAN,
    // emei_plan_policy_deep: OP_POLICY_PLAN's fields with the two-hidden-layer network in `policy_deep` (noisy set) and the terminal
    // value network in `policy_value` (w1 null: no bootstrap; out_mode, lo, hi and noisy unused)
    OP_POLICY_PLAN_DEEP,
    // emei_mpc_policy: n_steps control steps of "plan around the policy, act, step" — OP_MPC_MPPI's n_steps, mpc.horizon,
    // mpc.actions_out, mpc.plan_return_out, mpc.ess_out, mpc.temperature, flags and `seed` without a nominal; mpc.plan_index_out,
    // mpc.act_mode; `policy` and `policy_noise` as OP_POLICY_PLAN takes them, control step t under the key policy_noise.seed + t *
    // mpc.seed_stride; plan.n_candidates, plan.discount; plan.return_out = the workspace: [n * K] float64 returns, then [n * K]
    // float32 first actions
    OP_MPC_POLICY,
    // -- the 4-state kernels only
    OP_REWARD_TERMINAL,  // emei_reward_io / emei_terminal_io, no handle: obs_in -> reward_out (io_f64's dtype) and / or done_out
    // -- the body kernels only
    OP_REWARD,     // emei_reward_io: obs_in, pre_obs_in, actions -> reward_out, all in io_f64's dtype; batch_cost_scratch
    OP_TERMINAL,   // emei_terminal_io: obs_in -> done_out
    OP_OCCUPANCY,  // host only: *selected = waves of the rollout kernel (of `integrator`) the current device holds at once
};

// emei_set_obs_peers: the gathered buffers the staged rollout kernel also writes every observation row to
struct ObsPeers {
    void* obs[EMEI_MAX_OBS_PEERS] = {};
    int64_t row_envs = 0, col = 0;
    int count = 0;
    int32_t max_steps = 0;  // rows of every buffer
};

// What the plan kernels of both families take beyond their base descriptor (OP_PLAN): n_candidates lanes per
// env score `horizon` steps each from one start state.
enum PlanMode {
    PLAN_GIVEN = 0,   // emei_evaluate_sequences: the candidates are `actions`; return_out / length_out (and final_obs) per candidate
    PLAN_DRAWN,       // emei_plan_shooting: the candidates are drawn in the lanes under `cand`, and the kernel leaves one PlanPartial
                      // per (wave, env) segment in `partials` instead of return_out / length_out
    PLAN_DRAWN_KEEP,  // emei_plan_mppi / emei_plan_cem: as PLAN_DRAWN, and every candidate's return is kept in return_out as well
};
struct PlanLaunch {
    int mode = PLAN_GIVEN;
    const double* start_rows = nullptr;  // [n, state_dim] float64; null = the handle's state
    int32_t n_candidates = 1;
    double discount = 1.0;
    double* return_out = nullptr;   // [n * K]
    int32_t* length_out = nullptr;  // [n * K]
    CandidateSpec cand = {};
    void* partials = nullptr;
    const float* sigma_map = nullptr;  // emei_plan_cem: non-null -> the draws take their sigma per entry (CandidateSpecMap)
    float* first_actions = nullptr;  // OP_POLICY_PLAN(_DEEP): [n * K(, act_dim)] float32, every candidate's action at t = 0
};

// What the fused controllers take beyond `plan` (OP_MPC_MPPI / OP_MPC_CEM / OP_MPC_POLICY)
struct MpcLaunch {
    int32_t horizon = 1;
    float* nominal = nullptr;     // in/out [horizon, n(, act_dim)]
    void* actions_out = nullptr;  // [n_steps, n(, act_dim)]; 4-state: in PendLaunch::action_dtype; body: float32
    double* plan_return_out = nullptr;  // [n_steps, n] or null
    double* ess_out = nullptr;          // MPPI, policy: [n_steps, n] or null
    double temperature = 1.0;           // MPPI, policy
    float refill = 0.f, nominal_lo = 0.f, nominal_hi = 0.f;
    int32_t n_elites = 1, iterations = 1;  // CEM
    float sigma_min = 0.f;
    double* elite_return_out = nullptr;  // CEM: [n_steps, n] or null
    int32_t act_mode = 0;                // policy: enum emei_mpc_policy_act
    uint64_t seed_stride = 0;
    int32_t* plan_index_out = nullptr;  // policy: [n_steps, n] or null
};

// What the launch descriptors of both families hold: the handle's part (abi.hip: handle_fields) and the call's
struct LaunchCommon {
    int op = OP_ROLLOUT;
    int env_id = 0, precision = 0;
    void* state = nullptr;
    int32_t* steps = nullptr;
    uint32_t* episode = nullptr;
    unsigned long long* done_mask = nullptr;
    int64_t n = 0;
    int32_t n_steps = 1, freq_rate = 1, max_episode_steps = 0;
    uint32_t flags = 0;
    uint64_t seed = 0, env_offset = 0;
    const void* trig = nullptr;  // device {sin,cos} table (emei_trig_table)
    hipStream_t stream = nullptr;
    int* selected = nullptr;  // out: enum emei_kernel_id of the kernel launched (emei_last_rollout_kernel)
    const void* actions = nullptr;
    const void* obs_in = nullptr;  // stateless ops: [n, NO] float32, or float64 when io_f64
    int io_f64 = 0;                // stateless ops: obs_in / obs_out / reward_out (body: pre_obs_in and the reward's actions too) are float64
    const int64_t* env_index = nullptr;  // OP_INIT_OBS
    const uint32_t* episode_in = nullptr;
    float* obs_out = nullptr;
    double* obs_f64 = nullptr;
    float* reward_out = nullptr;
    uint8_t* done_out = nullptr;
    PlanLaunch plan;
    MpcLaunch mpc;
    PolicyArgs policy = {};
    PolicyNoiseArgs policy_noise = {};
    PolicyDeepArgs policy_deep = {};
    PolicyDeepArgs policy_value = {};
};

struct PendLaunch : LaunchCommon {
    int ode_method = 0;       // enum emei_ode_method (CartPole only)
    int32_t action_dtype = 0;  // of `actions` and mpc.actions_out
    PendParams p;
    uint32_t* host_flag = nullptr;  // emei_step_host with n = 1: the kernel ends by storing flag_value here (host memory, system
    uint32_t flag_value = 0;        // scope, after everything else it wrote)
    ObsPeers peers;
};

// The deep policy kernels keep h1 in dynamic LDS (emei_device.h:policy_deep_tile_bytes, up to 64 KiB): the opt-in HIP wants of a
// kernel that asks for a large dynamic segment, made once per kernel and device for the cap.  Host only; no stream is involved.
template <auto Kernel>
inline int policy_deep_lds_opt_in() {
    constexpr int kMaxDevices = 64;
    static bool done[kMaxDevices] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return EMEI_ERR_HIP;
    if (dev >= 0 && dev < kMaxDevices && done[dev]) return EMEI_OK;
    if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)policy_deep_tile_bytes(EMEI_POLICY_DEEP_MAX_HIDDEN)) != hipSuccess)
        return EMEI_ERR_HIP;
    if (dev >= 0 && dev < kMaxDevices) done[dev] = true;
    return EMEI_OK;
}

// pendulum_kernels.hip
int pend_launch(const PendLaunch& L);

// abi.hip: the per-device 256-entry {sin,cos} table (allocated and filled on first use)
const void* emei_trig_table(int device);

// util_kernels.hip
int launch_state_unpack(const double* aos, void* soa, int precision, int64_t n, int dim, hipStream_t s);
int launch_state_pack(const void* soa, double* aos, int precision, int64_t n, int dim, hipStream_t s);
int launch_compact_done(const unsigned long long* masks, int64_t n, int32_t* idx_out, int32_t* count_out, hipStream_t s);
// emei_mpc_mppi's and emei_mpc_cem's follow-up: env i's last done code (word 0 of its workspace row of `stride` doubles) -> one ballot word per 64 envs
int launch_mpc_done_pack(const double* work, int64_t stride, int64_t n, unsigned long long* done_mask, hipStream_t s);
// emei_sample_candidates / the second launch of emei_plan_shooting (act_dim 0: a discrete env)
int launch_sample_candidates(const CandidateSpec& sp, int64_t n_envs, int32_t n_cand, int32_t horizon, int act_dim, void* actions_out,
                             int action_dtype, hipStream_t s);
int launch_plan_finish(const void* partials, const CandidateSpec& sp, int64_t n_envs, int32_t n_cand, int32_t horizon, int act_dim,
                       void* best_action, int action_dtype, void* best_sequence, double* best_return, int32_t* best_index,
                       int32_t* best_length, hipStream_t s);
// the second launch of emei_plan_mppi: `returns` [n_envs * n_cand] as the plan kernel left them (overwritten by the weights)
int launch_plan_mppi_finish(const void* partials, double* returns, const CandidateSpec& sp, int64_t n_envs, int32_t n_cand, int32_t horizon,
                            int act_dim, double temperature, float* nominal_out, double* best_return, int32_t* best_index, double* ess,
                            hipStream_t s);
// emei_plan_policy keeps every candidate's action of step 0 in its workspace, sized without a handle: the widest action of the envs
// (the HalfCheetah's six components); launch_plan_policy_finish refuses more
constexpr int kPlanPolicyMaxAct = 6;
// the second launch of emei_plan_policy: `returns` and `first` [n_envs * n_cand(, act_dim)] as the policy plan kernel left them (read
// only); mean_out / ess null: the weights are not formed and temperature is not read
int launch_plan_policy_finish(const void* partials, const double* returns, const float* first, int64_t n_envs, int32_t n_cand, int act_dim,
                              double temperature, void* best_action, int action_dtype, float* mean_out, double* best_return,
                              int32_t* best_index, int32_t* best_length, double* ess, hipStream_t s);
// emei_sample_candidates_sigma: the Gaussian mode with a sigma per entry
int launch_sample_candidates_sigma(const CandidateSpecMap& sp, int64_t n_envs, int32_t n_cand, int32_t horizon, int act_dim, void* actions_out,
                                   hipStream_t s);
// the second launch of emei_plan_cem: `returns` as the plan kernel left them (overwritten by the 0 / 1 membership); sigma_map null:
// the draws of `sp`, else those of CandidateSpecMap(sp, sigma_map)
int launch_plan_cem_finish(const void* partials, double* returns, const CandidateSpec& sp, const float* sigma_map, int64_t n_envs,
                           int32_t n_cand, int32_t n_elites, int32_t horizon, int act_dim, float* mean_out, float* std_out,
                           double* best_return, int32_t* best_index, double* elite_return, hipStream_t s);

}  // namespace emei
