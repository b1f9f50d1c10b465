// pendulum_kernels.h — step / rollout kernels of the 4-state cart/pole family for gfx950.
//
// Layout: one thread per env instance; state is struct-of-arrays in HBM (4 arrays of n Reals + a
// step counter and an episode counter per env), so every state access of a wave is one fully
// coalesced 256 B (float) / 512 B (double) line group.  Observations leave as one float4 per lane
// (row-major [n,4] float32 = a 1 KiB contiguous store per wave).  The rollout keeps the state,
// the carried sin/cos and the counters in registers for all n_steps; per step it reads one action
// and writes obs + reward + done (22 B/env-step with uint8 actions).
// There is no dense contraction anywhere on this path, hence no MFMA: the roofline is HBM.
#pragma once
#include <type_traits>

#include "pendulum_envs.h"
#include "launch.h"

namespace emei {

template <class Env>
struct RolloutArgs {
    typename Env::real* state;  // SoA: 4 arrays of n
    int32_t* steps;             // per-env step counter (TimeLimit)
    uint32_t* episode;          // per-env episode counter (RNG counter word)
    unsigned long long* done_mask;  // one ballot word per wave: done of the LAST step
    const void* actions;
    const SinCosEntry* trig;  // 256-entry {sin,cos} table in device memory (abi.hip: emei_trig_table)
    float4* obs_out;
    float* reward_out;
    uint8_t* done_out;
    int64_t n;
    int32_t n_steps, freq_rate, action_dtype, max_episode_steps;
    uint32_t flags;
    uint64_t seed, env_offset;
    typename Env::Params p;
    // the generic kernel only (emei_step_host; appended so that no other field moves): see launch.h
    double* obs_f64;
    uint32_t* host_flag;
    uint32_t flag_value;
    uint32_t xcd_contiguous;  // staged kernel: see the env_block map (set by launch_rollout_full when gridDim.x % 8 == 0)
    uint32_t first_block;  // staged kernel: a launch may cover the blocks [first_block, first_block + gridDim.x) of the shard (launch_rollout_full)
};

// emei_set_obs_peers (multi-GPU observation return by peer writes): where the staged rollout kernel ALSO stores every step's
// observation — up to EMEI_MAX_OBS_PEERS gathered buffers [n_steps, row_envs, 4] float32 (hipIpc-mapped memory of the other ranks, and
// this rank's own), this shard's envs at columns [col, col + n).  A kernel argument of its own, so that the kernel without peers keeps
// its arguments (and its code) unchanged.
struct PeerObs {
    float4* obs[EMEI_MAX_OBS_PEERS];
    int64_t row_envs, col;
    uint32_t count;
};

// emei_step (n_steps = 1) and emei_rollout (n_steps = T): base_control.py:61-83 /
// mujoco_env.py:157-167 for every env of the shard, T times, without leaving the registers.
// FULL = all three outputs are non-null: the stores are then unconditional, which lets the compiler
// count them and wait for a chunk's action loads with vmcnt(3*kChunk) instead of vmcnt(0).
template <class Env, typename ActT, bool FULL>
__global__ void __launch_bounds__(kBlock) pend_rollout_kernel(const RolloutArgs<Env> a) {
    using R = typename Env::real;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, a.trig, Env::trig_rot_c(), Env::trig_rot_s());
    const ActT* __restrict__ actions = (const ActT*)a.actions;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t n = a.n;
    const uint32_t li = (uint32_t)i;  // n_envs < 2^31 (checked in emei_create)

    R s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = a.state[k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, a.p);

    const bool auto_reset = (a.flags & EMEI_FLAG_AUTO_RESET) != 0;
    // Actions are fetched a whole chunk of kChunk steps ahead of their use.  On gfx950 loads and
    // stores share one in-order counter (vmcnt), so waiting for a load also waits for every OLDER
    // store: with the loads issued one chunk early, the only stores older than them were issued
    // >= kChunk steps ago and have long retired, and the 3*kChunk stores of the current chunk stay in
    // flight behind the wait.  (Fetching one step ahead put the HBM write latency of the previous
    // step's stores on the serial per-env chain: 2.3x slower.)
    // The action dtype is a template parameter and out-of-range steps are clamped rather than
    // branched around, so the kChunk loads are one straight-line burst and the compiler can count
    // them (a dtype switch around each load made it fall back to vmcnt(0) after every load).
    constexpr int kChunk = 8;
    const int last = a.n_steps - 1;
    ActT cur[kChunk], nxt[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) cur[j] = (actions + (int64_t)min(j, last) * n)[li];
    uint32_t done = 0;
    auto do_step = [&](int t, ActT raw) __attribute__((always_inline)) {
        R o[4], rew;
        bool term;
        Env::step(s, c, Env::decode_t(raw), a.p, a.freq_rate, o, rew, term);
        ++steps;
        bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
        done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);

        // uniform (scalar) row base + 32-bit lane index: the address costs no vector instruction
        const int64_t row = (int64_t)t * n;
        if (FULL || a.obs_out) (a.obs_out + row)[li] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
        if (FULL || a.reward_out) (a.reward_out + row)[li] = (float)rew;
        if (FULL || a.done_out) (a.done_out + row)[li] = (uint8_t)done;

        // early-termination handling: the reset path (Philox + a fresh sincos) is skipped by the
        // whole wave unless the ballot says some lane is done
        if (auto_reset && __ballot(done != 0) != 0ull) {
            if (done != 0) {
                ++episode;
                steps = 0;
                Env::init(s, a.seed, a.env_offset + (uint64_t)i, episode, a.p);
                Env::prime(s, c, a.p);
            }
        }
    };
    int t0 = 0;
    // full chunks: no per-step bounds check, so every path through the body issues exactly
    // 3*kChunk stores after the prefetch and the wait for it can leave them all in flight
    for (; t0 + kChunk <= a.n_steps; t0 += kChunk) {
#pragma unroll
        for (int j = 0; j < kChunk; ++j) nxt[j] = (actions + (int64_t)min(t0 + kChunk + j, last) * n)[li];
#pragma unroll
        for (int j = 0; j < kChunk; ++j) do_step(t0 + j, cur[j]);
#pragma unroll
        for (int j = 0; j < kChunk; ++j) cur[j] = nxt[j];
    }
    // tail (< kChunk steps); also the whole of emei_step (n_steps = 1)
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
        if (t0 + j >= a.n_steps) break;
        do_step(t0 + j, cur[j]);
    }

#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[k * n + i] = s[k];
    a.steps[i] = steps;
    a.episode[i] = episode;
    // done bits of the last step, one 64-bit word per wave, for emei_compact_done
    unsigned long long m = __ballot(done != 0);
    if ((threadIdx.x & (kWave - 1)) == 0) a.done_mask[i / kWave] = m;
    if (a.obs_f64) {  // emei_step_host: the state's observation in float64 (after an auto-reset: the new episode's), as emei_get_obs
        R o[4];
        Env::obs_of(s, o);
        double2* dst = (double2*)(a.obs_f64 + 4 * i);
        dst[0] = make_double2((double)o[0], (double)o[1]);
        dst[1] = make_double2((double)o[2], (double)o[3]);
    }
    if (a.host_flag) {  // n = 1 (checked on the host): this thread wrote every result; release them to the host, then the flag
        __threadfence_system();
        __hip_atomic_store(a.host_flag, a.flag_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// emei_rollout_policy (the normative text: include/emei_hip.h): the loop of pend_rollout_kernel with the action load replaced by the
// lane's own evaluation of the policy on the observation it holds — x_0 from the state as emei_get_obs gives it, then the row each step
// emits, or the new episode's first observation after an auto-reset (what pend_init_obs_kernel computes).  One lane per env, state /
// carry / counters in registers, the same Env::step, reset and done-mask tail.  Nothing is fetched per step, so there is no
// prefetch and no chunking of the loop; the weights arrive as scalar loads (emei_device.h:policy_eval).  `a.actions` is unused,
// any output may be null.
template <class Env>
__global__ void __launch_bounds__(kBlock) pend_policy_rollout_kernel(const RolloutArgs<Env> a, const PolicyArgs pol) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, a.trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t n = a.n;
    const uint32_t li = (uint32_t)i;  // n_envs < 2^31 (checked in emei_create)

    R s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = a.state[k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, a.p);

    const bool auto_reset = (a.flags & EMEI_FLAG_AUTO_RESET) != 0;
    float x[4];
    {
        R o[4];
        Env::obs_of(s, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
    }
    uint32_t done = 0;
    for (int t = 0; t < a.n_steps; ++t) {
        float av[1];
        policy_eval<4, 1, Env::kDiscrete>(pol, x, av);
        const int64_t row = (int64_t)t * n;  // uniform (scalar) row base + 32-bit lane index
        if (pol.actions_out) store_action(pol.actions_out, pol.action_dtype, row + li, av[0]);
        R o[4], rew;
        bool term;
        Env::step(s, c, Env::decode_t((DrawT)av[0]), a.p, a.freq_rate, o, rew, term);
        ++steps;
        bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
        done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
        if (a.obs_out) (a.obs_out + row)[li] = make_float4(x[0], x[1], x[2], x[3]);
        if (a.reward_out) (a.reward_out + row)[li] = (float)rew;
        if (a.done_out) (a.done_out + row)[li] = (uint8_t)done;
        if (auto_reset && __ballot(done != 0) != 0ull) {
            if (done != 0) {
                ++episode;
                steps = 0;
                Env::init(s, a.seed, a.env_offset + (uint64_t)i, episode, a.p);
                Env::prime(s, c, a.p);
                Env::obs_of(s, o);
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
            }
        }
    }

#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[k * n + i] = s[k];
    a.steps[i] = steps;
    a.episode[i] = episode;
    // done bits of the last step, one 64-bit word per wave, for emei_compact_done
    unsigned long long m = __ballot(done != 0);
    if ((threadIdx.x & (kWave - 1)) == 0) a.done_mask[i / kWave] = m;
}

// emei_rollout_policy_noisy: pend_policy_rollout_kernel with the exploration term of step t drawn in the lane under the key
// nz.seed + t (emei_device.h:policy_eval_t<NOISY>); nothing else differs.  A kernel of its own name, so that the deterministic one
// stays the code it was.
template <class Env>
__global__ void __launch_bounds__(kBlock) pend_policy_rollout_noisy_kernel(const RolloutArgs<Env> a, const PolicyArgs pol,
                                                                           const PolicyNoiseArgs nz) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, a.trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t n = a.n;
    const uint32_t li = (uint32_t)i;  // n_envs < 2^31 (checked in emei_create)

    R s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = a.state[k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, a.p);

    const bool auto_reset = (a.flags & EMEI_FLAG_AUTO_RESET) != 0;
    float x[4];
    {
        R o[4];
        Env::obs_of(s, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
    }
    uint32_t done = 0;
    for (int t = 0; t < a.n_steps; ++t) {
        float av[1];
        policy_eval_t<4, 1, Env::kDiscrete, true>(pol, nz, nz.seed + (uint64_t)t, a.env_offset + (uint64_t)i, x, av);
        const int64_t row = (int64_t)t * n;  // uniform (scalar) row base + 32-bit lane index
        if (pol.actions_out) store_action(pol.actions_out, pol.action_dtype, row + li, av[0]);
        R o[4], rew;
        bool term;
        Env::step(s, c, Env::decode_t((DrawT)av[0]), a.p, a.freq_rate, o, rew, term);
        ++steps;
        bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
        done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
        if (a.obs_out) (a.obs_out + row)[li] = make_float4(x[0], x[1], x[2], x[3]);
        if (a.reward_out) (a.reward_out + row)[li] = (float)rew;
        if (a.done_out) (a.done_out + row)[li] = (uint8_t)done;
        if (auto_reset && __ballot(done != 0) != 0ull) {
            if (done != 0) {
                ++episode;
                steps = 0;
                Env::init(s, a.seed, a.env_offset + (uint64_t)i, episode, a.p);
                Env::prime(s, c, a.p);
                Env::obs_of(s, o);
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
            }
        }
    }

#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[k * n + i] = s[k];
    a.steps[i] = steps;
    a.episode[i] = episode;
    // done bits of the last step, one 64-bit word per wave, for emei_compact_done
    unsigned long long m = __ballot(done != 0);
    if ((threadIdx.x & (kWave - 1)) == 0) a.done_mask[i / kWave] = m;
}

// emei_rollout_policy_deep: pend_policy_rollout_noisy_kernel's loop under the network with two hidden layers
// (emei_device.h:policy_eval_deep_t; the noise is that function's wave-uniform switch pol.noisy, so this one kernel serves the call
// with and without it).  ONE-WAVE blocks: block b is env wave b, and the block's dynamic LDS is the wave's h1 tile.
template <class Env>
__global__ void __launch_bounds__(kWave) pend_policy_rollout_deep_kernel(const RolloutArgs<Env> a, const PolicyDeepArgs pol,
                                                                         const PolicyNoiseArgs nz) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    extern __shared__ __attribute__((aligned(16))) float4 deep_h1_s[];
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table<kWave>(trig_s, a.trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (i >= a.n) return;
    const int64_t n = a.n;
    const uint32_t li = (uint32_t)i;  // n_envs < 2^31 (checked in emei_create)

    R s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = a.state[k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, a.p);

    const bool auto_reset = (a.flags & EMEI_FLAG_AUTO_RESET) != 0;
    float x[4];
    {
        R o[4];
        Env::obs_of(s, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
    }
    uint32_t done = 0;
    for (int t = 0; t < a.n_steps; ++t) {
        float av[1];
        policy_eval_deep_t<4, 1, Env::kDiscrete>(pol, nz, nz.seed + (uint64_t)t, a.env_offset + (uint64_t)i, x, av, deep_h1_s,
                                                 (int)threadIdx.x);
        const int64_t row = (int64_t)t * n;  // uniform (scalar) row base + 32-bit lane index
        if (pol.actions_out) store_action(pol.actions_out, pol.action_dtype, row + li, av[0]);
        R o[4], rew;
        bool term;
        Env::step(s, c, Env::decode_t((DrawT)av[0]), a.p, a.freq_rate, o, rew, term);
        ++steps;
        bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
        done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
        if (a.obs_out) (a.obs_out + row)[li] = make_float4(x[0], x[1], x[2], x[3]);
        if (a.reward_out) (a.reward_out + row)[li] = (float)rew;
        if (a.done_out) (a.done_out + row)[li] = (uint8_t)done;
        if (auto_reset && __ballot(done != 0) != 0ull) {
            if (done != 0) {
                ++episode;
                steps = 0;
                Env::init(s, a.seed, a.env_offset + (uint64_t)i, episode, a.p);
                Env::prime(s, c, a.p);
                Env::obs_of(s, o);
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
            }
        }
    }

#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[k * n + i] = s[k];
    a.steps[i] = steps;
    a.episode[i] = episode;
    // done bits of the last step, one 64-bit word per wave, for emei_compact_done
    unsigned long long m = __ballot(done != 0);
    if (threadIdx.x == 0) a.done_mask[i / kWave] = m;
}

// ---------------------------------------------------------------------------------------------
// Staged rollout: the fast path of emei_rollout (all outputs present, n a multiple of 64,
// 16-byte aligned buffers).  Same arithmetic and results as pend_rollout_kernel; what changes is
// how bytes move.  A wave owns 64 consecutive envs, i.e. a 64-column stripe of the [T, N] action,
// reward and done arrays, and stages kStage = 16 steps of that stripe through its private slice of
// LDS so that every global access is a full 16 B per lane:
//   actions : one global_load_dwordx4 per lane and sizeof(ActT) fetches a 16-step tile, LDS holds it
//             row-major, each step reads its own element back (ds_read, lgkm counter: the wait no
//             longer sits behind the stores, which share vmcnt with loads on gfx950)
//   reward  : ds_write_b32 per step; every 4 steps one ds_read_b128 + global_store_dwordx4 (4 rows)
//   done    : ds_write_b8 per step; every 16 steps one ds_read_b128 + global_store_dwordx4 (16 rows)
//   obs     : already 16 B per lane, stored directly
// => 1.31 vector stores + 1/16 loads per env-step instead of 3 stores + 1 load, and no 64 B
// partial-line byte stores.  LDS slices are wave-private (LDS operations of one wave execute in
// order), so there is no barrier anywhere (an optional one per tile, Env::kTileBarrier, is off: see its comment).
// steps per staged tile: 16 for one-byte actions (1 KiB of LDS per wave and buffer); 8 for 4- and 8-byte actions, so that
// the double-buffered tiles of a 256-thread block stay at 16 / 32 KiB and four blocks (with the other slices) fit a CU's
// 160 KiB: config 3 runs 4 waves per SIMD
#ifndef EMEI_TILE_BARRIER
#define EMEI_TILE_BARRIER 1  // with Env::kTileBarrier: the per-tile block barrier of the staged kernel (A/B history: see its comment)
#endif
#ifndef EMEI_PRIO_ROTATE
#define EMEI_PRIO_ROTATE 1  // 0: a variant build without the priority rotation of the staged kernel, for A/B runs
#endif
template <typename ActT>
constexpr int stage_steps() { return sizeof(ActT) == 1 ? 16 : 8; }

// The body of the two staged kernels below (PEERS: with the peer stores of emei_set_obs_peers).
template <class Env, typename ActT, bool FREQ1, bool PEERS>
__device__ __forceinline__ void pend_rollout_staged(const RolloutArgs<Env>& a, const PeerObs& peers) {
    using R = typename Env::real;
    constexpr int kWavesPerBlock = kBlock / kWave;
    constexpr int kStage = stage_steps<ActT>();
    constexpr int kTileWaitKeep = kStage;  // VMEM operations left in flight when a staged action tile is retired
    constexpr int kActVec = kStage * sizeof(ActT) / 16;  // 1 KiB wave-loads (16 B per lane) per kStage x 64 tile of ActT
    static_assert(kStage % 4 == 0 && kStage * kWave * sizeof(ActT) % 1024 == 0, "whole wave-loads, whole reward groups");
    __shared__ uint4 act_s[kWavesPerBlock][2][kStage * kWave * sizeof(ActT) / 16];
    __shared__ float rew_s[kWavesPerBlock][4][kWave];
    __shared__ uint8_t done_s[kWavesPerBlock][kStage][kWave];
    // spare initial states (see maybe_reset): in LDS for the envs that run several waves per SIMD (registers are their
    // occupancy limit), in registers otherwise
    constexpr bool kLdsSpare = Env::kSpareInLds;
    __shared__ R spare_s[kLdsSpare ? kWavesPerBlock : 1][6][kLdsSpare ? kWave : 1];

    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, a.trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#if defined(EMEI_BLOCK_SWIZZLE)  // experiment: which env block a workgroup (and so an XCD) works on
    const int64_t i = (int64_t)((blockIdx.x + a.first_block) ^ (unsigned)EMEI_BLOCK_SWIZZLE) * kBlock + threadIdx.x;
#else
    // Which env block a workgroup works on.  Workgroups go to the 8 XCDs round-robin (workgroup b -> XCD b mod 8).  With
    // a.xcd_contiguous (shards of more than one wave per SIMD: launch_rollout_full) XCD k gets ONE contiguous eighth of the launch's
    // envs, i.e. of every output row, instead of every eighth 4 KiB piece: 131 072 envs 0.676 -> 0.615 ms, 1 048 576 envs 5.61 ->
    // 5.01 ms on one box; nothing (or slightly worse) at 65 536 envs, where the identity stays (profiles/r05_split_launch.txt).
    // Results do not depend on it (envs are independent); the map is fixed, so an env's lines stay in one XCD's L2 across launches.
    const unsigned env_block = a.xcd_contiguous ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int64_t i = (int64_t)(env_block + a.first_block) * kBlock + threadIdx.x;  // n % 64 == 0: whole waves only
#endif
    if (i >= a.n) return;
#if defined(EMEI_XCD_ONLY)  // experiment (timing only, results of the skipped envs are not produced): only the workgroups of the XCDs in this bit mask work
    if (!(((unsigned)EMEI_XCD_ONLY >> (blockIdx.x & 7u)) & 1u)) return;
#endif
    EMEI_CLOCK_BEGIN();
    const int64_t n = a.n;
    const uint32_t li = (uint32_t)i, i0 = li - (uint32_t)lane;
    const ActT* __restrict__ actions = (const ActT*)a.actions;

    R s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = a.state[k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, a.p);
    const bool auto_reset = (a.flags & EMEI_FLAG_AUTO_RESET) != 0;
    const int last = a.n_steps - 1;
    uint32_t done = 0;

    // tile geometry of one 16-byte vector v (0..kActVec-1) of this lane inside a 16-step tile
    constexpr int kLanesPerRow = kWave * sizeof(ActT) / 16;  // lanes that cover one 64-env row
    constexpr int kRowsPerVec = kWave / kLanesPerRow;        // rows one wave-wide vector load covers
    const int rsub = lane / kLanesPerRow, cbyte = (lane % kLanesPerRow) * 16;
    const char* act_lane_base = (const char*)(actions + i0) + cbyte;  // this lane's column inside a row
    const int64_t act_row_bytes = n * (int64_t)sizeof(ActT);
    // Action tiles go global -> LDS directly (LDS-DMA, global_load_lds_dwordx4): one wave-instruction
    // writes 1 KiB of LDS linearly (lane l -> base + 16 l), which is exactly the row-major tile image,
    // and no VGPR carries the tile across the 16 steps it is in flight (held in registers, hipcc
    // parked it in scratch and stalled on the load at once).  hipcc does not count asm memory
    // operations, so the wait that retires a tile is written out below (EMEI_TILE_WAIT).
    const uint32_t act_lds0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)&act_s[wv][0][0]);
    constexpr uint32_t kTileBytes = kStage * kWave * sizeof(ActT);
#define EMEI_LOAD_TILE(T0, BUF)                                                                           \
    _Pragma("unroll") for (int k_ = 0; k_ < kActVec; ++k_) {                                             \
        const int row_ = min((T0) + k_ * kRowsPerVec + rsub, last); /* never read past step T-1 */        \
        const char* src_ = act_lane_base + row_ * act_row_bytes;                                          \
        const uint32_t dst_ = act_lds0 + (uint32_t)(BUF) * kTileBytes + (uint32_t)k_ * 1024u;              \
        uint32_t keep_;                                                                                   \
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" \
                     : "=&s"(keep_) : "v"(src_), "s"(dst_) : "memory");                                    \
    }

    // FREQ1: freq_rate == 1 is resolved at compile time (no substep loop, no loop branches: every
    // taken branch costs a lone wave an instruction-buffer refill)
    const int freq_rate = FREQ1 ? 1 : a.freq_rate;
    auto advance = [&](ActT raw, R (&o)[4], R& rew) __attribute__((always_inline)) {
        bool term;
        Env::step(s, c, Env::decode_t(raw), a.p, freq_rate, o, rew, term);
        ++steps;
        bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
        done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
    };
    // Early termination.  The reset of a lane needs a fresh initial state (Philox4x32-10 + the env's
    // init distribution + its sin/cos): ~150-300 vector instructions that the whole wave executes for
    // the one or two lanes that are done.  Each lane therefore keeps a SPARE initial state for its next
    // episode: a reset just copies it, and spares are re-drawn only when a resetting lane has none —
    // then for every lane without one at once (the first reset of a wave draws all 64).  The draw is a
    // pure function of (seed, global env, episode), so results do not depend on when it is computed.
    R sp[4] = {R(0), R(0), R(0), R(0)}, sp_sn = R(0), sp_cs = R(0);  // dead outside the redraw when the spare lives in LDS
    float sp_e0 = 0.f, sp_e1 = 0.f;  // the non-trigonometric part of the spare's carry (Env::save_extra / load_extra)
    const unsigned long long reset_mask = auto_reset ? ~0ull : 0ull;
    // which lanes hold a spare: a wave-uniform 64-bit mask in scalar registers (ballot results and scalar logic only), so
    // that the bookkeeping of a reset costs no vector instruction; `inverse_ballot` turns it back into a lane predicate.
    // Env::kSpareFlagInVgpr (InvPend: its float64 literals fill the scalar file, hipcc kept the mask in two lanes of a
    // spill register — 2 v_readlane + 2 v_writelane + 2 v_readlane per resetting step, and some lane resets in 95 % of
    // config 3's wave-steps): a per-lane flag instead, 3 (>= every done code) where the lane holds a spare, else 0 — the
    // "a resetting lane has no spare" test is then ONE comparison, done > flag, and taking the spare one v_mov
    constexpr bool kVFlag = Env::kSpareFlagInVgpr;
    unsigned long long spare_mask = 0ull;
    uint32_t spare_flag = 0u;
    auto maybe_reset = [&]() __attribute__((always_inline)) {
#if defined(EMEI_NO_RESET)  // experiment (timing only, wrong results after the first done): what the per-step reset check and its block boundary cost
        return;
#endif
        EMEI_STAT_WAVE(16);  // staged-kernel event counters of a -DEMEI_NEWTON_STATS build (tools/pend_stats.py): env-steps (waves)
        const unsigned long long done_mask = __ballot(done != 0) & reset_mask;
        // cold for most envs: laid out of line so that the usual case falls through (Env::kResetLikely: in line)
        if (__builtin_expect(done_mask != 0ull, Env::kResetLikely ? 1 : 0)) {  // scalar test: no vector instruction
            EMEI_STAT_WAVE(17);  // ... steps in which some lane resets
            const bool refill = kVFlag ? (__ballot(done > spare_flag) & reset_mask) != 0ull : (done_mask & ~spare_mask) != 0ull;
            if (__builtin_expect(refill, 0)) {  // a resetting lane has no spare: redraw for every lane without one
                EMEI_STAT_WAVE(18);  // ... spare refills
                if (kVFlag ? spare_flag == 0u : __builtin_amdgcn_inverse_ballot_w64(~spare_mask)) {
                    typename Env::Carry sc;
                    sc.trig = c.trig;
                    Env::init(sp, a.seed, a.env_offset + (uint64_t)i, episode + 1u, a.p);
                    Env::prime(sp, sc, a.p);
                    if constexpr (kLdsSpare) {
                        spare_s[wv][0][lane] = sp[0], spare_s[wv][1][lane] = sp[1], spare_s[wv][2][lane] = sp[2];
                        spare_s[wv][3][lane] = sp[3], spare_s[wv][4][lane] = sc.sn, spare_s[wv][5][lane] = sc.cs;
                    } else {
                        sp_sn = sc.sn, sp_cs = sc.cs;
                        Env::save_extra(sc, sp_e0, sp_e1);
                    }
                }
                spare_mask = ~0ull, spare_flag = 3u;
            }
            if (__builtin_amdgcn_inverse_ballot_w64(done_mask)) {
                ++episode;
                steps = 0;
                if constexpr (kLdsSpare) {  // a lane only ever reads what it wrote itself: no fence
                    s[0] = spare_s[wv][0][lane], s[1] = spare_s[wv][1][lane], s[2] = spare_s[wv][2][lane];
                    s[3] = spare_s[wv][3][lane], c.sn = spare_s[wv][4][lane], c.cs = spare_s[wv][5][lane];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] = sp[k];
                    c.sn = sp_sn, c.cs = sp_cs;
                    Env::load_extra(c, sp_e0, sp_e1);
                }
                spare_flag = 0u;
            }
            spare_mask &= ~done_mask;
        }
    };
    // per-lane element offsets inside a flushed block of rows, computed once (the per-step address
    // is then a scalar row base plus this constant: no 64-bit vector multiply on the hot path)
    const int64_t rew_lane_off = (int64_t)(lane >> 4) * n + i0 + ((lane & 15) << 2);  // 16 lanes x 16 B per row
    const int64_t done_lane_off = (int64_t)(lane >> 2) * n + i0 + ((lane & 3) << 4);  // 4 lanes x 16 B per row
#if defined(EMEI_EXP_FLUSH_ROW0)  // experiment (timing only): the reward / done flushes always hit the first rows
#define EMEI_FLUSH_ROW(r) ((r) & 0)
#else
#define EMEI_FLUSH_ROW(r) (r)
#endif
    auto store_rew_rows = [&](int64_t row0, const float4& v) __attribute__((always_inline)) {
        store16_stream((float4*)(a.reward_out + EMEI_FLUSH_ROW(row0) * n + rew_lane_off), v);
    };
    auto store_done_rows = [&](int64_t row0, const uint4& v) __attribute__((always_inline)) {
        if (kStage == 16 || lane < 4 * kStage) store16_stream((uint4*)(a.done_out + EMEI_FLUSH_ROW(row0) * n + done_lane_off), v);  // kStage rows x 64 B
    };

    // Issue priority (Env::kRotatePriority: the InvertedPendulum kernels).  The SIMD's arbiter serves the OLDEST of its ready waves
    // first: of the four waves that share a SIMD (config 3) the first finishes after 45 % of the launch, the second after 60 %,
    // the third after 80 % (lifetimes in four clean groups of 1024 waves, profiles/r05_clock_probe.txt) and the SIMD ends the
    // launch with one wave.  Every tile the wave sets its priority to (tile + its wave slot) mod 4 — slots are 0..3, measured —
    // so that each of the four is the favoured one a quarter of the time.  Worth 6 % for the Balancing variants (0.683 -> 0.643 ms),
    // 0-3 % for SwingUp; finer rotation (every step, every two) is no better; for the HBM-bound CartPole kernel at two waves per
    // SIMD it was -8 % on one box and +4 % on another: not applied there.  s_setprio takes an immediate, hence the switch.
    const uint32_t wave_slot = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 4) & 3u;  // HW_REG_HW_ID (4), WAVE_ID = bits [3:0]
    auto rotate_priority = [&](uint32_t tile) __attribute__((always_inline)) {
#if EMEI_PRIO_ROTATE
        if constexpr (Env::kRotatePriority) switch ((tile + wave_slot) & 3u) {
            case 0: __builtin_amdgcn_s_setprio(0); break;
            case 1: __builtin_amdgcn_s_setprio(1); break;
            case 2: __builtin_amdgcn_s_setprio(2); break;
            default: __builtin_amdgcn_s_setprio(3); break;
        }
#endif
    };
    // PEERS: the observation row of step t also goes to every peer's gathered buffer (remote stores over xGMI: the launch then runs at the
    // links' rate, which is what the separate all-gather would take).  They are further stores AFTER the tile's loads in the shared in-order
    // counter, so the retire wait below (at most kStage operations left in flight) still covers every load.
    auto store_obs_peers = [&](int t, const float4& v) __attribute__((always_inline)) {
        if constexpr (PEERS) {
            const int64_t at = (int64_t)t * peers.row_envs + peers.col + li;
            for (uint32_t p = 0; p < peers.count; ++p) peers.obs[p][at] = v;
        }
    };
    EMEI_LOAD_TILE(0, 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int t0 = 0, buf = 0;
    // The LDS read of a flush is issued at the end of one step and its global store after the
    // arithmetic of the NEXT step (each step is its own scheduling region because of the reset
    // check, so a read placed next to its use would expose the LDS latency on the serial chain).
    // Which step flushes what is known at compile time inside the unrolled tile; only the hand-over
    // from the previous tile (step 0) is a run-time, wave-uniform condition.
    float4 rew_pend = make_float4(0.f, 0.f, 0.f, 0.f);
    uint4 done_pend = make_uint4(0u, 0u, 0u, 0u);
    for (; t0 + kStage <= a.n_steps; t0 += kStage, buf ^= 1) {
        EMEI_LOAD_TILE(t0 + kStage, buf ^ 1)  // next tile: in flight under the 16 steps below
        rotate_priority((uint32_t)(t0 / kStage));
        const ActT* act_l = (const ActT*)&act_s[wv][buf][0];
        ActT act_cur = act_l[lane];
        // 16 steps = 4 groups x 4 unrolled steps (one reward flush period), the group loop unrolled by two: at the loop's
        // back-edge hipcc moves the carried state back into its canonical registers (~18 copies), and with 8 steps per trip
        // that costs half as much per step — A/B on one box: 0.279 -> 0.270 ms (SwingUp), 0.165 -> 0.160 (Balancing),
        // 0.613 -> 0.605 (InvertedPendulum).  All 16 unrolled is faster still for Balancing but bimodal for SwingUp
        // (0.267 / 0.291 ms: the instruction cache two CUs share).
#ifndef EMEI_GROUP_UNROLL
#define EMEI_GROUP_UNROLL 2
#endif
#pragma unroll EMEI_GROUP_UNROLL
        for (int g = 0; g < kStage / 4; ++g) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 4 * g + q;
                // the next step's action leaves LDS while this step computes
                const ActT act_now = act_cur;
                act_cur = act_l[min(j + 1, kStage - 1) * kWave + lane];
                R o[4], rew;
                advance(act_now, o, rew);
                const float4 obs4 = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
#if defined(EMEI_EXP_OBS_ROW0)  // experiment (timing only): the observation stores alternate between rows 0 and 1 — the same instructions, no HBM write stream
                (a.obs_out + (int64_t)((t0 + j) & 1) * n)[li] = obs4;
#else
                store16_stream(a.obs_out + (int64_t)(t0 + j) * n + li, obs4);
#endif
                store_obs_peers(t0 + j, obs4);
                if (q == 0) {  // rows staged during the previous group: their LDS read has landed
                    if (t0 + j > 0) store_rew_rows(t0 + j - 4, rew_pend);
                    if (g == 0 && t0 > 0) store_done_rows(t0 - kStage, done_pend);
                }
                rew_s[wv][q][lane] = (float)rew;
                done_s[wv][j][lane] = (uint8_t)done;
                if (q == 3) {
                    wave_lds_fence();  // the flush reads what OTHER lanes staged
                    rew_pend = ((const float4*)&rew_s[wv][0][0])[lane];                             // 4 rows x 256 B
                    if (g == kStage / 4 - 1) done_pend = ((const uint4*)&done_s[wv][0][0])[lane & (4 * kStage - 1)];  // kStage rows x 64 B
                    wave_lds_fence();  // ... and is done before the next group overwrites the slice
                }
                maybe_reset();
            }
        }
        // Retire the tile.  Loads, stores and LDS-DMA share one in-order counter, and the tile's loads were
        // issued before ALL of this tile's stores, of which the kStage observation stores are unconditional
        // (the reward / done flushes add 1 to 5 more): leaving the kTileWaitKeep = kStage youngest operations
        // in flight therefore covers every LDS-DMA load, and what it additionally waits for was issued at
        // least kStage - 3 steps ago.  The count is DERIVED from the tile constants — a hand-written 19
        // (16 + the first tile's 3 reward flushes) was exact with zero margin — and tests/test_isa_guards.py
        // checks the emitted immediate and the stores of the loop body in the shipped code object.
        static_assert(kTileWaitKeep == kStage && kTileWaitKeep < 64, "one unconditional obs store per staged step");
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kTileWaitKeep) : "memory");
        // Env::kTileBarrier (no env sets it any more): the four waves of a block meet here, once per tile.  They work on 256 neighbouring
        // envs — 4 KiB of every output row — and otherwise drift apart.  With plain output stores this was worth 7-11 % for CartPoleSwingUp
        // on the slower boxes (0.287-0.294 -> 0.260-0.267 ms; nothing on the fast ones; CartPoleBalancing lost 4-5 % to the waiting).  The
        // non-temporal stores (emei_device.h:store16_stream) remove what it worked around, and on top of them the barrier COSTS 3-4 %
        // (0.2348 -> 0.2253 ms without it, 131 072 envs 0.4669 -> 0.4518): profiles/EXPERIMENTS.md.
        if constexpr (EMEI_TILE_BARRIER != 0 && Env::kTileBarrier) __builtin_amdgcn_s_barrier();
    }
    if (t0 > 0) {
        store_rew_rows(t0 - 4, rew_pend);
        store_done_rows(t0 - kStage, done_pend);
    }
    // tail (< kStage steps): direct loads and stores
    for (int t = t0; t < a.n_steps; ++t) {
        R o[4], rew;
        advance((actions + (int64_t)t * n)[li], o, rew);
        const float4 obs4 = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
        (a.obs_out + (int64_t)t * n)[li] = obs4;
        store_obs_peers(t, obs4);
        (a.reward_out + (int64_t)t * n)[li] = (float)rew;
        (a.done_out + (int64_t)t * n)[li] = (uint8_t)done;
        maybe_reset();
    }

#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[k * n + i] = s[k];
    a.steps[i] = steps;
    a.episode[i] = episode;
    unsigned long long m = __ballot(done != 0);
    if (lane == 0) a.done_mask[i / kWave] = m;
    EMEI_CLOCK_END();
#undef EMEI_LOAD_TILE
}

template <class Env, typename ActT, bool FREQ1>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(Env::kMinWavesPerEU)))
    pend_rollout_staged_kernel(const RolloutArgs<Env> a) {
    pend_rollout_staged<Env, ActT, FREQ1, false>(a, PeerObs{});
}

// ... and with the peer stores (emei_set_obs_peers; Env::kPeerWrite: the CartPole family, BASELINE configs[4]'s env)
template <class Env, typename ActT, bool FREQ1>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(Env::kMinWavesPerEU)))
    pend_rollout_staged_peers_kernel(const RolloutArgs<Env> a, const PeerObs peers) {
    pend_rollout_staged<Env, ActT, FREQ1, true>(a, peers);
}

// Env.reset on the device
template <class Env>
__global__ void __launch_bounds__(kBlock)
    pend_reset_kernel(typename Env::real* state, int32_t* steps, uint32_t* episode, int64_t n, uint64_t seed,
                      uint64_t env_offset, typename Env::Params p) {
    using R = typename Env::real;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    R s[4];
    Env::init(s, seed, env_offset + (uint64_t)i, 0u, p);
#pragma unroll
    for (int k = 0; k < 4; ++k) state[k * n + i] = s[k];
    steps[i] = 0;
    episode[i] = 0;
}

// initial observation of (env, episode) pairs under the device reset generator
template <class Env>
__global__ void __launch_bounds__(kBlock)
    pend_init_obs_kernel(const int64_t* env_index, const uint32_t* episode, float4* obs, int64_t count, uint64_t seed,
                         uint64_t env_offset, typename Env::Params p) {
    using R = typename Env::real;
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    R s[4], o[4];
    Env::init(s, seed, env_offset + (uint64_t)env_index[k], episode[k], p);
    Env::obs_of(s, o);
    obs[k] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
}

// current_obs as float64 [n,4]
template <class Env>
__global__ void __launch_bounds__(kBlock)
    pend_get_obs_kernel(const typename Env::real* state, double* obs, int64_t n) {
    using R = typename Env::real;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    R s[4], o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = state[k * n + i];
    Env::obs_of(s, o);
    double2* dst = (double2*)(obs + 4 * i);
    dst[0] = make_double2((double)o[0], (double)o[1]);
    dst[1] = make_double2((double)o[2], (double)o[3]);
}

// ---------------------------------------------------------------------------------------------
// stateless batched functions on [n,4] observations of the caller's dtype T (float or double: emei_io_dtype)
// get_batch_reward / get_batch_terminal (core.py:182-188).  float64 rows are not narrowed: the reference evaluates
// these functions on float64 arrays (cartpole.py:124-129,145-151; inverted_pendulum.py:73-183)
template <typename T>
__device__ __forceinline__ void load_row4(const T* base, int64_t i, T (&v)[4]) {
    if constexpr (sizeof(T) == 4) {
        const float4 x = ((const float4*)base)[i];
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
        const double2 x = ((const double2*)base)[2 * i], y = ((const double2*)base)[2 * i + 1];
        v[0] = x.x, v[1] = x.y, v[2] = y.x, v[3] = y.y;
    }
}
template <typename T, typename R>
__device__ __forceinline__ void store_row4(T* base, int64_t i, const R (&o)[4]) {
    if constexpr (sizeof(T) == 4) {
        ((float4*)base)[i] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
    } else {
        ((double2*)base)[2 * i] = make_double2((double)o[0], (double)o[1]);
        ((double2*)base)[2 * i + 1] = make_double2((double)o[2], (double)o[3]);
    }
}

template <class Env, typename T>
__global__ void __launch_bounds__(kBlock)
    pend_reward_terminal_kernel(const T* obs, T* reward, uint8_t* terminal, int64_t n,
                                typename Env::Params p, const SinCosEntry* trig) {
    using R = typename Env::real;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    T v[4];
    load_row4(obs, i, v);
    R o[4] = {(R)v[0], (R)v[1], (R)v[2], (R)v[3]};
    // the observation IS the state for reward/terminal purposes (wrapped angle has the same cosine);
    // build the carry from it.  For InvertedPendulum o[1] is theta, prime() adds phi_off itself.
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(o, c, p);
    if (reward) {
        // float64 rows: the reward in the working precision (the fused kernels round it to the float32 they store)
        if constexpr (sizeof(T) == 8) reward[i] = (T)Env::reward_exact(o, c, p);
        else reward[i] = (T)Env::reward(o, c, p);
    }
    if (terminal) terminal[i] = (uint8_t)Env::terminal(o, c, p);
}

// get_batch_next_obs (core.py:190-193): one step from caller-supplied observations
template <class Env, typename T>
__global__ void __launch_bounds__(kBlock)
    pend_next_obs_kernel(const T* obs, const void* actions, int action_dtype, T* next_obs, int64_t n,
                         int freq_rate, typename Env::Params p, const SinCosEntry* trig) {
    using R = typename Env::real;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    T v[4];
    load_row4(obs, i, v);
    R s[4] = {(R)v[0], (R)v[1], (R)v[2], (R)v[3]}, o[4], rew;
    bool term;
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, p);
    Env::step(s, c, Env::load_action(actions, action_dtype, i), p, freq_rate, o, rew, term);
    store_row4(next_obs, i, o);
}

// emei_evaluate_sequences (core.py:18-37,190-193: the model a planner queries): lane j scores candidate (i = j / K, k = j % K)
// of env i — `horizon` steps of actions [t, j] from env i's start state with the arithmetic of pend_rollout_kernel, the state
// in registers throughout.  ret = sum_{t < L} discount^t * (double)(float)r_t in step order (the float32 reward the rollout
// stores), L = the first terminal step + 1 (else horizon); final_obs = the float32 observation of step L - 1.  A lane keeps
// stepping after its terminal step without accumulating (as a rollout without auto-reset would); the wave leaves the loop
// once a ballot finds none of its lanes live.  Per candidate the kernel writes 12 B (16 more with final_obs), per step it
// reads one action.
// DRAWN (emei_plan_shooting): the action source is the lane itself — candidate (env_offset + i, k)'s draws under `sp`
// (emei_device.h:draw_action; ActT is then the drawn value's type, int or float, and `actions` unused), one Philox block per four
// steps for the discrete envs instead of the prefetch — and instead of 12 B per candidate the wave leaves one PlanPartial per
// (wave, env) segment (plan_reduce_wave).  The step loop is the same code either way.
// KEEP (emei_plan_mppi, with DRAWN): every lane also stores its return to ret_out[j] (8 B per candidate) for the weights of
// plan_mppi_finish_kernel; nothing else changes, and the instantiations without it are the code they were.
// Spec (emei_plan_cem with a sigma_map: CandidateSpecMap, with DRAWN and KEEP): the type draw_action reads the candidate rule from.
template <class Env, typename ActT, bool DRAWN = false, bool KEEP = false, class Spec = CandidateSpec>
__global__ void __launch_bounds__(kBlock)
    pend_plan_kernel(const typename Env::real* state, const double* start_rows, const ActT* actions, int64_t n_envs, int32_t n_cand,
                     int32_t horizon, double discount, int freq_rate, typename Env::Params p, const SinCosEntry* trig,
                     double* ret_out, int32_t* len_out, float4* final_obs, Spec sp, PlanPartial* partials) {
    using R = typename Env::real;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t nk = n_envs * n_cand;
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nk) return;
    const int64_t i = j / n_cand;
    R s[4];
    // start state: the handle's SoA, or the caller's float64 rows narrowed as emei_set_state narrows them (util_kernels.hip)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = start_rows ? (R)start_rows[i * 4 + k] : state[k * n_envs + i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, p);

    double ret = 0.0, g = 1.0;
    int32_t len = horizon;
    bool live = true;
    float4 fo = make_float4(0.f, 0.f, 0.f, 0.f);
    // actions a chunk ahead of their use, as in pend_rollout_kernel (steps past the horizon clamped, not branched around)
    constexpr int kChunk = 8;
    const int last = horizon - 1;
    ActT cur[kChunk], nxt[kChunk];
    CandidateWordsT<true> cw(sp.seed, sp.env_offset + (uint64_t)i, (uint32_t)(j - i * n_cand));
    if constexpr (!DRAWN) {
#pragma unroll
        for (int u = 0; u < kChunk; ++u) cur[u] = (actions + (int64_t)min(u, last) * nk)[j];
    }
    bool any_live = true;
    for (int t0 = 0; t0 < horizon && any_live; t0 += kChunk) {
        if constexpr (!DRAWN) {
#pragma unroll
            for (int u = 0; u < kChunk; ++u) nxt[u] = (actions + (int64_t)min(t0 + kChunk + u, last) * nk)[j];
        }
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            const int t = t0 + u;
            if (t >= horizon) break;
            R o[4], rew;
            bool term;
            if constexpr (DRAWN) cur[u] = (ActT)draw_action(cw, sp, n_envs, i, t, 0, Env::kDiscrete ? 0 : Env::kActDim);
            Env::step(s, c, Env::decode_t(cur[u]), p, freq_rate, o, rew, term);
            if (live) {
                ret = ret + g * (double)(float)rew;
                g = g * discount;
                fo = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
                if (term) live = false, len = t + 1;
            }
            if (__ballot(live) == 0ull) {  // wave-uniform
                any_live = false;
                break;
            }
        }
        if constexpr (!DRAWN) {
#pragma unroll
            for (int u = 0; u < kChunk; ++u) cur[u] = nxt[u];
        }
    }
    if constexpr (DRAWN) {
        if constexpr (KEEP) ret_out[j] = ret;  // j < nk here
        plan_reduce_wave(j, nk, i, n_cand, ret, len, partials);
    } else {
        ret_out[j] = ret;
        len_out[j] = len;
        if (final_obs) final_obs[j] = fo;
    }
}

// emei_evaluate_policies (the normative text: include/emei_hip.h): pend_plan_kernel's non-DRAWN loop with the action load replaced
// by the lane's own evaluation of ITS policy on the float32 row it holds, as pend_policy_rollout_kernel evaluates the one policy.
// One lane per (policy, env) pair and a block never mixes policies: with env_blocks = ceil(n_envs / kBlock), block b serves policy
// p = b / env_blocks and env block b % env_blocks (env blocks fastest: neighbouring blocks read the same weights).  p comes from
// blockIdx alone, so the offset weight bases stay wave-uniform and policy_eval (unchanged) keeps reading them as scalar loads.
// Nothing is read or written per step; a lane's 12 B (28 with final_obs) leave at its last counted step, at [p * n_envs + i].
template <class Env>
__global__ void __launch_bounds__(kBlock)
    pend_policy_eval_kernel(const typename Env::real* state, const double* start_rows, int64_t n_envs, uint32_t env_blocks,
                            int32_t horizon, double discount, int freq_rate, typename Env::Params p, const SinCosEntry* trig,
                            const PolicyArgs stacked, double* ret_out, int32_t* len_out, float4* final_obs) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, trig, Env::trig_rot_c(), Env::trig_rot_s());
    const uint32_t pi = blockIdx.x / env_blocks;  // the block's policy: scalar
    const int64_t i = (int64_t)(blockIdx.x - pi * env_blocks) * kBlock + threadIdx.x;
    if (i >= n_envs) return;
    const int64_t j = (int64_t)pi * n_envs + i;
    PolicyArgs pol = stacked;  // member pi of the population: n_out = 1, fan-in of the output layer = hidden, or 4 without one
    pol.w1 += (int64_t)pi * pol.hidden * 4, pol.b1 += (int64_t)pi * pol.hidden;
    pol.w2 += (int64_t)pi * (pol.hidden > 0 ? pol.hidden : 4), pol.b2 += pi;

    R s[4];
    // start state: the handle's SoA, or the caller's float64 rows narrowed as emei_set_state narrows them (util_kernels.hip)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = start_rows ? (R)start_rows[i * 4 + k] : state[k * n_envs + i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, p);
    float x[4];
    {
        R o[4];
        Env::obs_of(s, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
    }
    double ret = 0.0, g = 1.0;
    bool live = true;
    for (int t = 0; t < horizon; ++t) {
        float av[1];
        policy_eval<4, 1, Env::kDiscrete>(pol, x, av);
        R o[4], rew;
        bool term;
        Env::step(s, c, Env::decode_t((DrawT)av[0]), p, freq_rate, o, rew, term);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
        if (live) {
            ret = ret + g * (double)(float)rew;
            g = g * discount;
            if (term || t == horizon - 1) {  // the lane's last counted step
                live = false;
                ret_out[j] = ret;
                if (len_out) len_out[j] = t + 1;
                if (final_obs) final_obs[j] = make_float4(x[0], x[1], x[2], x[3]);
            }
        }
        if (__ballot(live) == 0ull) break;  // wave-uniform
    }
}

// emei_plan_policy (the normative text: include/emei_hip.h): pend_plan_kernel's DRAWN + KEEP loop — one lane per candidate
// (i = j / K, k = j % K), every return kept in ret_out[j], one PlanPartial per (wave, env) segment through plan_reduce_wave — with the
// drawn action replaced by the lane's evaluation of THE policy on the float32 row it holds, as pend_policy_rollout_noisy_kernel
// evaluates it: the noise of step t under the key nz.seed + t, with the lane's k in the counter word, and none at all for k = 0.
// Every lane reads the same network, so the weights stay wave-uniform scalar loads.  The lane also leaves its action of step 0 in
// first_out[j] (4 B per candidate) for plan_policy_finish_kernel; nothing else is read or written per step.
template <class Env>
__global__ void __launch_bounds__(kBlock)
    pend_policy_plan_kernel(const typename Env::real* state, const double* start_rows, int64_t n_envs, int32_t n_cand, int32_t horizon,
                            double discount, int freq_rate, typename Env::Params p, const SinCosEntry* trig, const PolicyArgs pol,
                            const PolicyNoiseArgs nz, uint64_t env_offset, double* ret_out, float* first_out, PlanPartial* partials) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t nk = n_envs * n_cand;
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nk) return;
    const int64_t i = j / n_cand;
    const uint32_t k = (uint32_t)(j - i * n_cand);
    R s[4];
    // start state: the handle's SoA, or the caller's float64 rows narrowed as emei_set_state narrows them (util_kernels.hip)
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = start_rows ? (R)start_rows[i * 4 + q] : state[q * n_envs + i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, p);
    float x[4];
    {
        R o[4];
        Env::obs_of(s, o);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = (float)o[q];
    }
    double ret = 0.0, g = 1.0;
    int32_t len = horizon;
    bool live = true;
    for (int t = 0; t < horizon; ++t) {
        float av[1];
        policy_eval_t<4, 1, Env::kDiscrete, true>(pol, nz, nz.seed + (uint64_t)t, env_offset + (uint64_t)i, x, av, k, k != 0u);
        if (t == 0) first_out[j] = av[0];
        R o[4], rew;
        bool term;
        Env::step(s, c, Env::decode_t((DrawT)av[0]), p, freq_rate, o, rew, term);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = (float)o[q];
        if (live) {
            ret = ret + g * (double)(float)rew;
            g = g * discount;
            if (term) live = false, len = t + 1;
        }
        if (__ballot(live) == 0ull) break;  // wave-uniform
    }
    ret_out[j] = ret;  // j < nk here
    plan_reduce_wave(j, nk, i, n_cand, ret, len, partials);
}

// emei_evaluate_policies_deep: pend_policy_eval_kernel's loop under the network with two hidden layers, as ONE-WAVE blocks (the
// block's dynamic LDS is the wave's h1 tile): with env_waves = ceil(n_envs / 64), block b serves policy p = b / env_waves and env
// wave b % env_waves, so p is still scalar and member p's offset weight bases stay wave-uniform.
template <class Env>
__global__ void __launch_bounds__(kWave)
    pend_policy_eval_deep_kernel(const typename Env::real* state, const double* start_rows, int64_t n_envs, uint32_t env_waves,
                                 int32_t horizon, double discount, int freq_rate, typename Env::Params p, const SinCosEntry* trig,
                                 const PolicyDeepArgs stacked, double* ret_out, int32_t* len_out, float4* final_obs) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    extern __shared__ __attribute__((aligned(16))) float4 deep_h1_s[];
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table<kWave>(trig_s, trig, Env::trig_rot_c(), Env::trig_rot_s());
    const uint32_t pi = blockIdx.x / env_waves;  // the block's policy: scalar
    const int64_t i = (int64_t)(blockIdx.x - pi * env_waves) * kWave + threadIdx.x;
    if (i >= n_envs) return;
    const int64_t j = (int64_t)pi * n_envs + i;
    PolicyDeepArgs pol = stacked;  // member pi of the population: n_out = 1
    pol.w1 += (int64_t)pi * pol.hidden1 * 4, pol.b1 += (int64_t)pi * pol.hidden1;
    pol.w2 += (int64_t)pi * pol.hidden2 * pol.hidden1, pol.b2 += (int64_t)pi * pol.hidden2;
    pol.w3 += (int64_t)pi * pol.hidden2, pol.b3 += pi;
    const PolicyNoiseArgs none{};  // pol.noisy == 0: never read

    R s[4];
    // start state: the handle's SoA, or the caller's float64 rows narrowed as emei_set_state narrows them (util_kernels.hip)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = start_rows ? (R)start_rows[i * 4 + k] : state[k * n_envs + i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, p);
    float x[4];
    {
        R o[4];
        Env::obs_of(s, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
    }
    double ret = 0.0, g = 1.0;
    bool live = true;
    for (int t = 0; t < horizon; ++t) {
        float av[1];
        policy_eval_deep_t<4, 1, Env::kDiscrete>(pol, none, 0, 0, x, av, deep_h1_s, (int)threadIdx.x);
        R o[4], rew;
        bool term;
        Env::step(s, c, Env::decode_t((DrawT)av[0]), p, freq_rate, o, rew, term);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)o[k];
        if (live) {
            ret = ret + g * (double)(float)rew;
            g = g * discount;
            if (term || t == horizon - 1) {  // the lane's last counted step
                live = false;
                ret_out[j] = ret;
                if (len_out) len_out[j] = t + 1;
                if (final_obs) final_obs[j] = make_float4(x[0], x[1], x[2], x[3]);
            }
        }
        if (__ballot(live) == 0ull) break;  // wave-uniform
    }
}

// emei_plan_policy_deep (the normative text: include/emei_hip.h): pend_policy_plan_kernel's loop under the network with two hidden
// layers, as ONE-WAVE blocks (the block's dynamic LDS is the wave's h1 tile, sized by the wider first layer of `pol` and `val`): lane
// l of block b holds candidate j = 64 b + l, so plan_reduce_wave's slot (j >> 6) + i is the one the 256-thread kernel writes.
// Terminal value (val.w1 non-null, wave-uniform): `live` falls only at a terminal bit here, so after the loop it says "never
// terminated"; the loop leaves early only once no lane is live, and otherwise every lane has stepped to x_H — the wave then
// evaluates `val` in the same tile on the rows it holds, raw (no output clause), and the live lanes take ret + g_H * (double)v by a
// select.
template <class Env>
__global__ void __launch_bounds__(kWave)
    pend_policy_plan_deep_kernel(const typename Env::real* state, const double* start_rows, int64_t n_envs, int32_t n_cand,
                                 int32_t horizon, double discount, int freq_rate, typename Env::Params p, const SinCosEntry* trig,
                                 const PolicyDeepArgs pol, const PolicyNoiseArgs nz, const PolicyDeepArgs val, uint64_t env_offset,
                                 double* ret_out, float* first_out, PlanPartial* partials) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    extern __shared__ __attribute__((aligned(16))) float4 deep_h1_s[];
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table<kWave>(trig_s, trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t nk = n_envs * n_cand;
    const int64_t j = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (j >= nk) return;
    const int64_t i = j / n_cand;
    const uint32_t k = (uint32_t)(j - i * n_cand);
    R s[4];
    // start state: the handle's SoA, or the caller's float64 rows narrowed as emei_set_state narrows them (util_kernels.hip)
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = start_rows ? (R)start_rows[i * 4 + q] : state[q * n_envs + i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, p);
    float x[4];
    {
        R o[4];
        Env::obs_of(s, o);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = (float)o[q];
    }
    double ret = 0.0, g = 1.0;
    int32_t len = horizon;
    bool live = true;
    for (int t = 0; t < horizon; ++t) {
        float av[1];
        policy_eval_deep_t<4, 1, Env::kDiscrete>(pol, nz, nz.seed + (uint64_t)t, env_offset + (uint64_t)i, x, av, deep_h1_s,
                                                 (int)threadIdx.x, k, k != 0u);
        if (t == 0) first_out[j] = av[0];
        R o[4], rew;
        bool term;
        Env::step(s, c, Env::decode_t((DrawT)av[0]), p, freq_rate, o, rew, term);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = (float)o[q];
        if (live) {
            ret = ret + g * (double)(float)rew;
            g = g * discount;
            if (term) live = false, len = t + 1;
        }
        if (__ballot(live) == 0ull) break;  // wave-uniform
    }
    if (val.w1 && __ballot(live) != 0ull) {  // wave-uniform: some lane never terminated, so every lane holds its x_H
        float v[1];
        policy_eval_deep_t<4, 1, false, true>(val, nz, 0, 0, x, v, deep_h1_s, (int)threadIdx.x);  // val.noisy == 0: nz is never read
        const double tail = g * (double)v[0];  // rounded to float64, then added
        const double boot = ret + tail;
        ret = live ? boot : ret;
    }
    ret_out[j] = ret;  // j < nk here
    plan_reduce_wave(j, nk, i, n_cand, ret, len, partials);
}

// emei_evaluate_sequences_value / emei_plan_shooting_value / emei_plan_mppi_value / emei_plan_cem_value (the normative text:
// include/emei_hip.h): pend_plan_kernel's loop, expression for expression, as ONE-WAVE blocks whose dynamic LDS is the wave's h1 tile
// of the value network — lane l of block b holds candidate j = 64 b + l, so the waves and plan_reduce_wave's slots are those of the
// 256-thread kernel.  DRAWN here is pend_plan_kernel's DRAWN + KEEP (the shooting call keeps its returns too: one instantiation).
// Terminal value: `live` falls only at a terminal bit, so after the loop it says "never terminated"; the loop leaves early only once
// no lane is live, and a live lane's `fo`, refreshed at every step it counted, is x_H — the wave then evaluates `val` on the rows it
// holds, raw (no output clause), and the live lanes take ret + g_H * (double)v by a select, as pend_policy_plan_deep_kernel's do.
// len and final_obs are what pend_plan_kernel leaves.
template <class Env, typename ActT, bool DRAWN = false, class Spec = CandidateSpec>
__global__ void __launch_bounds__(kWave)
    pend_plan_value_kernel(const typename Env::real* state, const double* start_rows, const ActT* actions, int64_t n_envs, int32_t n_cand,
                           int32_t horizon, double discount, int freq_rate, typename Env::Params p, const SinCosEntry* trig,
                           const PolicyDeepArgs val, double* ret_out, int32_t* len_out, float4* final_obs, Spec sp, PlanPartial* partials) {
    using R = typename Env::real;
    extern __shared__ __attribute__((aligned(16))) float4 deep_h1_s[];
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table<kWave>(trig_s, trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int64_t nk = n_envs * n_cand;
    const int64_t j = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (j >= nk) return;
    const int64_t i = j / n_cand;
    R s[4];
    // start state: the handle's SoA, or the caller's float64 rows narrowed as emei_set_state narrows them (util_kernels.hip)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = start_rows ? (R)start_rows[i * 4 + k] : state[k * n_envs + i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    Env::prime(s, c, p);

    double ret = 0.0, g = 1.0;
    int32_t len = horizon;
    bool live = true;
    float4 fo = make_float4(0.f, 0.f, 0.f, 0.f);
    // actions a chunk ahead of their use, as in pend_rollout_kernel (steps past the horizon clamped, not branched around)
    constexpr int kChunk = 8;
    const int last = horizon - 1;
    ActT cur[kChunk], nxt[kChunk];
    CandidateWordsT<true> cw(sp.seed, sp.env_offset + (uint64_t)i, (uint32_t)(j - i * n_cand));
    if constexpr (!DRAWN) {
#pragma unroll
        for (int u = 0; u < kChunk; ++u) cur[u] = (actions + (int64_t)min(u, last) * nk)[j];
    }
    bool any_live = true;
    for (int t0 = 0; t0 < horizon && any_live; t0 += kChunk) {
        if constexpr (!DRAWN) {
#pragma unroll
            for (int u = 0; u < kChunk; ++u) nxt[u] = (actions + (int64_t)min(t0 + kChunk + u, last) * nk)[j];
        }
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            const int t = t0 + u;
            if (t >= horizon) break;
            R o[4], rew;
            bool term;
            if constexpr (DRAWN) cur[u] = (ActT)draw_action(cw, sp, n_envs, i, t, 0, Env::kDiscrete ? 0 : Env::kActDim);
            Env::step(s, c, Env::decode_t(cur[u]), p, freq_rate, o, rew, term);
            if (live) {
                ret = ret + g * (double)(float)rew;
                g = g * discount;
                fo = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
                if (term) live = false, len = t + 1;
            }
            if (__ballot(live) == 0ull) {  // wave-uniform
                any_live = false;
                break;
            }
        }
        if constexpr (!DRAWN) {
#pragma unroll
            for (int u = 0; u < kChunk; ++u) cur[u] = nxt[u];
        }
    }
    if (__ballot(live) != 0ull) {  // wave-uniform: some lane never terminated, so the loop ran all `horizon` steps
        const float x[4] = {fo.x, fo.y, fo.z, fo.w};  // a live lane's: x_H
        const PolicyNoiseArgs none{};                 // val.noisy == 0: never read
        float v[1];
        policy_eval_deep_t<4, 1, false, true>(val, none, 0, 0, x, v, deep_h1_s, (int)threadIdx.x);
        const double tail = g * (double)v[0];  // rounded to float64, then added
        const double boot = ret + tail;
        ret = live ? boot : ret;
    }
    ret_out[j] = ret;  // j < nk here
    if constexpr (DRAWN) {
        plan_reduce_wave(j, nk, i, n_cand, ret, len, partials);
    } else {
        len_out[j] = len;
        if (final_obs) final_obs[j] = fo;
    }
}

// ---------------------------------------------------------------------------------------------
// emei_mpc_mppi: receding-horizon MPPI control episodes in ONE launch (the normative text: include/emei_hip.h).
// The draws read the nominal from the wave's LDS slice: CandidateSpecLds (emei_device.h, shared with the body kernels' controllers).

template <class Env>
struct MpcArgs {
    typename Env::real* state;  // SoA: 4 arrays of n
    int32_t* steps;
    uint32_t* episode;
    const SinCosEntry* trig;
    float* nominal;  // in/out [horizon, n(, act_dim)]
    double* work;    // [n, n_cand] returns, then weights; word 0 of env i's row ends as its last done code (mpc_done_pack_kernel)
    void* actions_out;
    float4* obs_out;
    float* reward_out;
    uint8_t* done_out;
    double* plan_return_out;
    double* ess_out;
    int64_t n;
    int32_t n_steps, horizon, n_cand, freq_rate, action_dtype, max_episode_steps;
    uint32_t flags;
    uint64_t reset_seed, env_offset, seed;
    double discount, temperature;
    float sigma, lo, hi, refill, nominal_lo, nominal_hi;
    typename Env::Params p;
};

// One WAVE per env, for all n_steps control steps; lane l owns the candidates k = l, l + 64, ... (plan_mppi_finish_kernel's layout,
// so the summation tree is that kernel's by construction).  Per control step:
//   1. the lanes clamp the nominal (the wave's LDS slice);
//   2. every lane scores its candidates with pend_plan_kernel's DRAWN loop from the register copy of the env's real state
//      (ret = ret + g * (double)(float)rew in step order; the wave leaves a pass once a ballot finds no lane live), keeps the
//      return in `work` (8 B per candidate: no cap on n_candidates; a lane reads back only what it wrote) and folds (k*, r*) in
//      ascending k, then over the lanes — the planner's order is total, so this is plan_finish_kernel's winner;
//   3. weights, Z, the effective sample size and the weighted mean are plan_mppi_finish_kernel's lines, copied rather than shared
//      (that kernel's comment: it must not be rescheduled); lane 0 writes the new nominal into LDS;
//   4. the first entry is the action; the real state — wave-uniform values in registers, computed redundantly by every lane —
//      takes emei_step's step (the carry primed from the state, as a launch of its own would), TimeLimit and auto-reset as
//      pend_rollout_kernel; lane 0 stores the step's outputs.  Those stores are small and uncoalesced, which is accepted: this
//      path is bound by the latency of one wave's dependent arithmetic, not by HBM;
//   5. the nominal is shifted (or refilled after a reset).
// The nominal is read from global memory once and written back once.  stage_trig_table's block barrier is taken by every wave,
// also by those past n; after it the waves of a block run different trip counts, so there is NO block barrier: what lane 0
// writes into LDS reaches the other lanes through wave_lds_fence().
template <class Env>
__global__ void __launch_bounds__(kBlock) pend_mpc_mppi_kernel(const MpcArgs<Env> a) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    constexpr int kWavesPerBlock = kBlock / kWave;
    constexpr int na = Env::kActDim;                          // components per step of the nominal
    constexpr int act_dim = Env::kDiscrete ? 0 : Env::kActDim;  // draw_action's: 0 = coin flips
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    __shared__ float nom_s[kWavesPerBlock][EMEI_MPC_MAX_HORIZON * na];
    stage_trig_table(trig_s, a.trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wv;  // wave-uniform
    if (i >= a.n) return;
    const int64_t n = a.n;
    const int32_t n_cand = a.n_cand, horizon = a.horizon;
    const int32_t n_comp = horizon * na;  // <= EMEI_MPC_MAX_HORIZON * na (abi.hip)
    float* nom = nom_s[wv];
    for (int32_t c = lane; c < n_comp; c += kWave) nom[c] = a.nominal[((int64_t)(c / na) * n + i) * na + c % na];

    R s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = a.state[k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    const bool auto_reset = (a.flags & EMEI_FLAG_AUTO_RESET) != 0;
    const uint64_t g = a.env_offset + (uint64_t)i;
    double* wt = a.work + i * n_cand;
    CandidateSpecLds sp;
    sp.env_offset = a.env_offset;
    sp.nominal.p = (const __attribute__((address_space(3))) float*)nom;
    sp.sigma = a.sigma, sp.lo = a.lo, sp.hi = a.hi;
    uint32_t done = 0;

    for (int32_t t = 0; t < a.n_steps; ++t) {
        // 1.
        for (int32_t cc = lane; cc < n_comp; cc += kWave) nom[cc] = fminf(fmaxf(nom[cc], a.nominal_lo), a.nominal_hi);
        wave_lds_fence();
        // 2.
        sp.seed = a.seed + (uint64_t)t;
        Env::prime(s, c, a.p);
        double rs = __builtin_nan("");  // (NaN, INT32_MAX) loses to every candidate
        int32_t ks = INT32_MAX;
        for (int32_t k0 = 0; k0 < n_cand; k0 += kWave) {  // wave-uniform trip count: every lane takes part in the ballot
            const int32_t k = k0 + lane;
            R cs[4] = {s[0], s[1], s[2], s[3]};
            typename Env::Carry cc = c;
            CandidateWordsT<true> cw(sp.seed, g, (uint32_t)k);
            double ret = 0.0, gd = 1.0;
            bool live = k < n_cand;
            for (int32_t h = 0; h < horizon; ++h) {
                R o[4], rew;
                bool term;
                const DrawT act = (DrawT)draw_action(cw, sp, 1, 0, h, 0, act_dim);
                Env::step(cs, cc, Env::decode_t(act), a.p, a.freq_rate, o, rew, term);
                if (live) {
                    ret = ret + gd * (double)(float)rew;
                    gd = gd * a.discount;
                    if (term) live = false;
                }
                if (__ballot(live) == 0ull) break;  // wave-uniform
            }
            if (k < n_cand) {
                wt[k] = ret;
                if (plan_replaces(rs, ks, ret, k)) rs = ret, ks = k;
            }
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const double r2 = __shfl_xor(rs, d, kWave);
            const int32_t k2 = __shfl_xor(ks, d, kWave);
            if (plan_replaces(rs, ks, r2, k2)) rs = r2, ks = k2;
        }
        // 3.
        double z = 0.0, z2 = 0.0;
        for (int32_t k = lane; k < n_cand; k += kWave) {
            const double r = wt[k];
            const double e = exp((r - rs) / a.temperature);  // r < r*: the argument is negative, -inf included
            const double w = rs != rs ? 1.0 : (r != r ? 0.0 : (r == rs ? 1.0 : e));
            wt[k] = w;
            z += w, z2 += w * w;
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) z += __shfl_xor(z, d, kWave);
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) z2 += __shfl_xor(z2, d, kWave);
        if (lane == 0) {
            if (a.plan_return_out) a.plan_return_out[(int64_t)t * n + i] = rs;
            if (a.ess_out) a.ess_out[(int64_t)t * n + i] = z * z / z2;
        }
        for (int32_t c0 = 0; c0 < n_comp; c0 += 4) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int32_t k = lane; k < n_cand; k += kWave) {
                const double w = wt[k];
                CandidateWordsT<true> cw(sp.seed, g, (uint32_t)k);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int32_t cc = min(c0 + u, n_comp - 1);  // past the end: the last component again, dropped below
                    const float v = draw_action(cw, sp, 1, 0, cc / na, cc % na, act_dim);
                    acc[u] += w * (double)v;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) acc[u] += __shfl_xor(acc[u], d, kWave);
            }
            wave_lds_fence();  // every lane's draws of this block have read the entries lane 0 now replaces
            if (lane == 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int32_t cc = c0 + u;
                    if (cc < n_comp) nom[cc] = (float)(acc[u] / z);
                }
            }
        }
        wave_lds_fence();  // lane 0's nominal is what every lane reads from here on
        // 4.
        float av[na];
#pragma unroll
        for (int q = 0; q < na; ++q) {
            av[q] = nom[q];
            if constexpr (Env::kDiscrete) av[q] = av[q] >= 0.5f ? 1.f : 0.f;
            if (lane == 0) store_action(a.actions_out, a.action_dtype, ((int64_t)t * n + i) * na + q, av[q]);
        }
        {
            R o[4], rew;
            bool term;
            Env::step(s, c, Env::decode_t((DrawT)av[0]), a.p, a.freq_rate, o, rew, term);
            ++steps;
            const bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
            done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
            if (lane == 0) {
                const int64_t at = (int64_t)t * n + i;
                if (a.obs_out) a.obs_out[at] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
                if (a.reward_out) a.reward_out[at] = (float)rew;
                if (a.done_out) a.done_out[at] = (uint8_t)done;
            }
        }
        const bool reset_now = auto_reset && __builtin_amdgcn_readfirstlane(done) != 0u;  // wave-uniform
        if (reset_now) {
            ++episode;
            steps = 0;
            Env::init(s, a.reset_seed, g, episode, a.p);
        }
        // 5. pass by pass in ascending order: a pass reads [base + na, base + 64 + na) and writes [base, base + 64)
        for (int32_t base = 0; base < n_comp; base += kWave) {
            const int32_t cc = base + lane;
            const float v = (!reset_now && cc + na < n_comp) ? nom[cc + na] : a.refill;
            wave_lds_fence();
            if (cc < n_comp) nom[cc] = v;
            wave_lds_fence();
        }
    }

    for (int32_t cc = lane; cc < n_comp; cc += kWave) a.nominal[((int64_t)(cc / na) * n + i) * na + cc % na] = nom[cc];
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.state[k * n + i] = s[k];
        a.steps[i] = steps;
        a.episode[i] = episode;
        ((unsigned long long*)wt)[0] = (unsigned long long)done;  // lane 0's own slot, after its last use
    }
}

// ---------------------------------------------------------------------------------------------
// emei_mpc_policy: policy-guided control episodes in ONE launch (the normative text: include/emei_hip.h).  There is no nominal: the
// policy is the warm start, so the kernel keeps nothing in LDS beyond the trig table and the horizon has no cap.

template <class Env>
struct MpcPolicyArgs {
    typename Env::real* state;  // SoA: 4 arrays of n
    int32_t* steps;
    uint32_t* episode;
    const SinCosEntry* trig;
    double* work;  // [n, n_cand] returns, then [n, n_cand] float32 first actions; word 0 of env i's row of returns ends as its last
                   // done code (mpc_done_pack_kernel)
    void* actions_out;
    float4* obs_out;
    float* reward_out;
    uint8_t* done_out;
    double* plan_return_out;
    int32_t* plan_index_out;
    double* ess_out;
    int64_t n;
    int32_t n_steps, horizon, n_cand, freq_rate, action_dtype, max_episode_steps, act_mode;
    uint32_t flags;
    uint64_t reset_seed, env_offset, seed_stride;
    double discount, temperature;
    typename Env::Params p;
};

// pend_mpc_mppi_kernel's skeleton — one WAVE per env for all n_steps control steps, lane l owning the candidates k = l, l + 64, ..., the
// real state and its counters wave-uniform values in registers — around emei_plan_policy.  Per control step t, under the key
// key_t = nz.seed + t * seed_stride:
//   1. the carry is primed from the state and x_0 is its float32 observation (pend_policy_plan_kernel's start);
//   2. every lane scores its candidates with pend_policy_plan_kernel's loop, expression for expression: the policy on the row the
//      lane holds under the key key_t + h with the lane's k in the counter word, no noise for k = 0, the weights wave-uniform scalar
//      loads; ret = ret + g * (double)(float)rew in step order; the wave leaves a pass once a ballot finds no lane live (padding
//      lanes k >= n_cand take part and are never live).  The lane keeps its return (8 B) and its action of step 0 (4 B) in `work`
//      — a lane reads back only what it wrote — and folds (k*, r*, a*) in ascending k, then over the lanes: the planner's order is
//      total, so this is plan_policy_finish_kernel's winner and its best_action;
//   3. with ACT_MEAN or an ess_out (wave-uniform): Z, sum w^2, the weighted sum of the first actions and the quotient are
//      plan_policy_finish_kernel<true>'s lines, copied rather than shared (that kernel's instruction stream stays what it is);
//   4. the action — the winner's, or the mean (discrete envs: mean >= 0.5f) — then pend_mpc_mppi_kernel's step 4: emei_step's step
//      on the real state, TimeLimit and auto-reset; lane 0 stores the step's outputs.
// stage_trig_table's block barrier is taken by every wave, also by those past n; after it there is NO block barrier.
template <class Env>
__global__ void __launch_bounds__(kBlock) pend_mpc_policy_kernel(const MpcPolicyArgs<Env> a, const PolicyArgs pol, const PolicyNoiseArgs nz) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    static_assert(Env::kActDim == 1, "one float32 first-action slot per candidate (abi.hip sizes the workspace)");
    constexpr int kWavesPerBlock = kBlock / kWave;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, a.trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wv;  // wave-uniform
    if (i >= a.n) return;
    const int64_t n = a.n;
    const int32_t n_cand = a.n_cand, horizon = a.horizon;

    R s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = a.state[k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    const bool auto_reset = (a.flags & EMEI_FLAG_AUTO_RESET) != 0;
    const bool weighted = a.act_mode == EMEI_MPC_POLICY_ACT_MEAN || a.ess_out != nullptr;  // wave-uniform
    const uint64_t g = a.env_offset + (uint64_t)i;
    double* wt = a.work + i * n_cand;
    float* fa = (float*)(a.work + n * n_cand) + i * n_cand;  // the env's first actions
    uint32_t done = 0;

    for (int32_t t = 0; t < a.n_steps; ++t) {
        // 1.
        const uint64_t key_t = nz.seed + (uint64_t)t * a.seed_stride;
        Env::prime(s, c, a.p);
        float x0[4];
        {
            R o[4];
            Env::obs_of(s, o);
#pragma unroll
            for (int q = 0; q < 4; ++q) x0[q] = (float)o[q];
        }
        // 2.
        double rs = __builtin_nan("");  // (NaN, INT32_MAX) loses to every candidate
        int32_t ks = INT32_MAX;
        float as = 0.f;
        for (int32_t k0 = 0; k0 < n_cand; k0 += kWave) {  // wave-uniform trip count: every lane takes part in the ballot
            const int32_t k = k0 + lane;
            R cs[4] = {s[0], s[1], s[2], s[3]};
            typename Env::Carry cc = c;
            float x[4] = {x0[0], x0[1], x0[2], x0[3]};
            double ret = 0.0, gd = 1.0;
            float first = 0.f;
            bool live = k < n_cand;
            for (int32_t h = 0; h < horizon; ++h) {
                float av[1];
                policy_eval_t<4, 1, Env::kDiscrete, true>(pol, nz, key_t + (uint64_t)h, g, x, av, (uint32_t)k, k != 0);
                if (h == 0) first = av[0];
                R o[4], rew;
                bool term;
                Env::step(cs, cc, Env::decode_t((DrawT)av[0]), a.p, a.freq_rate, o, rew, term);
#pragma unroll
                for (int q = 0; q < 4; ++q) x[q] = (float)o[q];
                if (live) {
                    ret = ret + gd * (double)(float)rew;
                    gd = gd * a.discount;
                    if (term) live = false;
                }
                if (__ballot(live) == 0ull) break;  // wave-uniform
            }
            if (k < n_cand) {
                wt[k] = ret;
                fa[k] = first;
                if (plan_replaces(rs, ks, ret, k)) rs = ret, ks = k, as = first;
            }
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const double r2 = __shfl_xor(rs, d, kWave);
            const int32_t k2 = __shfl_xor(ks, d, kWave);
            const float a2 = __shfl_xor(as, d, kWave);
            if (plan_replaces(rs, ks, r2, k2)) rs = r2, ks = k2, as = a2;
        }
        // 3.
        float mean = 0.f;
        if (weighted) {
            double z = 0.0, z2 = 0.0, acc = 0.0;
            for (int32_t k = lane; k < n_cand; k += kWave) {
                const double r = wt[k];
                const double e = exp((r - rs) / a.temperature);  // r < r*: the argument is negative, -inf included
                const double w = rs != rs ? 1.0 : (r != r ? 0.0 : (r == rs ? 1.0 : e));
                z += w, z2 += w * w;
                acc += w * (double)fa[k];
            }
            z = wave_sum_all(z), z2 = wave_sum_all(z2);  // Z >= 1: candidate k* has weight 1
            const double sum = wave_sum_all(acc);
            mean = (float)(sum / z);
            if (lane == 0 && a.ess_out) a.ess_out[(int64_t)t * n + i] = z * z / z2;
        }
        if (lane == 0) {
            if (a.plan_return_out) a.plan_return_out[(int64_t)t * n + i] = rs;
            if (a.plan_index_out) a.plan_index_out[(int64_t)t * n + i] = ks;
        }
        // 4.
        float av = as;
        if (a.act_mode == EMEI_MPC_POLICY_ACT_MEAN) {  // wave-uniform
            av = mean;
            if constexpr (Env::kDiscrete) av = av >= 0.5f ? 1.f : 0.f;
        }
        if (lane == 0) store_action(a.actions_out, a.action_dtype, (int64_t)t * n + i, av);
        {
            R o[4], rew;
            bool term;
            Env::step(s, c, Env::decode_t((DrawT)av), a.p, a.freq_rate, o, rew, term);
            ++steps;
            const bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
            done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
            if (lane == 0) {
                const int64_t at = (int64_t)t * n + i;
                if (a.obs_out) a.obs_out[at] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
                if (a.reward_out) a.reward_out[at] = (float)rew;
                if (a.done_out) a.done_out[at] = (uint8_t)done;
            }
        }
        const bool reset_now = auto_reset && __builtin_amdgcn_readfirstlane(done) != 0u;  // wave-uniform
        if (reset_now) {
            ++episode;
            steps = 0;
            Env::init(s, a.reset_seed, g, episode, a.p);
        }
    }

    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.state[k * n + i] = s[k];
        a.steps[i] = steps;
        a.episode[i] = episode;
        ((unsigned long long*)wt)[0] = (unsigned long long)done;  // lane 0's own slot, after its last use
    }
}

// ---------------------------------------------------------------------------------------------
// emei_mpc_cem: receding-horizon CEM control episodes in ONE launch (the normative text: include/emei_hip.h).
// The draws of the continuous envs read the mean AND the sigma from LDS: CandidateSpecLdsMap (emei_device.h); the discrete ones keep
// CandidateSpecLds: the sigma-map path of draw_action has no coin-flip branch.

template <class Env>
struct MpcCemArgs {
    typename Env::real* state;  // SoA: 4 arrays of n
    int32_t* steps;
    uint32_t* episode;
    const SinCosEntry* trig;
    float* nominal;  // in/out [horizon, n(, act_dim)]
    double* work;    // [n, n_cand] returns, then membership flags; word 0 of env i's row ends as its last done code (mpc_done_pack_kernel)
    void* actions_out;
    float4* obs_out;
    float* reward_out;
    uint8_t* done_out;
    double* plan_return_out;
    double* elite_return_out;
    int64_t n;
    int32_t n_steps, horizon, n_cand, n_elites, iterations, freq_rate, action_dtype, max_episode_steps;
    uint32_t flags;
    uint64_t reset_seed, env_offset, seed;
    double discount;
    float sigma, sigma_min, lo, hi, refill, nominal_lo, nominal_hi;
    typename Env::Params p;
};

// pend_mpc_mppi_kernel's layout — one WAVE per env for all n_steps control steps, lane l owning the candidates k = l, l + 64, ..., the
// real state and its carry in registers, the mean in the wave's LDS slice — with the planner replaced.  Per control step, `iterations`
// times:
//   (a, b) the lanes clamp the mean and, in the first iteration, set the sigma slice (a second LDS slice per wave) to the scalar;
//   (c) every lane scores its candidates as pend_mpc_mppi_kernel does (pend_plan_kernel's DRAWN loop, the draws reading mean and sigma
//       from LDS), keeps the returns in `work` and folds (k*, r*);
//       the elite set is plan_cem_finish_kernel's: the MSB-first radix select over plan_key (eight passes, 256 LDS counters per wave,
//       a suffix scan over the lanes), then membership row by row (ballot + prefix popcount, ties to the lower k), the flag written
//       over the return and read back by the lane that wrote it only;
//       the moments are that kernel's step 4, copied rather than shared: the members alone redrawn, d = (double)a - m0, S1 / S2 per
//       lane in ascending k, the butterfly, m0 + S1 / M and sqrt(max(S2 / M - mu^2, 0)); lane 0 writes mean and sigma into LDS behind a
//       fence, so that every lane's draws of that block have read the old entries (the in-place rule);
//   (d) the lanes floor the sigma.
// Then act, step, auto-reset and shift: pend_mpc_mppi_kernel's steps 4 and 5.
// stage_trig_table's block barrier is taken by every wave, also by those past n; after it the waves of a block run different trip
// counts, so there is NO block barrier (plan_cem_finish_kernel's __syncthreads() around the counters become wave_lds_fence(): the
// counters are per wave, and a wave's LDS operations — the ds_add of the histogram included — execute in order).
template <class Env>
__global__ void __launch_bounds__(kBlock) pend_mpc_cem_kernel(const MpcCemArgs<Env> a) {
    using R = typename Env::real;
    using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
    using Spec = typename std::conditional<Env::kDiscrete, CandidateSpecLds, CandidateSpecLdsMap>::type;
    constexpr bool kMap = !Env::kDiscrete;
    constexpr int kWavesPerBlock = kBlock / kWave;
    constexpr int na = Env::kActDim;                          // components per step of the mean
    constexpr int act_dim = Env::kDiscrete ? 0 : Env::kActDim;  // draw_action's: 0 = coin flips
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    __shared__ float nom_s[kWavesPerBlock][EMEI_MPC_MAX_HORIZON * na];
    __shared__ float sig_s[kWavesPerBlock][kMap ? EMEI_MPC_MAX_HORIZON * na : 1];
    __shared__ uint32_t hist_s[kWavesPerBlock][256];
    stage_trig_table(trig_s, a.trig, Env::trig_rot_c(), Env::trig_rot_s());
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wv;  // wave-uniform
    if (i >= a.n) return;
    const int64_t n = a.n;
    const int32_t n_cand = a.n_cand, horizon = a.horizon;
    const int32_t n_comp = horizon * na;  // <= EMEI_MPC_MAX_HORIZON * na (abi.hip)
    float* nom = nom_s[wv];
    float* sig = sig_s[wv];
    uint32_t* hist = hist_s[wv];
    for (int32_t c = lane; c < n_comp; c += kWave) nom[c] = a.nominal[((int64_t)(c / na) * n + i) * na + c % na];

    R s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = a.state[k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    typename Env::Carry c;
    trig_ctx_init(c.trig, trig_s);
    const bool auto_reset = (a.flags & EMEI_FLAG_AUTO_RESET) != 0;
    const uint64_t g = a.env_offset + (uint64_t)i;
    double* wt = a.work + i * n_cand;
    Spec sp;
    sp.env_offset = a.env_offset;
    sp.nominal.p = (const __attribute__((address_space(3))) float*)nom;
    if constexpr (kMap) sp.sigma_map.p = (const __attribute__((address_space(3))) float*)sig;
    else sp.sigma = a.sigma;
    sp.lo = a.lo, sp.hi = a.hi;
    const double m_el = (double)a.n_elites;
    uint32_t done = 0;

    for (int32_t t = 0; t < a.n_steps; ++t) {
        Env::prime(s, c, a.p);
        for (int32_t it = 0; it < a.iterations; ++it) {
            // (a), (b)
            for (int32_t cc = lane; cc < n_comp; cc += kWave) {
                nom[cc] = fminf(fmaxf(nom[cc], a.nominal_lo), a.nominal_hi);
                if constexpr (kMap) {
                    if (it == 0) sig[cc] = a.sigma;
                }
            }
            wave_lds_fence();
            // (c) the returns and (k*, r*)
            sp.seed = a.seed + (uint64_t)t * (uint64_t)a.iterations + (uint64_t)it;
            double rs = __builtin_nan("");  // (NaN, INT32_MAX) loses to every candidate
            int32_t ks = INT32_MAX;
            for (int32_t k0 = 0; k0 < n_cand; k0 += kWave) {  // wave-uniform trip count: every lane takes part in the ballot
                const int32_t k = k0 + lane;
                R cs[4] = {s[0], s[1], s[2], s[3]};
                typename Env::Carry cc = c;
                CandidateWordsT<true> cw(sp.seed, g, (uint32_t)k);
                double ret = 0.0, gd = 1.0;
                bool live = k < n_cand;
                for (int32_t h = 0; h < horizon; ++h) {
                    R o[4], rew;
                    bool term;
                    const DrawT act = (DrawT)draw_action(cw, sp, 1, 0, h, 0, act_dim);
                    Env::step(cs, cc, Env::decode_t(act), a.p, a.freq_rate, o, rew, term);
                    if (live) {
                        ret = ret + gd * (double)(float)rew;
                        gd = gd * a.discount;
                        if (term) live = false;
                    }
                    if (__ballot(live) == 0ull) break;  // wave-uniform
                }
                if (k < n_cand) {
                    wt[k] = ret;
                    if (plan_replaces(rs, ks, ret, k)) rs = ret, ks = k;
                }
            }
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const double r2 = __shfl_xor(rs, d, kWave);
                const int32_t k2 = __shfl_xor(ks, d, kWave);
                if (plan_replaces(rs, ks, r2, k2)) rs = r2, ks = k2;
            }
            const bool last_it = it == a.iterations - 1;
            if (lane == 0 && last_it && a.plan_return_out) a.plan_return_out[(int64_t)t * n + i] = rs;
            // the threshold: `need` = the rank looked for among the candidates whose bytes above `shift` equal `prefix`'s
            uint64_t prefix = 0ull;
            int32_t need = a.n_elites;
            for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
                for (int b = 0; b < 4; ++b) hist[4 * lane + b] = 0u;
                wave_lds_fence();
                for (int32_t k = lane; k < n_cand; k += kWave) {
                    const uint64_t key = plan_key(wt[k]);
                    const uint64_t high = shift == 56 ? 0ull : key >> (shift + 8);
                    if (high == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
                }
                wave_lds_fence();
                int32_t cb[4], own = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) cb[b] = (int32_t)hist[4 * lane + b], own += cb[b];
                int32_t above = own;  // candidates in this lane's bins and in those of the lanes above it
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) {
                    const int32_t up = __shfl_down(above, d, kWave);
                    if (lane + d < kWave) above += up;
                }
                above -= own;
                const bool mine = above < need && need <= above + own;  // one lane
                int32_t digit = 0, rest = need;
                if (mine) {
                    int32_t acc = above;
#pragma unroll
                    for (int b = 3; b >= 0; --b) {
                        if (acc < need && need <= acc + cb[b]) digit = 4 * lane + b, rest = need - acc;
                        acc += cb[b];
                    }
                }
                const unsigned long long owner = __ballot(mine);
                const int src = owner ? __builtin_ctzll(owner) : 0;
                digit = __shfl(digit, src, kWave), need = __shfl(rest, src, kWave);
                prefix = (prefix << 8) | (uint64_t)(uint32_t)digit;
                wave_lds_fence();  // the counters are read before the next pass clears them
            }
            // membership: prefix = T, need = how many of the key == T candidates are members (>= 1)
            int32_t taken = 0;
            for (int32_t k0 = 0; k0 < n_cand; k0 += kWave) {  // wave-uniform trip count: every lane takes part in the ballot
                const int32_t k = k0 + lane;
                const double r = k < n_cand ? wt[k] : 0.0;
                const uint64_t key = plan_key(r);
                const bool tie = k < n_cand && key == prefix;
                const unsigned long long ties = __ballot(tie);
                const int32_t rank = taken + (int32_t)__popcll(ties & ((1ull << lane) - 1ull));  // of this lane's tie among all ties, by k
                const bool in = k < n_cand && (key > prefix || (tie && rank < need));
                if (k < n_cand) wt[k] = in ? 1.0 : 0.0;
                if (tie && rank == need - 1 && last_it && a.elite_return_out) a.elite_return_out[(int64_t)t * n + i] = r;
                taken += (int32_t)__popcll(ties);
            }
            // the moments (plan_cem_finish_kernel's step 4)
            for (int32_t c0 = 0; c0 < n_comp; c0 += 4) {
                double m0[4], s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int32_t cc = min(c0 + u, n_comp - 1);  // past the end: the last component again, dropped below
                    m0[u] = Env::kDiscrete ? 0.0 : (double)nom[cc];
                }
                for (int32_t k = lane; k < n_cand; k += kWave) {
                    if (wt[k] == 0.0) continue;  // no draw for a candidate outside the set
                    CandidateWordsT<true> cw(sp.seed, g, (uint32_t)k);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int32_t cc = min(c0 + u, n_comp - 1);
                        const double d = (double)draw_action(cw, sp, 1, 0, cc / na, cc % na, act_dim) - m0[u];
                        s1[u] += d, s2[u] += d * d;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int d = 1; d < kWave; d <<= 1) s1[u] += __shfl_xor(s1[u], d, kWave);
#pragma unroll
                    for (int d = 1; d < kWave; d <<= 1) s2[u] += __shfl_xor(s2[u], d, kWave);
                }
                wave_lds_fence();  // every lane's draws (and m0) of this block have read the entries lane 0 now replaces
                if (lane == 0) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int32_t cc = c0 + u;
                        if (cc >= n_comp) continue;
                        const double mu = s1[u] / m_el;
                        nom[cc] = (float)(m0[u] + mu);
                        if constexpr (kMap) sig[cc] = (float)sqrt(fmax(s2[u] / m_el - mu * mu, 0.0));
                    }
                }
            }
            wave_lds_fence();  // lane 0's mean and sigma are what every lane reads from here on
            // (d)
            if constexpr (kMap) {
                for (int32_t cc = lane; cc < n_comp; cc += kWave) sig[cc] = fmaxf(sig[cc], a.sigma_min);
                wave_lds_fence();
            }
        }
        // act
        float av[na];
#pragma unroll
        for (int q = 0; q < na; ++q) {
            av[q] = nom[q];
            if constexpr (Env::kDiscrete) av[q] = av[q] >= 0.5f ? 1.f : 0.f;
            if (lane == 0) store_action(a.actions_out, a.action_dtype, ((int64_t)t * n + i) * na + q, av[q]);
        }
        // step: the wave-uniform real state, computed redundantly by every lane; lane 0 stores
        {
            R o[4], rew;
            bool term;
            Env::step(s, c, Env::decode_t((DrawT)av[0]), a.p, a.freq_rate, o, rew, term);
            ++steps;
            const bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
            done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
            if (lane == 0) {
                const int64_t at = (int64_t)t * n + i;
                if (a.obs_out) a.obs_out[at] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
                if (a.reward_out) a.reward_out[at] = (float)rew;
                if (a.done_out) a.done_out[at] = (uint8_t)done;
            }
        }
        const bool reset_now = auto_reset && __builtin_amdgcn_readfirstlane(done) != 0u;  // wave-uniform
        if (reset_now) {
            ++episode;
            steps = 0;
            Env::init(s, a.reset_seed, g, episode, a.p);
        }
        // warm start, pass by pass in ascending order: a pass reads [base + na, base + 64 + na) and writes [base, base + 64)
        for (int32_t base = 0; base < n_comp; base += kWave) {
            const int32_t cc = base + lane;
            const float v = (!reset_now && cc + na < n_comp) ? nom[cc + na] : a.refill;
            wave_lds_fence();
            if (cc < n_comp) nom[cc] = v;
            wave_lds_fence();
        }
    }

    for (int32_t cc = lane; cc < n_comp; cc += kWave) a.nominal[((int64_t)(cc / na) * n + i) * na + cc % na] = nom[cc];
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.state[k * n + i] = s[k];
        a.steps[i] = steps;
        a.episode[i] = episode;
        ((unsigned long long*)wt)[0] = (unsigned long long)done;  // lane 0's own slot, after its last use
    }
}

// ---------------------------------------------------------------------------------------------
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

#ifndef EMEI_XCD_CONTIGUOUS
#define EMEI_XCD_CONTIGUOUS 1  // 0: a variant build with the identity workgroup -> env block map, for A/B runs
#endif
#ifndef EMEI_SPLIT_LAUNCH
#define EMEI_SPLIT_LAUNCH 1  // 0: a variant build without the split of large HBM-bound launches, for A/B runs
#endif
// CUs of the current device (cached: the launch path neither allocates nor synchronises; an attribute query is neither)
static inline int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus[dev] = 256;
    return cus[dev];
}

// Returns the enum emei_kernel_id launched, or a negative EMEI_ERR_* (peers set on a path that has no peer stores).
template <class Env, typename ActT>
static int launch_rollout_full(const RolloutArgs<Env>& a, dim3 grid, hipStream_t stream, const ObsPeers& peers) {
    const bool full = a.obs_out && a.reward_out && a.done_out;
    PeerObs po{};
    if (peers.count > 0) {
        if (!Env::kPeerWrite) return EMEI_ERR_UNSUPPORTED;
        for (int p = 0; p < peers.count; ++p) {
            if (!aligned16(peers.obs[p])) return EMEI_ERR_UNSUPPORTED;
            po.obs[p] = (float4*)peers.obs[p];
        }
        po.row_envs = peers.row_envs, po.col = peers.col, po.count = (uint32_t)peers.count;
    }
    if (full && a.n_steps >= stage_steps<ActT>() && a.n % kWave == 0 && aligned16(a.actions) && aligned16(a.obs_out) &&
        aligned16(a.reward_out) && aligned16(a.done_out))
    {
        // Env::kSplitLaunch (the HBM-bound CartPole kernels): a shard of 2 or 3 waves per SIMD (BASELINE configs[4]'s 131 072 envs per GPU)
        // runs as consecutive launches of ONE wave per SIMD each (one 256-thread block per CU): co-resident waves' write streams
        // get in each other's way at that occupancy.  Same box: 131 072 envs 0.706 -> 0.671 ms, 196 608 0.976 -> 0.912; nothing at
        // 4 waves per SIMD, +8 % (worse) at 8, nothing at 16 — hence kSplitMaxRounds = 3 (profiles/r05_split_launch.txt).  Envs are
        // independent: the same bits.
        unsigned per_launch = grid.x;
        if constexpr (EMEI_SPLIT_LAUNCH != 0 && Env::kSplitLaunch) {
            const unsigned round = (unsigned)device_cus();  // blocks of one wave per SIMD
            if (grid.x > round && grid.x <= Env::kSplitMaxRounds * round) per_launch = round;
        }
        RolloutArgs<Env> b = a;
#ifdef EMEI_XCD_ALWAYS  // experiment: the XCD-contiguous map at every size
        const bool big = true;
#else
        const bool big = grid.x > (unsigned)device_cus();  // more than one wave per SIMD
#endif
        for (unsigned first = 0; first < grid.x; first += per_launch) {
            b.first_block = first;
            const dim3 g(min(per_launch, grid.x - first));
            b.xcd_contiguous = EMEI_XCD_CONTIGUOUS != 0 && Env::kXcdContiguous && big && g.x % 8 == 0;
            if constexpr (Env::kPeerWrite) {
                if (po.count > 0) {
                    if (a.freq_rate == 1)
                        hipLaunchKernelGGL((pend_rollout_staged_peers_kernel<Env, ActT, true>), g, dim3(kBlock), 0, stream, b, po);
                    else
                        hipLaunchKernelGGL((pend_rollout_staged_peers_kernel<Env, ActT, false>), g, dim3(kBlock), 0, stream, b, po);
                    continue;
                }
            }
            if (a.freq_rate == 1)
                hipLaunchKernelGGL((pend_rollout_staged_kernel<Env, ActT, true>), g, dim3(kBlock), 0, stream, b);
            else
                hipLaunchKernelGGL((pend_rollout_staged_kernel<Env, ActT, false>), g, dim3(kBlock), 0, stream, b);
        }
        if (po.count > 0) return a.freq_rate == 1 ? EMEI_KERNEL_PEND_STAGED_PEERS_FREQ1 : EMEI_KERNEL_PEND_STAGED_PEERS;
        return a.freq_rate == 1 ? EMEI_KERNEL_PEND_STAGED_FREQ1 : EMEI_KERNEL_PEND_STAGED;
    }
    if (po.count > 0) return EMEI_ERR_UNSUPPORTED;  // ragged n, a short horizon, unaligned or missing outputs: the generic kernels have no peer stores
    if (full) {
        hipLaunchKernelGGL((pend_rollout_kernel<Env, ActT, true>), grid, dim3(kBlock), 0, stream, a);
        return EMEI_KERNEL_PEND_GENERIC_FULL;
    }
    hipLaunchKernelGGL((pend_rollout_kernel<Env, ActT, false>), grid, dim3(kBlock), 0, stream, a);
    return EMEI_KERNEL_PEND_GENERIC;
}

// the one launch of pend_plan_kernel: DRAWN kernels read no actions and write no lengths or final observations, and only KEEP
// gives them a return_out; one lane per candidate, n * n_candidates < 2^31 (checked in abi.hip)
template <class Env, class ActT, bool DRAWN, bool KEEP, class Spec>
static void launch_pend_plan(const PendLaunch& L, const RolloutArgs<Env>& a, const Spec& sp) {
    const PlanLaunch& P = L.plan;
    const dim3 pgrid((unsigned)((L.n * P.n_candidates + kBlock - 1) / kBlock));
    hipLaunchKernelGGL((pend_plan_kernel<Env, ActT, DRAWN, KEEP, Spec>), pgrid, dim3(kBlock), 0, L.stream,
                       (const typename Env::real*)L.state, P.start_rows, DRAWN ? nullptr : (const ActT*)L.actions, L.n, P.n_candidates,
                       L.n_steps, P.discount, L.freq_rate, a.p, a.trig, DRAWN && !KEEP ? nullptr : P.return_out,
                       DRAWN ? nullptr : P.length_out, DRAWN ? nullptr : (float4*)L.obs_out, sp,
                       DRAWN ? (PlanPartial*)P.partials : nullptr);
}

// the one launch of pend_plan_value_kernel: launch_pend_plan's arguments on one-wave blocks with the value network's h1 tile; the
// drawn kernels always keep their returns
template <class Env, class ActT, bool DRAWN, class Spec>
static int launch_pend_plan_value(const PendLaunch& L, const RolloutArgs<Env>& a, const Spec& sp) {
    const PlanLaunch& P = L.plan;
    if (int rc = policy_deep_lds_opt_in<pend_plan_value_kernel<Env, ActT, DRAWN, Spec>>()) return rc;
    const dim3 pgrid((unsigned)((L.n * P.n_candidates + kWave - 1) / kWave));
    hipLaunchKernelGGL((pend_plan_value_kernel<Env, ActT, DRAWN, Spec>), pgrid, dim3(kWave), policy_deep_tile_bytes(L.policy_value.hidden1),
                       L.stream, (const typename Env::real*)L.state, P.start_rows, DRAWN ? nullptr : (const ActT*)L.actions, L.n,
                       P.n_candidates, L.n_steps, P.discount, L.freq_rate, a.p, a.trig, L.policy_value, P.return_out,
                       DRAWN ? nullptr : P.length_out, DRAWN ? nullptr : (float4*)L.obs_out, sp, DRAWN ? (PlanPartial*)P.partials : nullptr);
    return EMEI_OK;
}

// host-side dispatch over (env id, precision)
// every launch of one Env type (one translation unit instantiates exactly one Env: pendulum_tu.hip)
template <class Env>
static int launch_env(const PendLaunch& L) {
    using R = typename Env::real;
    RolloutArgs<Env> a;
    a.state = (R*)L.state;
    a.steps = L.steps;
    a.episode = L.episode;
    a.done_mask = L.done_mask;
    a.actions = L.actions;
    a.trig = (const SinCosEntry*)L.trig;
    a.obs_out = (float4*)L.obs_out;
    a.reward_out = L.reward_out;
    a.done_out = L.done_out;
    a.n = L.n;
    a.n_steps = L.n_steps;
    a.freq_rate = L.freq_rate;
    a.action_dtype = L.action_dtype;
    a.max_episode_steps = L.max_episode_steps;
    a.flags = L.flags;
    a.seed = L.seed;
    a.env_offset = L.env_offset;
    a.p = Env::make_params(L.p);
    a.obs_f64 = L.op == OP_ROLLOUT ? L.obs_f64 : nullptr;
    a.host_flag = L.op == OP_ROLLOUT ? L.host_flag : nullptr;
    a.flag_value = L.flag_value;
    a.first_block = 0, a.xcd_contiguous = 0;
    dim3 grid((unsigned)((L.n + kBlock - 1) / kBlock));
    switch (L.op) {
        case OP_ROLLOUT: {
            // discrete envs take uint8/int32/int64 actions, continuous envs float32
            int sel;
            if constexpr (Env::kDiscrete) {
                if (L.action_dtype == EMEI_ACT_U8) sel = launch_rollout_full<Env, uint8_t>(a, grid, L.stream, L.peers);
                else if (L.action_dtype == EMEI_ACT_I32) sel = launch_rollout_full<Env, int32_t>(a, grid, L.stream, L.peers);
                else if (L.action_dtype == EMEI_ACT_I64) sel = launch_rollout_full<Env, int64_t>(a, grid, L.stream, L.peers);
                else return EMEI_ERR_INVALID;
            } else {
                if (L.action_dtype != EMEI_ACT_F32) return EMEI_ERR_INVALID;
                sel = launch_rollout_full<Env, float>(a, grid, L.stream, L.peers);
            }
            if (sel < 0) return sel;
            if (L.selected) *L.selected = sel;
            break;
        }
        case OP_RESET:
            hipLaunchKernelGGL(pend_reset_kernel<Env>, grid, dim3(kBlock), 0, L.stream, (R*)L.state, L.steps,
                               L.episode, L.n, L.seed, L.env_offset, a.p);
            break;
        case OP_INIT_OBS:
            hipLaunchKernelGGL(pend_init_obs_kernel<Env>, grid, dim3(kBlock), 0, L.stream, L.env_index, L.episode_in,
                               (float4*)L.obs_out, L.n, L.seed, L.env_offset, a.p);
            break;
        case OP_GET_OBS:
            hipLaunchKernelGGL(pend_get_obs_kernel<Env>, grid, dim3(kBlock), 0, L.stream, (const R*)L.state,
                               L.obs_f64, L.n);
            break;
        case OP_REWARD_TERMINAL:
            if (L.io_f64)
                hipLaunchKernelGGL((pend_reward_terminal_kernel<Env, double>), grid, dim3(kBlock), 0, L.stream,
                                   (const double*)L.obs_in, (double*)L.reward_out, L.done_out, L.n, a.p, a.trig);
            else
                hipLaunchKernelGGL((pend_reward_terminal_kernel<Env, float>), grid, dim3(kBlock), 0, L.stream,
                                   (const float*)L.obs_in, (float*)L.reward_out, L.done_out, L.n, a.p, a.trig);
            break;
        case OP_NEXT_OBS:
            if (L.io_f64)
                hipLaunchKernelGGL((pend_next_obs_kernel<Env, double>), grid, dim3(kBlock), 0, L.stream, (const double*)L.obs_in,
                                   L.actions, L.action_dtype, (double*)L.obs_out, L.n, L.freq_rate, a.p, a.trig);
            else
                hipLaunchKernelGGL((pend_next_obs_kernel<Env, float>), grid, dim3(kBlock), 0, L.stream, (const float*)L.obs_in,
                                   L.actions, L.action_dtype, (float*)L.obs_out, L.n, L.freq_rate, a.p, a.trig);
            break;
        case OP_PLAN: {
            const PlanLaunch& P = L.plan;
            if (P.mode == PLAN_GIVEN) {
                // discrete envs take uint8/int32/int64 actions, continuous envs float32
                const CandidateSpec none{};
                if constexpr (Env::kDiscrete) {
                    if (L.action_dtype == EMEI_ACT_U8) launch_pend_plan<Env, uint8_t, false, false>(L, a, none);
                    else if (L.action_dtype == EMEI_ACT_I32) launch_pend_plan<Env, int32_t, false, false>(L, a, none);
                    else if (L.action_dtype == EMEI_ACT_I64) launch_pend_plan<Env, int64_t, false, false>(L, a, none);
                    else return EMEI_ERR_INVALID;
                } else {
                    if (L.action_dtype != EMEI_ACT_F32) return EMEI_ERR_INVALID;
                    launch_pend_plan<Env, float, false, false>(L, a, none);
                }
                break;
            }
            using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
            if (!P.partials) return EMEI_ERR_INVALID;
            if (P.mode == PLAN_DRAWN_KEEP && !P.return_out) return EMEI_ERR_INVALID;
            if (P.sigma_map) {  // emei_plan_cem with a sigma per entry: continuous envs, every return kept
                if constexpr (!Env::kDiscrete) {
                    if (P.mode != PLAN_DRAWN_KEEP) return EMEI_ERR_INVALID;
                    launch_pend_plan<Env, DrawT, true, true>(L, a, CandidateSpecMap(P.cand, P.sigma_map));
                } else {
                    return EMEI_ERR_INVALID;
                }
            } else if (P.mode == PLAN_DRAWN_KEEP) {
                launch_pend_plan<Env, DrawT, true, true>(L, a, P.cand);
            } else {
                launch_pend_plan<Env, DrawT, true, false>(L, a, P.cand);
            }
            break;
        }
        case OP_MPC_MPPI: {
            MpcArgs<Env> m;
            m.state = (R*)L.state, m.steps = L.steps, m.episode = L.episode, m.trig = a.trig;
            m.nominal = L.mpc.nominal, m.work = L.plan.return_out, m.actions_out = L.mpc.actions_out;
            m.obs_out = (float4*)L.obs_out, m.reward_out = L.reward_out, m.done_out = L.done_out;
            m.plan_return_out = L.mpc.plan_return_out, m.ess_out = L.mpc.ess_out;
            m.n = L.n, m.n_steps = L.n_steps, m.horizon = L.mpc.horizon, m.n_cand = L.plan.n_candidates, m.freq_rate = L.freq_rate;
            m.action_dtype = L.action_dtype, m.max_episode_steps = L.max_episode_steps, m.flags = L.flags;
            m.reset_seed = L.seed, m.env_offset = L.env_offset, m.seed = L.plan.cand.seed;
            m.discount = L.plan.discount, m.temperature = L.mpc.temperature;
            m.sigma = L.plan.cand.sigma, m.lo = L.plan.cand.lo, m.hi = L.plan.cand.hi;
            m.refill = L.mpc.refill, m.nominal_lo = L.mpc.nominal_lo, m.nominal_hi = L.mpc.nominal_hi;
            m.p = a.p;
            if (L.mpc.horizon < 1 || L.mpc.horizon > EMEI_MPC_MAX_HORIZON) return EMEI_ERR_INVALID;  // the LDS slice of the nominal
            constexpr int kWavesPerBlock = kBlock / kWave;  // one wave per env
            const dim3 mgrid((unsigned)((L.n + kWavesPerBlock - 1) / kWavesPerBlock));
            hipLaunchKernelGGL(pend_mpc_mppi_kernel<Env>, mgrid, dim3(kBlock), 0, L.stream, m);
            if (L.selected) *L.selected = EMEI_KERNEL_PEND_MPC_MPPI;
            break;
        }
        case OP_MPC_CEM: {
            MpcCemArgs<Env> m;
            m.state = (R*)L.state, m.steps = L.steps, m.episode = L.episode, m.trig = a.trig;
            m.nominal = L.mpc.nominal, m.work = L.plan.return_out, m.actions_out = L.mpc.actions_out;
            m.obs_out = (float4*)L.obs_out, m.reward_out = L.reward_out, m.done_out = L.done_out;
            m.plan_return_out = L.mpc.plan_return_out, m.elite_return_out = L.mpc.elite_return_out;
            m.n = L.n, m.n_steps = L.n_steps, m.horizon = L.mpc.horizon, m.n_cand = L.plan.n_candidates, m.n_elites = L.mpc.n_elites;
            m.iterations = L.mpc.iterations, m.freq_rate = L.freq_rate;
            m.action_dtype = L.action_dtype, m.max_episode_steps = L.max_episode_steps, m.flags = L.flags;
            m.reset_seed = L.seed, m.env_offset = L.env_offset, m.seed = L.plan.cand.seed;
            m.discount = L.plan.discount;
            m.sigma = L.plan.cand.sigma, m.sigma_min = L.mpc.sigma_min, m.lo = L.plan.cand.lo, m.hi = L.plan.cand.hi;
            m.refill = L.mpc.refill, m.nominal_lo = L.mpc.nominal_lo, m.nominal_hi = L.mpc.nominal_hi;
            m.p = a.p;
            if (L.mpc.horizon < 1 || L.mpc.horizon > EMEI_MPC_MAX_HORIZON) return EMEI_ERR_INVALID;  // the LDS slices of the mean and the sigma
            if (L.mpc.iterations < 1 || L.mpc.n_elites < 1 || L.mpc.n_elites > L.plan.n_candidates) return EMEI_ERR_INVALID;
            constexpr int kWavesPerBlock = kBlock / kWave;  // one wave per env
            const dim3 mgrid((unsigned)((L.n + kWavesPerBlock - 1) / kWavesPerBlock));
            hipLaunchKernelGGL(pend_mpc_cem_kernel<Env>, mgrid, dim3(kBlock), 0, L.stream, m);
            if (L.selected) *L.selected = EMEI_KERNEL_PEND_MPC_CEM;
            break;
        }
        case OP_MPC_POLICY: {
            MpcPolicyArgs<Env> m;
            m.state = (R*)L.state, m.steps = L.steps, m.episode = L.episode, m.trig = a.trig;
            m.work = L.plan.return_out, m.actions_out = L.mpc.actions_out;
            m.obs_out = (float4*)L.obs_out, m.reward_out = L.reward_out, m.done_out = L.done_out;
            m.plan_return_out = L.mpc.plan_return_out, m.plan_index_out = L.mpc.plan_index_out, m.ess_out = L.mpc.ess_out;
            m.n = L.n, m.n_steps = L.n_steps, m.horizon = L.mpc.horizon, m.n_cand = L.plan.n_candidates, m.freq_rate = L.freq_rate;
            m.action_dtype = L.action_dtype, m.max_episode_steps = L.max_episode_steps, m.act_mode = L.mpc.act_mode, m.flags = L.flags;
            m.reset_seed = L.seed, m.env_offset = L.env_offset, m.seed_stride = L.mpc.seed_stride;
            m.discount = L.plan.discount, m.temperature = L.mpc.temperature;
            m.p = a.p;
            if (L.mpc.horizon < 1 || L.plan.n_candidates < 1 || !m.work || !m.actions_out) return EMEI_ERR_INVALID;
            constexpr int kWavesPerBlock = kBlock / kWave;  // one wave per env
            const dim3 mgrid((unsigned)((L.n + kWavesPerBlock - 1) / kWavesPerBlock));
            hipLaunchKernelGGL(pend_mpc_policy_kernel<Env>, mgrid, dim3(kBlock), 0, L.stream, m, L.policy, L.policy_noise);
            if (L.selected) *L.selected = EMEI_KERNEL_PEND_MPC_POLICY;
            break;
        }
        case OP_POLICY:
            if (L.peers.count > 0) return EMEI_ERR_UNSUPPORTED;  // no peer stores on this kernel (abi.hip refuses with a message)
            hipLaunchKernelGGL(pend_policy_rollout_kernel<Env>, grid, dim3(kBlock), 0, L.stream, a, L.policy);
            if (L.selected) *L.selected = EMEI_KERNEL_PEND_POLICY;
            break;
        case OP_POLICY_NOISY:
            if (L.peers.count > 0) return EMEI_ERR_UNSUPPORTED;
            hipLaunchKernelGGL(pend_policy_rollout_noisy_kernel<Env>, grid, dim3(kBlock), 0, L.stream, a, L.policy, L.policy_noise);
            if (L.selected) *L.selected = EMEI_KERNEL_PEND_POLICY_NOISY;
            break;
        case OP_POLICY_EVAL: {  // emei_evaluate_policies: block b = (policy b / grid.x, env block b % grid.x); abi.hip bounds the grid
            const PlanLaunch& P = L.plan;
            hipLaunchKernelGGL(pend_policy_eval_kernel<Env>, dim3(grid.x * (unsigned)P.n_candidates), dim3(kBlock), 0, L.stream,
                               (const R*)L.state, P.start_rows, L.n, grid.x, L.n_steps, P.discount, L.freq_rate, a.p, a.trig, L.policy,
                               P.return_out, P.length_out, (float4*)L.obs_out);
            break;
        }
        case OP_POLICY_PLAN: {  // emei_plan_policy: one lane per candidate, n * n_candidates < 2^31 (checked in abi.hip)
            const PlanLaunch& P = L.plan;
            if (!P.partials || !P.return_out || !P.first_actions) return EMEI_ERR_INVALID;
            const dim3 pgrid((unsigned)((L.n * P.n_candidates + kBlock - 1) / kBlock));
            hipLaunchKernelGGL(pend_policy_plan_kernel<Env>, pgrid, dim3(kBlock), 0, L.stream, (const R*)L.state, P.start_rows, L.n,
                               P.n_candidates, L.n_steps, P.discount, L.freq_rate, a.p, a.trig, L.policy, L.policy_noise, L.env_offset,
                               P.return_out, P.first_actions, (PlanPartial*)P.partials);
            break;
        }
        case OP_POLICY_PLAN_DEEP: {  // emei_plan_policy_deep: OP_POLICY_PLAN's lanes as one-wave blocks, the tile as dynamic LDS
            const PlanLaunch& P = L.plan;
            if (!P.partials || !P.return_out || !P.first_actions) return EMEI_ERR_INVALID;
            if (int rc = policy_deep_lds_opt_in<pend_policy_plan_deep_kernel<Env>>()) return rc;
            const dim3 pgrid((unsigned)((L.n * P.n_candidates + kWave - 1) / kWave));
            const int h1 = L.policy_value.w1 && L.policy_value.hidden1 > L.policy_deep.hidden1 ? L.policy_value.hidden1 : L.policy_deep.hidden1;
            hipLaunchKernelGGL(pend_policy_plan_deep_kernel<Env>, pgrid, dim3(kWave), policy_deep_tile_bytes(h1), L.stream, (const R*)L.state,
                               P.start_rows, L.n, P.n_candidates, L.n_steps, P.discount, L.freq_rate, a.p, a.trig, L.policy_deep,
                               L.policy_noise, L.policy_value, L.env_offset, P.return_out, P.first_actions, (PlanPartial*)P.partials);
            break;
        }
        case OP_POLICY_DEEP: {  // one-wave blocks, the wave's h1 tile as dynamic LDS
            if (L.peers.count > 0) return EMEI_ERR_UNSUPPORTED;
            if (int rc = policy_deep_lds_opt_in<pend_policy_rollout_deep_kernel<Env>>()) return rc;
            const dim3 wgrid((unsigned)((L.n + kWave - 1) / kWave));
            hipLaunchKernelGGL(pend_policy_rollout_deep_kernel<Env>, wgrid, dim3(kWave), policy_deep_tile_bytes(L.policy_deep.hidden1),
                               L.stream, a, L.policy_deep, L.policy_noise);
            if (L.selected) *L.selected = EMEI_KERNEL_PEND_POLICY_DEEP;
            break;
        }
        case OP_POLICY_EVAL_DEEP: {  // block b = (policy b / env waves, env wave b % env waves); abi.hip bounds the grid
            const PlanLaunch& P = L.plan;
            if (int rc = policy_deep_lds_opt_in<pend_policy_eval_deep_kernel<Env>>()) return rc;
            const unsigned env_waves = (unsigned)((L.n + kWave - 1) / kWave);
            hipLaunchKernelGGL(pend_policy_eval_deep_kernel<Env>, dim3(env_waves * (unsigned)P.n_candidates), dim3(kWave),
                               policy_deep_tile_bytes(L.policy_deep.hidden1), L.stream, (const R*)L.state, P.start_rows, L.n, env_waves,
                               L.n_steps, P.discount, L.freq_rate, a.p, a.trig, L.policy_deep, P.return_out, P.length_out,
                               (float4*)L.obs_out);
            break;
        }
        case OP_PLAN_VALUE: {  // OP_PLAN's dispatch over pend_plan_value_kernel; PLAN_DRAWN goes to the KEEP instantiation
            const PlanLaunch& P = L.plan;
            if (!L.policy_value.w1 || !P.return_out) return EMEI_ERR_INVALID;
            int rc;
            if (P.mode == PLAN_GIVEN) {
                const CandidateSpec none{};
                if constexpr (Env::kDiscrete) {
                    if (L.action_dtype == EMEI_ACT_U8) rc = launch_pend_plan_value<Env, uint8_t, false>(L, a, none);
                    else if (L.action_dtype == EMEI_ACT_I32) rc = launch_pend_plan_value<Env, int32_t, false>(L, a, none);
                    else if (L.action_dtype == EMEI_ACT_I64) rc = launch_pend_plan_value<Env, int64_t, false>(L, a, none);
                    else return EMEI_ERR_INVALID;
                } else {
                    if (L.action_dtype != EMEI_ACT_F32) return EMEI_ERR_INVALID;
                    rc = launch_pend_plan_value<Env, float, false>(L, a, none);
                }
            } else {
                using DrawT = typename std::conditional<Env::kDiscrete, int, float>::type;
                if (!P.partials) return EMEI_ERR_INVALID;
                if (P.sigma_map) {  // emei_plan_cem_value with a sigma per entry: continuous envs
                    if constexpr (!Env::kDiscrete) rc = launch_pend_plan_value<Env, DrawT, true>(L, a, CandidateSpecMap(P.cand, P.sigma_map));
                    else return EMEI_ERR_INVALID;
                } else {
                    rc = launch_pend_plan_value<Env, DrawT, true>(L, a, P.cand);
                }
            }
            if (rc) return rc;
            break;
        }
        default: return EMEI_ERR_INVALID;
    }
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}


}  // namespace emei
