// body_mpc_kernels.h — emei_mpc_mppi / emei_mpc_cem for the bodies that opt in with Body::kFusedMpc (the InvertedDoublePendulum):
// receding-horizon control episodes in ONE launch (the normative text: include/emei_hip.h).  Included by body_kernels.h, in front of
// launch_body.
//
// The skeleton is pend_mpc_mppi_kernel's / pend_mpc_cem_kernel's (pendulum_kernels.h): one WAVE per env for all n_steps control steps, in
// 256-thread blocks of four envs; lane l owns the candidates k = l, l + 64, ...; the mean (for CEM also the per-entry sigma and the
// 256 select counters) lives in the wave's LDS slice; the env's real state, its step and episode counters are wave-uniform values in
// registers, computed redundantly by every lane.  stage_trig_table's block barrier is taken by every wave, also by those past n; after
// it the waves of a block run different trip counts, so there is NO block barrier: what lane 0 writes into LDS reaches the other lanes
// through wave_lds_fence().
//
// What a body changes is the model.  Scoring is body_plan_kernel's DRAWN loop, expression for expression (a fresh word stream, `pre`,
// a fresh Warm, freq_rate substeps and Body::outputs per step); the real step is body_rollout_kernel's without observation noise
// (abi.hip refuses such a handle), and a reset is body_init of (reset key, global env index, episode) — what that kernel's spare
// state holds.  The planner stages are the lines of the 4-state kernels, copied rather than shared (as those copy the finish kernels of
// util_kernels.hip: their instruction streams must stay what they are).  No lane of an opted-in body reads another lane's data, so
// the lane a candidate runs on — here lane k % 64 of the env's wave, in body_plan_kernel lane (i * K + k) % 64 — does not enter its bits.
#pragma once

namespace emei {

template <class Body>
struct BodyMpcArgs {
    typename Body::real* state;  // SoA: NS arrays of n
    int32_t* steps;
    uint32_t* episode;
    const SinCosEntry* trig;
    unsigned long long* cap_hits;
    float* nominal;  // in/out [horizon, n, NA]
    double* work;    // [n, n_cand] returns, then weights / membership flags; word 0 of env i's row ends as its last done code (mpc_done_pack_kernel)
    float* actions_out;
    float* obs_out;
    float* reward_out;
    uint8_t* done_out;
    double* plan_return_out;
    double* ess_out;           // MPPI
    double* elite_return_out;  // CEM
    int64_t n;
    int32_t n_steps, horizon, n_cand, n_elites, iterations, freq_rate, max_episode_steps, semi;
    uint32_t flags;
    uint64_t reset_seed, env_offset, seed;
    double discount, temperature;
    float sigma, sigma_min, lo, hi, refill, nominal_lo, nominal_hi;
    NoiseArgs<Body::NS> noise;
    typename Body::Model m;
};

// Every lane scores its candidates k = lane, lane + 64, ... from the env's real state `s` (body_plan_kernel's DRAWN loop), keeps the
// returns in wt[] (8 B per candidate: no cap on n_candidates; a lane reads back only what it wrote) and folds the winner (ks, rs) in
// ascending k, then over the lanes — the planner's order is total, so this is plan_finish_kernel's winner.
template <class Body, bool RK4, class Spec>
__device__ __forceinline__ void body_mpc_score(const typename Body::real (&s)[Body::NS], const Spec& sp, uint64_t g, int lane,
                                               const BodyMpcArgs<Body>& a, const TrigCtx& trig, double* wt, double& rs, int32_t& ks) {
    using R = typename Body::real;
    constexpr int NS = Body::NS, NO = Body::NO, NA = Body::NA;
    rs = __builtin_nan("");  // (NaN, INT32_MAX) loses to every candidate
    ks = INT32_MAX;
    for (int32_t k0 = 0; k0 < a.n_cand; k0 += kWave) {  // wave-uniform trip count: every lane takes part in the ballot
        const int32_t k = k0 + lane;
        R cs[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) cs[q] = s[q];
        double ret = 0.0, gd = 1.0;
        bool live = k < a.n_cand;
        for (int32_t h = 0; h < a.horizon; ++h) {
            R ctrl[NA];
            CandidateWords cw(sp.seed, g, (uint32_t)k);
#pragma unroll
            for (int q = 0; q < NA; ++q) ctrl[q] = (R)draw_action(cw, sp, 1, 0, h, q, NA);
            R pre[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) pre[q] = cs[q];
            typename Body::Warm warm{};
            for (int f = 0; f < a.freq_rate; ++f) body_substep<Body, RK4>(cs, ctrl, a.m, a.semi != 0, trig, warm);
            float o[NO];
            R rew;
            bool term;
            Body::outputs(cs, pre, ctrl, a.m, a.freq_rate, o, rew, term, trig);
            if (live) {
                ret = ret + gd * (double)(float)rew;
                gd = gd * a.discount;
                if (term) live = false;
            }
            if (__ballot(live) == 0ull) break;  // wave-uniform
        }
        if (k < a.n_cand) {
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
}

// Act, step, auto-reset and warm start of control step t: the action is the mean's first entry; the real state takes
// body_rollout_kernel's step (TimeLimit and the done code as there; under auto-reset a done env starts its next episode from
// body_init); lane 0 stores the step's outputs — small uncoalesced stores, which is accepted: this path is bound by the latency of one
// wave's dependent arithmetic, not by HBM; then the mean is shifted by one step, or refilled after a reset.  -> the done code
template <class Body, bool RK4>
__device__ __forceinline__ uint32_t body_mpc_act_step(typename Body::real (&s)[Body::NS], int32_t& steps, uint32_t& episode, float* nom,
                                                      int32_t n_comp, int32_t t, int64_t i, uint64_t g, int lane,
                                                      const BodyMpcArgs<Body>& a, const TrigCtx& trig) {
    using R = typename Body::real;
    constexpr int NS = Body::NS, NO = Body::NO, NA = Body::NA;
    const int64_t at = (int64_t)t * a.n + i;
    R ctrl[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q) {
        const float av = nom[q];
        ctrl[q] = (R)av;
        if (lane == 0) a.actions_out[at * NA + q] = av;
    }
    R pre[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) pre[q] = s[q];
    typename Body::Warm warm{};
    for (int f = 0; f < a.freq_rate; ++f) body_substep<Body, RK4>(s, ctrl, a.m, a.semi != 0, trig, warm);
    float o[NO];
    R rew;
    bool term;
    Body::outputs(s, pre, ctrl, a.m, a.freq_rate, o, rew, term, trig);
    ++steps;
    const bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
    const uint32_t done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
    if (lane == 0) {
        if (a.obs_out) {
#pragma unroll
            for (int q = 0; q < NO; ++q) a.obs_out[at * NO + q] = o[q];
        }
        if (a.reward_out) a.reward_out[at] = (float)rew;
        if (a.done_out) a.done_out[at] = (uint8_t)done;
    }
    const bool reset_now = (a.flags & EMEI_FLAG_AUTO_RESET) != 0 && __builtin_amdgcn_readfirstlane(done) != 0u;  // wave-uniform
    if (reset_now) {
        ++episode;
        steps = 0;
        body_init<Body>(s, a.reset_seed, g, episode, a.noise);
    }
    // warm start, pass by pass in ascending order: a pass reads [base + NA, base + 64 + NA) and writes [base, base + 64)
    for (int32_t base = 0; base < n_comp; base += kWave) {
        const int32_t cc = base + lane;
        const float v = (!reset_now && cc + NA < n_comp) ? nom[cc + NA] : a.refill;
        wave_lds_fence();
        if (cc < n_comp) nom[cc] = v;
        wave_lds_fence();
    }
    return done;
}

// after the last control step: the mean goes back to global memory, lane 0 stores the state, the counters and the done code
template <class Body>
__device__ __forceinline__ void body_mpc_write_back(const typename Body::real (&s)[Body::NS], int32_t steps, uint32_t episode,
                                                    uint32_t done, const float* nom, int32_t n_comp, int64_t i, int lane, double* wt,
                                                    const BodyMpcArgs<Body>& a) {
    constexpr int NA = Body::NA;
    for (int32_t cc = lane; cc < n_comp; cc += kWave) a.nominal[((int64_t)(cc / NA) * a.n + i) * NA + cc % NA] = nom[cc];
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < Body::NS; ++q) a.state[(int64_t)q * a.n + i] = s[q];
        a.steps[i] = steps;
        a.episode[i] = episode;
        ((unsigned long long*)wt)[0] = (unsigned long long)done;  // lane 0's own slot, after its last use
    }
}

// Per control step: 1. the lanes clamp the nominal; 2. body_mpc_score; 3. weights, Z, the effective sample size and the weighted mean:
// pend_mpc_mppi_kernel's step 3 (plan_mppi_finish_kernel's lines), lane 0 writes the new nominal into LDS; 4., 5. body_mpc_act_step.
template <class Body, bool RK4>
__global__ void __launch_bounds__(kBlock) body_mpc_mppi_kernel(const BodyMpcArgs<Body> a) {
    static_assert(Body::kFusedMpc && Body::kScratchPerLane == 0, "a body without block scratch that opted in");
    using R = typename Body::real;
    constexpr int kWavesPerBlock = kBlock / kWave;
    constexpr int NS = Body::NS, na = Body::NA;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    __shared__ float nom_s[kWavesPerBlock][EMEI_MPC_MAX_HORIZON * na];
    stage_trig_table(trig_s, a.trig);
    TrigCtx trig;
    trig.tab = trig_s;
    trig.scratch_stride = kBlock;
    trig.cap_hits = a.cap_hits;
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wv;  // wave-uniform
    if (i >= a.n) return;
    const int64_t n = a.n;
    const int32_t n_cand = a.n_cand;
    const int32_t n_comp = a.horizon * na;  // <= EMEI_MPC_MAX_HORIZON * na (abi.hip)
    float* nom = nom_s[wv];
    for (int32_t c = lane; c < n_comp; c += kWave) nom[c] = a.nominal[((int64_t)(c / na) * n + i) * na + c % na];

    R s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = a.state[(int64_t)k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
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
        double rs;
        int32_t ks;
        body_mpc_score<Body, RK4>(s, sp, g, lane, a, trig, wt, rs, ks);
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
                CandidateWords cw(sp.seed, g, (uint32_t)k);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int32_t cc = min(c0 + u, n_comp - 1);  // past the end: the last component again, dropped below
                    const float v = draw_action(cw, sp, 1, 0, cc / na, cc % na, na);
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
        // 4., 5.
        done = body_mpc_act_step<Body, RK4>(s, steps, episode, nom, n_comp, t, i, g, lane, a, trig);
    }
    body_mpc_write_back<Body>(s, steps, episode, done, nom, n_comp, i, lane, wt, a);
}

// Per control step, `iterations` times: (a, b) the lanes clamp the mean and, in the first iteration, set the sigma slice to the
// scalar; (c) body_mpc_score, then the elite set and its moments: pend_mpc_cem_kernel's lines (plan_cem_finish_kernel's: the MSB-first
// radix select over plan_key with 256 LDS counters per wave, membership row by row with ties to the lower k, the members alone redrawn
// for the shifted moments), lane 0 writes mean and sigma into LDS behind a fence; (d) the lanes floor the sigma.  Then
// body_mpc_act_step.  The counters are per wave, and a wave's LDS operations — the ds_add of the histogram included — execute in
// order: wave_lds_fence() where plan_cem_finish_kernel has a block barrier.
template <class Body, bool RK4>
__global__ void __launch_bounds__(kBlock) body_mpc_cem_kernel(const BodyMpcArgs<Body> a) {
    static_assert(Body::kFusedMpc && Body::kScratchPerLane == 0, "a body without block scratch that opted in");
    using R = typename Body::real;
    constexpr int kWavesPerBlock = kBlock / kWave;
    constexpr int NS = Body::NS, na = Body::NA;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    __shared__ float nom_s[kWavesPerBlock][EMEI_MPC_MAX_HORIZON * na];
    __shared__ float sig_s[kWavesPerBlock][EMEI_MPC_MAX_HORIZON * na];
    __shared__ uint32_t hist_s[kWavesPerBlock][256];
    stage_trig_table(trig_s, a.trig);
    TrigCtx trig;
    trig.tab = trig_s;
    trig.scratch_stride = kBlock;
    trig.cap_hits = a.cap_hits;
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wv;  // wave-uniform
    if (i >= a.n) return;
    const int64_t n = a.n;
    const int32_t n_cand = a.n_cand;
    const int32_t n_comp = a.horizon * na;  // <= EMEI_MPC_MAX_HORIZON * na (abi.hip)
    float* nom = nom_s[wv];
    float* sig = sig_s[wv];
    uint32_t* hist = hist_s[wv];
    for (int32_t c = lane; c < n_comp; c += kWave) nom[c] = a.nominal[((int64_t)(c / na) * n + i) * na + c % na];

    R s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = a.state[(int64_t)k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    const uint64_t g = a.env_offset + (uint64_t)i;
    double* wt = a.work + i * n_cand;
    CandidateSpecLdsMap sp;
    sp.env_offset = a.env_offset;
    sp.nominal.p = (const __attribute__((address_space(3))) float*)nom;
    sp.sigma_map.p = (const __attribute__((address_space(3))) float*)sig;
    sp.lo = a.lo, sp.hi = a.hi;
    const double m_el = (double)a.n_elites;
    uint32_t done = 0;

    for (int32_t t = 0; t < a.n_steps; ++t) {
        for (int32_t it = 0; it < a.iterations; ++it) {
            // (a), (b)
            for (int32_t cc = lane; cc < n_comp; cc += kWave) {
                nom[cc] = fminf(fmaxf(nom[cc], a.nominal_lo), a.nominal_hi);
                if (it == 0) sig[cc] = a.sigma;
            }
            wave_lds_fence();
            // (c) the returns and (k*, r*)
            sp.seed = a.seed + (uint64_t)t * (uint64_t)a.iterations + (uint64_t)it;
            double rs;
            int32_t ks;
            body_mpc_score<Body, RK4>(s, sp, g, lane, a, trig, wt, rs, ks);
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
                    m0[u] = (double)nom[cc];
                }
                for (int32_t k = lane; k < n_cand; k += kWave) {
                    if (wt[k] == 0.0) continue;  // no draw for a candidate outside the set
                    CandidateWords cw(sp.seed, g, (uint32_t)k);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int32_t cc = min(c0 + u, n_comp - 1);
                        const double d = (double)draw_action(cw, sp, 1, 0, cc / na, cc % na, na) - m0[u];
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
                        sig[cc] = (float)sqrt(fmax(s2[u] / m_el - mu * mu, 0.0));
                    }
                }
            }
            wave_lds_fence();  // lane 0's mean and sigma are what every lane reads from here on
            // (d)
            for (int32_t cc = lane; cc < n_comp; cc += kWave) sig[cc] = fmaxf(sig[cc], a.sigma_min);
            wave_lds_fence();
        }
        done = body_mpc_act_step<Body, RK4>(s, steps, episode, nom, n_comp, t, i, g, lane, a, trig);
    }
    body_mpc_write_back<Body>(s, steps, episode, done, nom, n_comp, i, lane, wt, a);
}

// ---------------------------------------------------------------------------------------------
// emei_mpc_policy for the opted-in bodies: the skeleton above around emei_plan_policy.  No nominal: nothing in LDS beyond the trig table.
template <class Body>
struct BodyMpcPolicyArgs {
    typename Body::real* state;  // SoA: NS arrays of n
    int32_t* steps;
    uint32_t* episode;
    const SinCosEntry* trig;
    unsigned long long* cap_hits;
    double* work;  // [n, n_cand] returns, then [n, n_cand] float32 first actions; word 0 of env i's row of returns ends as its last
                   // done code (mpc_done_pack_kernel)
    float* actions_out;
    float* obs_out;
    float* reward_out;
    uint8_t* done_out;
    double* plan_return_out;
    int32_t* plan_index_out;
    double* ess_out;
    int64_t n;
    int32_t n_steps, horizon, n_cand, freq_rate, max_episode_steps, semi, act_mode;
    uint32_t flags;
    uint64_t reset_seed, env_offset, seed_stride;
    double discount, temperature;
    NoiseArgs<Body::NS> noise;
    typename Body::Model m;
};

// Per control step t, under the key key_t = nz.seed + t * seed_stride:
//   1., 2. every lane scores its candidates with body_policy_plan_kernel's loop, expression for expression — x_0 is the float32
//      observation of the state (Body::obs_of, as emei_get_obs rounds it), formed in front of the loop and at the end of every
//      control step, behind the reset; the
//      action of step 0 from x_0 under key_t, the action of step h + 1 from the row step h emits under key_t + h + 1, the lane's k in the counter word, no
//      noise for k = 0, the weights wave-uniform scalar loads; a fresh Warm, freq_rate substeps and Body::outputs per step;
//      ret = ret + g * (double)(float)rew — keeps its return and its action of step 0 in `work` (a lane reads back only what it
//      wrote) and folds (k*, r*, a*) in ascending k, then over the lanes;
//   3. with ACT_MEAN or an ess_out (wave-uniform): plan_policy_finish_kernel<true>'s lines, copied rather than shared;
//   4. the action — the winner's, or the mean — then body_mpc_act_step's step part: body_rollout_kernel's step without observation
//      noise, TimeLimit, and body_init of (reset key, global env index, episode) under auto-reset; lane 0 stores the outputs.
template <class Body, bool RK4>
__global__ void __launch_bounds__(kBlock)
    body_mpc_policy_kernel(const BodyMpcPolicyArgs<Body> a, const PolicyArgs pol, const PolicyNoiseArgs nz) {
    static_assert(Body::kFusedMpc && Body::kScratchPerLane == 0, "a body without block scratch that opted in");
    static_assert(Body::NA == 1, "one float32 first-action slot per candidate (abi.hip sizes the workspace)");
    using R = typename Body::real;
    constexpr int kWavesPerBlock = kBlock / kWave;
    constexpr int NS = Body::NS, NO = Body::NO, NA = Body::NA;
    __shared__ SinCosEntry trig_s[kTrigTableSize];
    stage_trig_table(trig_s, a.trig);
    TrigCtx trig;
    trig.tab = trig_s;
    trig.scratch_stride = kBlock;
    trig.cap_hits = a.cap_hits;
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wv;  // wave-uniform
    if (i >= a.n) return;
    const int64_t n = a.n;
    const int32_t n_cand = a.n_cand;

    R s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = a.state[(int64_t)k * n + i];
    int32_t steps = a.steps[i];
    uint32_t episode = a.episode[i];
    const bool weighted = a.act_mode == EMEI_MPC_POLICY_ACT_MEAN || a.ess_out != nullptr;  // wave-uniform
    const uint64_t g = a.env_offset + (uint64_t)i;
    double* wt = a.work + i * n_cand;
    float* fa = (float*)(a.work + n * n_cand) + i * n_cand;  // the env's first actions
    uint32_t done = 0;
    // x_0 of the first control step; every later one observes at the end of the step in front of it, behind the reset
    float x0[NO];
    {
        double od[NO];
        Body::obs_of(s, od, a.m);
#pragma unroll
        for (int q = 0; q < NO; ++q) x0[q] = (float)od[q];
    }

    for (int32_t t = 0; t < a.n_steps; ++t) {
        // 1., 2.
        const uint64_t key_t = nz.seed + (uint64_t)t * a.seed_stride;
        double rs = __builtin_nan("");  // (NaN, INT32_MAX) loses to every candidate
        int32_t ks = INT32_MAX;
        float as = 0.f;
        for (int32_t k0 = 0; k0 < n_cand; k0 += kWave) {  // wave-uniform trip count: every lane takes part in the ballot
            const int32_t k = k0 + lane;
            R cs[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) cs[q] = s[q];
            float act[NA];
            policy_eval_t<NO, NA, false, true>(pol, nz, key_t, g, x0, act, (uint32_t)k, k != 0);
            const float first = act[0];
            double ret = 0.0, gd = 1.0;
            bool live = k < n_cand;
            for (int32_t h = 0; h < a.horizon; ++h) {
                R ctrl[NA];
#pragma unroll
                for (int q = 0; q < NA; ++q) ctrl[q] = (R)act[q];
                R pre[NS];
#pragma unroll
                for (int q = 0; q < NS; ++q) pre[q] = cs[q];
                typename Body::Warm warm{};
                for (int f = 0; f < a.freq_rate; ++f) body_substep<Body, RK4>(cs, ctrl, a.m, a.semi != 0, trig, warm);
                float o[NO];
                R rew;
                bool term;
                Body::outputs(cs, pre, ctrl, a.m, a.freq_rate, o, rew, term, trig);
                if (live) {
                    ret = ret + gd * (double)(float)rew;
                    gd = gd * a.discount;
                    if (term) live = false;
                }
                if (__ballot(live) == 0ull || h == a.horizon - 1) break;  // wave-uniform
                policy_eval_t<NO, NA, false, true>(pol, nz, key_t + (uint64_t)h + 1u, g, o, act, (uint32_t)k, k != 0);  // the next step's action
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
        const int64_t at = (int64_t)t * n + i;
        if (lane == 0) {
            if (a.plan_return_out) a.plan_return_out[at] = rs;
            if (a.plan_index_out) a.plan_index_out[at] = ks;
        }
        // 4.
        const float av = a.act_mode == EMEI_MPC_POLICY_ACT_MEAN ? mean : as;  // wave-uniform
        R ctrl[NA] = {(R)av};
        if (lane == 0) a.actions_out[at] = av;
        R pre[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) pre[q] = s[q];
        typename Body::Warm warm{};
        for (int f = 0; f < a.freq_rate; ++f) body_substep<Body, RK4>(s, ctrl, a.m, a.semi != 0, trig, warm);
        float o[NO];
        R rew;
        bool term;
        Body::outputs(s, pre, ctrl, a.m, a.freq_rate, o, rew, term, trig);
        ++steps;
        const bool trunc = (a.max_episode_steps > 0) & (steps >= a.max_episode_steps);
        done = (term ? EMEI_DONE_TERMINAL : 0u) | (trunc ? EMEI_DONE_TRUNCATED : 0u);
        if (lane == 0) {
            if (a.obs_out) {
#pragma unroll
                for (int q = 0; q < NO; ++q) a.obs_out[at * NO + q] = o[q];
            }
            if (a.reward_out) a.reward_out[at] = (float)rew;
            if (a.done_out) a.done_out[at] = (uint8_t)done;
        }
        const bool reset_now = (a.flags & EMEI_FLAG_AUTO_RESET) != 0 && __builtin_amdgcn_readfirstlane(done) != 0u;  // wave-uniform
        if (reset_now) {
            ++episode;
            steps = 0;
            body_init<Body>(s, a.reset_seed, g, episode, a.noise);
        }
        {  // the next control step's x_0
            double od[NO];
            Body::obs_of(s, od, a.m);
#pragma unroll
            for (int q = 0; q < NO; ++q) x0[q] = (float)od[q];
        }
    }

    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) a.state[(int64_t)q * n + i] = s[q];
        a.steps[i] = steps;
        a.episode[i] = episode;
        ((unsigned long long*)wt)[0] = (unsigned long long)done;  // lane 0's own slot, after its last use
    }
}

// the one launch of emei_mpc_policy's body route (OP_MPC_POLICY), one wave per env
template <class Body>
static int launch_body_mpc_policy(const BodyLaunch& L, const typename Body::Model& m) {
    const MpcLaunch& M = L.mpc;
    if (M.horizon < 1 || L.plan.n_candidates < 1 || !L.plan.return_out || !M.actions_out) return EMEI_ERR_INVALID;
    if (NoiseArgs<Body::NS>(L.noise).obs_on) return EMEI_ERR_UNSUPPORTED;  // the plan's model steps without observation noise
    BodyMpcPolicyArgs<Body> a;
    a.state = (typename Body::real*)L.state, a.steps = L.steps, a.episode = L.episode;
    a.trig = (const SinCosEntry*)L.trig, a.cap_hits = L.cap_hits;
    a.work = L.plan.return_out, a.actions_out = (float*)M.actions_out;
    a.obs_out = L.obs_out, a.reward_out = L.reward_out, a.done_out = L.done_out;
    a.plan_return_out = M.plan_return_out, a.plan_index_out = M.plan_index_out, a.ess_out = M.ess_out;
    a.n = L.n, a.n_steps = L.n_steps, a.horizon = M.horizon, a.n_cand = L.plan.n_candidates;
    a.freq_rate = L.freq_rate, a.max_episode_steps = L.max_episode_steps;
    a.semi = L.integrator == EMEI_INTEG_SEMI_IMPLICIT, a.act_mode = M.act_mode, a.flags = L.flags;
    a.reset_seed = L.seed, a.env_offset = L.env_offset, a.seed_stride = M.seed_stride;
    a.discount = L.plan.discount, a.temperature = M.temperature;
    a.noise = NoiseArgs<Body::NS>(L.noise), a.m = m;
    constexpr int kWavesPerBlock = kBlock / kWave;
    const dim3 mgrid((unsigned)((L.n + kWavesPerBlock - 1) / kWavesPerBlock));
    if (L.integrator == EMEI_INTEG_RK4)
        hipLaunchKernelGGL((body_mpc_policy_kernel<Body, true>), mgrid, dim3(kBlock), 0, L.stream, a, L.policy, L.policy_noise);
    else
        hipLaunchKernelGGL((body_mpc_policy_kernel<Body, false>), mgrid, dim3(kBlock), 0, L.stream, a, L.policy, L.policy_noise);
    if (L.selected) *L.selected = EMEI_KERNEL_BODY_MPC_POLICY;
    return EMEI_OK;
}

// the one launch of either controller (OP_MPC_MPPI / OP_MPC_CEM), one wave per env
template <class Body>
static int launch_body_mpc(const BodyLaunch& L, const typename Body::Model& m) {
    const MpcLaunch& M = L.mpc;
    const bool cem = L.op == OP_MPC_CEM;
    if (M.horizon < 1 || M.horizon > EMEI_MPC_MAX_HORIZON) return EMEI_ERR_INVALID;  // the LDS slices of the mean and the sigma
    if (cem && (M.iterations < 1 || M.n_elites < 1 || M.n_elites > L.plan.n_candidates)) return EMEI_ERR_INVALID;
    if (NoiseArgs<Body::NS>(L.noise).obs_on) return EMEI_ERR_UNSUPPORTED;  // the plan's model steps without observation noise
    BodyMpcArgs<Body> a;
    a.state = (typename Body::real*)L.state, a.steps = L.steps, a.episode = L.episode;
    a.trig = (const SinCosEntry*)L.trig, a.cap_hits = L.cap_hits;
    a.nominal = M.nominal, a.work = L.plan.return_out, a.actions_out = (float*)M.actions_out;
    a.obs_out = L.obs_out, a.reward_out = L.reward_out, a.done_out = L.done_out;
    a.plan_return_out = M.plan_return_out, a.ess_out = M.ess_out, a.elite_return_out = M.elite_return_out;
    a.n = L.n, a.n_steps = L.n_steps, a.horizon = M.horizon, a.n_cand = L.plan.n_candidates;
    a.n_elites = M.n_elites, a.iterations = M.iterations, a.freq_rate = L.freq_rate, a.max_episode_steps = L.max_episode_steps;
    a.semi = L.integrator == EMEI_INTEG_SEMI_IMPLICIT, a.flags = L.flags;
    a.reset_seed = L.seed, a.env_offset = L.env_offset, a.seed = L.plan.cand.seed;
    a.discount = L.plan.discount, a.temperature = M.temperature;
    a.sigma = L.plan.cand.sigma, a.sigma_min = M.sigma_min, a.lo = L.plan.cand.lo, a.hi = L.plan.cand.hi;
    a.refill = M.refill, a.nominal_lo = M.nominal_lo, a.nominal_hi = M.nominal_hi;
    a.noise = NoiseArgs<Body::NS>(L.noise), a.m = m;
    constexpr int kWavesPerBlock = kBlock / kWave;
    const dim3 mgrid((unsigned)((L.n + kWavesPerBlock - 1) / kWavesPerBlock));
    const bool rk4 = L.integrator == EMEI_INTEG_RK4;
    if (cem) {
        if (rk4) hipLaunchKernelGGL((body_mpc_cem_kernel<Body, true>), mgrid, dim3(kBlock), 0, L.stream, a);
        else hipLaunchKernelGGL((body_mpc_cem_kernel<Body, false>), mgrid, dim3(kBlock), 0, L.stream, a);
    } else {
        if (rk4) hipLaunchKernelGGL((body_mpc_mppi_kernel<Body, true>), mgrid, dim3(kBlock), 0, L.stream, a);
        else hipLaunchKernelGGL((body_mpc_mppi_kernel<Body, false>), mgrid, dim3(kBlock), 0, L.stream, a);
    }
    if (L.selected) *L.selected = cem ? EMEI_KERNEL_BODY_MPC_CEM : EMEI_KERNEL_BODY_MPC_MPPI;
    return EMEI_OK;
}

}  // namespace emei
