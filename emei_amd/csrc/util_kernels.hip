// util_kernels.hip — state marshalling and wavefront-ballot compaction of done envs (gfx950).
#include "launch.h"

namespace emei {

// [n,dim] float64 row-major (the reference's `self.state` rows) -> SoA of R
template <typename R>
__global__ void __launch_bounds__(kBlock) state_unpack_kernel(const double* aos, R* soa, int64_t n, int dim) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < dim; ++k) soa[(int64_t)k * n + i] = (R)aos[i * dim + k];
}
template <typename R>
__global__ void __launch_bounds__(kBlock) state_pack_kernel(const R* soa, double* aos, int64_t n, int dim) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < dim; ++k) aos[i * dim + k] = (double)soa[(int64_t)k * n + i];
}

int launch_state_unpack(const double* aos, void* soa, int precision, int64_t n, int dim, hipStream_t s) {
    dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (precision == EMEI_PRECISION_F32)
        hipLaunchKernelGGL(state_unpack_kernel<float>, grid, dim3(kBlock), 0, s, aos, (float*)soa, n, dim);
    else
        hipLaunchKernelGGL(state_unpack_kernel<double>, grid, dim3(kBlock), 0, s, aos, (double*)soa, n, dim);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}
int launch_state_pack(const void* soa, double* aos, int precision, int64_t n, int dim, hipStream_t s) {
    dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (precision == EMEI_PRECISION_F32)
        hipLaunchKernelGGL(state_pack_kernel<float>, grid, dim3(kBlock), 0, s, (const float*)soa, aos, n, dim);
    else
        hipLaunchKernelGGL(state_pack_kernel<double>, grid, dim3(kBlock), 0, s, (const double*)soa, aos, n, dim);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------
// Compaction.  The step kernels leave one ballot word per wave (bit b = env 64*w+b is done).  A
// single 1024-thread workgroup turns those words into the SORTED list of done env indices:
// popcount -> workgroup exclusive scan -> every wave expands 64 mask words cooperatively, lane b
// writing env 64*w+b at offset + popcount(mask & lanes_below(b)), so the index stores of one mask
// word are contiguous.  Deterministic (no atomics); output is ascending.
constexpr int kCompactBlock = 1024;

__global__ void __launch_bounds__(kCompactBlock)
    compact_done_kernel(const unsigned long long* masks, int64_t n_words, int64_t n_envs, int32_t* idx_out,
                        int32_t* count_out) {
    __shared__ int wave_tot[kCompactBlock / kWave];
    __shared__ int running_s;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    if (tid == 0) running_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_words; base += kCompactBlock) {
        const int64_t w = base + tid;
        unsigned long long m = (w < n_words) ? masks[w] : 0ull;
        // the last word may carry lanes beyond n_envs only as zeros (inactive lanes never ballot)
        int cnt = __popcll(m);
        // inclusive scan inside the wave
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == kWave - 1) wave_tot[wv] = incl;
        __syncthreads();
        int wave_base = 0, block_tot = 0;
        for (int k = 0; k < kCompactBlock / kWave; ++k) {
            int t = wave_tot[k];
            if (k < wv) wave_base += t;
            block_tot += t;
        }
        const int running = running_s;
        int off = running + wave_base + incl - cnt;  // exclusive offset of this lane's word
        // cooperative expansion: word k of this wave is handled by all 64 lanes
        for (int k = 0; k < kWave; ++k) {
            unsigned long long mk = __shfl(m, k);
            if (mk == 0ull) continue;  // wave-uniform
            int offk = __shfl(off, k);
            int64_t wk = base + (int64_t)wv * kWave + k;
            if ((mk >> lane) & 1ull) {
                int pos = __popcll(mk & ((1ull << lane) - 1ull));
                idx_out[offk + pos] = (int32_t)(wk * kWave + lane);
            }
        }
        __syncthreads();
        if (tid == 0) running_s = running + block_tot;
        __syncthreads();
    }
    if (tid == 0) *count_out = running_s;
    (void)n_envs;
}

int launch_compact_done(const unsigned long long* masks, int64_t n, int32_t* idx_out, int32_t* count_out,
                        hipStream_t s) {
    int64_t n_words = (n + kWave - 1) / kWave;
    hipLaunchKernelGGL(compact_done_kernel, dim3(1), dim3(kCompactBlock), 0, s, masks, n_words, n, idx_out, count_out);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}

// emei_mpc_mppi keeps one wave per env, so no wave holds the done bits of 64 envs: its kernel leaves env i's last done code in word 0
// of the env's workspace row, and this follow-up launch ballots them into the mask words emei_compact_done reads (no atomics).
__global__ void __launch_bounds__(kBlock)
    mpc_done_pack_kernel(const unsigned long long* work, int64_t stride, int64_t n, unsigned long long* done_mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool done = i < n && work[i * stride] != 0ull;  // lanes past n ballot zeros
    const unsigned long long m = __ballot(done);
    if (i < n && (threadIdx.x & (kWave - 1)) == 0) done_mask[i / kWave] = m;
}

int launch_mpc_done_pack(const double* work, int64_t stride, int64_t n, unsigned long long* done_mask, hipStream_t s) {
    dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(mpc_done_pack_kernel, grid, dim3(kBlock), 0, s, (const unsigned long long*)work, stride, n, done_mask);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------
// emei_sample_candidates: lane j writes the sequence of candidate (i = j / K, k = j % K) — what the plan kernels draw in their
// lanes (emei_device.h:draw_action) — step by step, the stores of a step contiguous over the lanes.
template <class Spec>
__global__ void __launch_bounds__(kBlock)
    sample_candidates_kernel(Spec sp, int64_t n_envs, int32_t n_cand, int32_t horizon, int act_dim, void* out, int action_dtype) {
    const int64_t nk = n_envs * n_cand;
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nk) return;
    const int64_t i = j / n_cand;
    const int na = act_dim > 0 ? act_dim : 1;
    CandidateWords cw(sp.seed, sp.env_offset + (uint64_t)i, (uint32_t)(j - i * n_cand));
    for (int32_t t = 0; t < horizon; ++t)
        for (int a = 0; a < na; ++a) store_action(out, action_dtype, ((int64_t)t * nk + j) * na + a, draw_action(cw, sp, n_envs, i, t, a, act_dim));
}

// Second launch of emei_plan_shooting, one wave per env: the best of the env's partials (slots w + i of the waves w its
// candidates lay on; the order is total, so the lanes' strided pass and the butterfly give the first maximum), then candidate k*'s
// sequence drawn again, the lanes striding over the steps.
__global__ void __launch_bounds__(kBlock)
    plan_finish_kernel(const PlanPartial* partials, CandidateSpec sp, int64_t n_envs, int32_t n_cand, int32_t horizon, int act_dim,
                       void* best_action, int action_dtype, void* best_sequence, double* best_return, int32_t* best_index,
                       int32_t* best_length) {
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;  // wave-uniform
    const int lane = (int)(threadIdx.x & (kWave - 1));
    if (i >= n_envs) return;
    const int64_t w0 = (i * n_cand) / kWave, w1 = ((i + 1) * n_cand - 1) / kWave;
    // (NaN, INT32_MAX) loses to every partial: k < n_cand <= 2^31 - 1
    double ret = __builtin_nan("");
    int32_t k = INT32_MAX, len = 0;
    for (int64_t w = w0 + lane; w <= w1; w += kWave) {
        const PlanPartial p = partials[w + i];
        if (plan_replaces(ret, k, p.ret, p.k)) ret = p.ret, k = p.k, len = p.len;
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double r2 = __shfl_xor(ret, d, kWave);
        const int32_t k2 = __shfl_xor(k, d, kWave), l2 = __shfl_xor(len, d, kWave);
        if (plan_replaces(ret, k, r2, k2)) ret = r2, k = k2, len = l2;
    }
    if (lane == 0) {
        best_return[i] = ret;
        best_index[i] = k;
        if (best_length) best_length[i] = len;
    }
    const int na = act_dim > 0 ? act_dim : 1;
    for (int32_t t = lane; t < horizon; t += kWave) {
        CandidateWords cw(sp.seed, sp.env_offset + (uint64_t)i, (uint32_t)k);
        for (int a = 0; a < na; ++a) {
            const float v = draw_action(cw, sp, n_envs, i, t, a, act_dim);
            if (best_sequence) store_action(best_sequence, action_dtype, ((int64_t)t * n_envs + i) * na + a, v);
            if (t == 0) store_action(best_action, action_dtype, i * na + a, v);
        }
    }
}

// Second launch of emei_plan_mppi, one wave per env, lane l owning the candidates k = l, l + 64, ...:
//   1. (k*, r*) from the env's partials, as plan_finish_kernel finds them;
//   2. the lane turns its candidates' returns (left by the plan kernel, 8 B each) into the weights of the header's case analysis
//      and writes them back over the returns — it is the only reader of what it wrote, so nothing has to become visible to another
//      lane — and Z = sum w, sum w^2 are reduced;
//   3. the word stream is walked one Philox block at a time: block b carries the components c = 4b .. 4b + 3 (c = t * act_dim + a;
//      four coin flips, four uniforms or two Box-Muller pairs: draw_action reads W[c] or the pair (W[c & ~1], W[c | 1]), inside
//      block c >> 2 either way), the lane redraws them for each of its candidates through draw_action — each Philox block of each
//      candidate once — and accumulates four weighted float64 sums, the wave reduces them and lane 0 stores the four means.
// Summation order (the reproducibility clause): a lane adds its candidates in ascending k, the butterfly adds lanes l and l ^ d for
// d = 1, 2, .., 32 — a tree over k alone, whatever n_envs, the shard or the first launch's waves were.
// In place (nominal_out == sp.nominal): entry (t, i, a) is read by this wave in block c >> 2 only, before the block's stores, and
// belongs to no other wave.
__global__ void __launch_bounds__(kBlock)
    plan_mppi_finish_kernel(const PlanPartial* partials, double* returns, CandidateSpec sp, int64_t n_envs, int32_t n_cand, int32_t horizon,
                            int act_dim, double temperature, float* nominal_out, double* best_return, int32_t* best_index, double* ess) {
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;  // wave-uniform
    const int lane = (int)(threadIdx.x & (kWave - 1));
    if (i >= n_envs) return;
    const int64_t w0 = (i * n_cand) / kWave, w1 = ((i + 1) * n_cand - 1) / kWave;
    double rs = __builtin_nan("");  // (NaN, INT32_MAX) loses to every partial
    int32_t ks = INT32_MAX;
    for (int64_t w = w0 + lane; w <= w1; w += kWave) {
        const PlanPartial p = partials[w + i];
        if (plan_replaces(rs, ks, p.ret, p.k)) rs = p.ret, ks = p.k;
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double r2 = __shfl_xor(rs, d, kWave);
        const int32_t k2 = __shfl_xor(ks, d, kWave);
        if (plan_replaces(rs, ks, r2, k2)) rs = r2, ks = k2;
    }
    double* wt = returns + i * n_cand;
    double z = 0.0, z2 = 0.0;
    for (int32_t k = lane; k < n_cand; k += kWave) {
        const double r = wt[k];
        const double e = exp((r - rs) / temperature);  // r < r*: the argument is negative, -inf included
        const double w = rs != rs ? 1.0 : (r != r ? 0.0 : (r == rs ? 1.0 : e));
        wt[k] = w;
        z += w, z2 += w * w;
    }
    z = wave_sum_all(z), z2 = wave_sum_all(z2);  // Z >= 1: candidate k* has weight 1
    if (lane == 0) {
        if (best_return) best_return[i] = rs;
        if (best_index) best_index[i] = ks;
        if (ess) ess[i] = z * z / z2;
    }
    const int na = act_dim > 0 ? act_dim : 1;
    const int32_t n_comp = horizon * na;  // <= 2^31 - 1 (abi.hip:check_candidates)
    for (int32_t c0 = 0; c0 < n_comp; c0 += 4) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int32_t k = lane; k < n_cand; k += kWave) {
            const double w = wt[k];
            CandidateWords cw(sp.seed, sp.env_offset + (uint64_t)i, (uint32_t)k);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t c = min(c0 + u, n_comp - 1);  // past the end: the last component again, dropped below
                const float v = draw_action(cw, sp, n_envs, i, c / na, c % na, act_dim);
                acc[u] += w * (double)v;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = wave_sum_all(acc[u]);
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t c = c0 + u;
                if (c < n_comp) nominal_out[((int64_t)(c / na) * n_envs + i) * na + c % na] = (float)(acc[u] / z);
            }
        }
    }
}

// Second launch of emei_plan_policy, one wave per env, lane l owning the candidates k = l, l + 64, ... (plan_mppi_finish_kernel's
// layout and summation tree).  The candidates' returns and their actions of step 0 are where the policy plan kernel left them, so
// nothing is redrawn and no policy is evaluated here:
//   1. (k*, r*, L) from the env's partials, as plan_finish_kernel finds them; best_action is candidate k*'s stored action;
//   2. WEIGHTED (mean_out or ess wanted): the weights of emei_plan_mppi's case analysis, Z = sum w, sum w^2 and one weighted sum per
//      action component, a lane's candidates in ascending k, then the butterfly — a tree over k alone.
// `returns` and `first` are read only (returns may be the caller's return_out).
template <bool WEIGHTED>
__global__ void __launch_bounds__(kBlock)
    plan_policy_finish_kernel(const PlanPartial* partials, const double* returns, const float* first, int64_t n_envs, int32_t n_cand,
                              int act_dim, double temperature, void* best_action, int action_dtype, float* mean_out, double* best_return,
                              int32_t* best_index, int32_t* best_length, double* ess) {
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;  // wave-uniform
    const int lane = (int)(threadIdx.x & (kWave - 1));
    if (i >= n_envs) return;
    const int64_t w0 = (i * n_cand) / kWave, w1 = ((i + 1) * n_cand - 1) / kWave;
    double rs = __builtin_nan("");  // (NaN, INT32_MAX) loses to every partial
    int32_t ks = INT32_MAX, len = 0;
    for (int64_t w = w0 + lane; w <= w1; w += kWave) {
        const PlanPartial p = partials[w + i];
        if (plan_replaces(rs, ks, p.ret, p.k)) rs = p.ret, ks = p.k, len = p.len;
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double r2 = __shfl_xor(rs, d, kWave);
        const int32_t k2 = __shfl_xor(ks, d, kWave), l2 = __shfl_xor(len, d, kWave);
        if (plan_replaces(rs, ks, r2, k2)) rs = r2, ks = k2, len = l2;
    }
    const int na = act_dim > 0 ? act_dim : 1;
    const float* fa = first + i * n_cand * na;  // the env's [n_cand, na] actions of step 0
    if (lane == 0) {
        if (best_return) best_return[i] = rs;
        if (best_index) best_index[i] = ks;
        if (best_length) best_length[i] = len;
    }
    if (lane < na) store_action(best_action, action_dtype, i * na + lane, fa[(int64_t)ks * na + lane]);
    if constexpr (WEIGHTED) {
        const double* rt = returns + i * n_cand;
        double z = 0.0, z2 = 0.0, acc[kPlanPolicyMaxAct] = {};
        for (int32_t k = lane; k < n_cand; k += kWave) {
            const double r = rt[k];
            const double e = exp((r - rs) / temperature);  // r < r*: the argument is negative, -inf included
            const double w = rs != rs ? 1.0 : (r != r ? 0.0 : (r == rs ? 1.0 : e));
            z += w, z2 += w * w;
#pragma unroll
            for (int a = 0; a < kPlanPolicyMaxAct; ++a)
                if (a < na) acc[a] += w * (double)fa[(int64_t)k * na + a];
        }
        z = wave_sum_all(z), z2 = wave_sum_all(z2);  // Z >= 1: candidate k* has weight 1
#pragma unroll
        for (int a = 0; a < kPlanPolicyMaxAct; ++a) {
            if (a < na) {  // wave-uniform
                const double sum = wave_sum_all(acc[a]);
                if (lane == 0 && mean_out) mean_out[i * na + a] = (float)(sum / z);
            }
        }
        if (lane == 0 && ess) ess[i] = z * z / z2;
    }
}

int launch_plan_policy_finish(const void* partials, const double* returns, const float* first, int64_t n_envs, int32_t n_cand, int act_dim,
                              double temperature, void* best_action, int action_dtype, float* mean_out, double* best_return,
                              int32_t* best_index, int32_t* best_length, double* ess, hipStream_t s) {
    if (act_dim > kPlanPolicyMaxAct) return EMEI_ERR_INVALID;
    constexpr int kEnvsPerBlock = kBlock / kWave;  // one wave per env
    dim3 grid((unsigned)((n_envs + kEnvsPerBlock - 1) / kEnvsPerBlock));
    if (mean_out || ess)
        hipLaunchKernelGGL(plan_policy_finish_kernel<true>, grid, dim3(kBlock), 0, s, (const PlanPartial*)partials, returns, first, n_envs,
                           n_cand, act_dim, temperature, best_action, action_dtype, mean_out, best_return, best_index, best_length, ess);
    else
        hipLaunchKernelGGL(plan_policy_finish_kernel<false>, grid, dim3(kBlock), 0, s, (const PlanPartial*)partials, returns, first, n_envs,
                           n_cand, act_dim, temperature, best_action, action_dtype, mean_out, best_return, best_index, best_length, ess);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------
// emei_plan_cem (the planner's order as a 64-bit key: emei_device.h:plan_key).

// (k*, r*) of env i from its partials (slots w + i of the waves w its candidates lay on), as plan_finish_kernel finds them: the
// lanes' strided pass, then the butterfly; every lane of the wave ends with the winner.  (plan_mppi_finish_kernel keeps the same lines
// inline: called through here hipcc schedules that kernel differently, and DESIGN §4's measurements are of the code as it stands.)
__device__ __forceinline__ void plan_winner(const PlanPartial* partials, int64_t i, int32_t n_cand, int lane, double& rs, int32_t& ks) {
    const int64_t w0 = (i * n_cand) / kWave, w1 = ((i + 1) * n_cand - 1) / kWave;
    rs = __builtin_nan("");  // (NaN, INT32_MAX) loses to every partial
    ks = INT32_MAX;
    for (int64_t w = w0 + lane; w <= w1; w += kWave) {
        const PlanPartial p = partials[w + i];
        if (plan_replaces(rs, ks, p.ret, p.k)) rs = p.ret, ks = p.k;
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double r2 = __shfl_xor(rs, d, kWave);
        const int32_t k2 = __shfl_xor(ks, d, kWave);
        if (plan_replaces(rs, ks, r2, k2)) rs = r2, ks = k2;
    }
}

// Second launch of emei_plan_cem, one wave per env, lane l owning the candidates k = l, l + 64, ... (plan_mppi_finish_kernel's layout):
//   1. (k*, r*) from the env's partials, as plan_finish_kernel finds them;
//   2. T = the key of the n_elites-th candidate in the planner's order, by an MSB-first radix select over the keys' eight bytes: a
//      pass histograms the byte of the candidates whose higher bytes equal T's (256 LDS counters per wave, ds_add), lane l sums
//      bins 4l .. 4l + 3, a suffix scan over the lanes finds the bin the rank falls into and the rank inside it — eight passes over
//      the K returns (L2-resident: the plan kernel has just written them), no K^2 anywhere;
//   3. membership, row of 64 by row of 64 in ascending k: key > T is in; of the key == T candidates the first `need` = n_elites -
//      #{key > T} are (a ballot and a prefix popcount per row, a wave-uniform count of those taken so far), the last of them is
//      the set's last member and gives elite_return; the lane writes 1.0 / 0.0 over the return — as MPPI's weights, read back by
//      the lane that wrote them only;
//   4. the moments: plan_mppi_finish_kernel's walk over the Philox blocks, the members alone redrawn, S1 = sum d and S2 = sum d^2 of
//      d = (double)action - m0 in float64, the lane's members in ascending k, then the butterfly: a tree over k alone.
// Every wave of the block takes the barriers of step 2 (a wave past n_envs with no candidates).
// In place (mean_out == sp.nominal, std_out == sigma_map): entry (t, i, a) of either is read by this wave in block c >> 2 only — the
// draws and m0 — before the block's stores, and belongs to no other wave.
template <class Spec>
__global__ void __launch_bounds__(kBlock)
    plan_cem_finish_kernel(const PlanPartial* partials, double* returns, Spec sp, int64_t n_envs, int32_t n_cand, int32_t n_elites,
                           int32_t horizon, int act_dim, float* mean_out, float* std_out, double* best_return, int32_t* best_index,
                           double* elite_return) {
    __shared__ uint32_t hist_s[kBlock / kWave][256];
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;  // wave-uniform
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const bool have = i < n_envs;
    const int32_t nc = have ? n_cand : 0;
    uint32_t* hist = hist_s[threadIdx.x / kWave];
    double* wt = returns + (have ? i : 0) * n_cand;
    if (have) {
        double rs;
        int32_t ks;
        plan_winner(partials, i, n_cand, lane, rs, ks);
        if (lane == 0) {
            if (best_return) best_return[i] = rs;
            if (best_index) best_index[i] = ks;
        }
    }
    // 2. `need` = the rank looked for among the candidates whose bytes above `shift` equal `prefix`'s; there are >= need of them
    uint64_t prefix = 0ull;
    int32_t need = n_elites;
    for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
        for (int b = 0; b < 4; ++b) hist[4 * lane + b] = 0u;
        __syncthreads();
        for (int32_t k = lane; k < nc; k += kWave) {
            const uint64_t key = plan_key(wt[k]);
            const uint64_t high = shift == 56 ? 0ull : key >> (shift + 8);
            if (high == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        int32_t c[4], own = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) c[b] = (int32_t)hist[4 * lane + b], own += c[b];
        int32_t above = own;  // candidates in this lane's bins and in those of the lanes above it
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int32_t t = __shfl_down(above, d, kWave);
            if (lane + d < kWave) above += t;
        }
        above -= own;
        const bool mine = above < need && need <= above + own;  // one lane (none in a wave without candidates)
        int32_t digit = 0, rest = need;
        if (mine) {
            int32_t a = above;
#pragma unroll
            for (int b = 3; b >= 0; --b) {
                if (a < need && need <= a + c[b]) digit = 4 * lane + b, rest = need - a;
                a += c[b];
            }
        }
        const unsigned long long owner = __ballot(mine);
        const int src = owner ? __builtin_ctzll(owner) : 0;
        digit = __shfl(digit, src, kWave), need = __shfl(rest, src, kWave);
        prefix = (prefix << 8) | (uint64_t)(uint32_t)digit;
        __syncthreads();  // the counters are read before the next pass clears them
    }
    if (!have) return;
    // 3. prefix = T, need = how many of the key == T candidates are members (>= 1)
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
        if (tie && rank == need - 1 && elite_return) elite_return[i] = r;
        taken += (int32_t)__popcll(ties);
    }
    // 4.
    const int na = act_dim > 0 ? act_dim : 1;
    const int32_t n_comp = horizon * na;  // <= 2^31 - 1 (abi.hip:check_candidates)
    const double m = (double)n_elites;
    for (int32_t c0 = 0; c0 < n_comp; c0 += 4) {
        double m0[4], s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t c = min(c0 + u, n_comp - 1);  // past the end: the last component again, dropped below
            if (act_dim == 0) m0[u] = 0.0;
            else m0[u] = sp.nominal ? (double)sp.nominal[((int64_t)(c / na) * n_envs + i) * na + c % na] : (double)(0.5f * (sp.lo + sp.hi));
        }
        for (int32_t k = lane; k < n_cand; k += kWave) {
            if (wt[k] == 0.0) continue;  // no draw for a candidate outside the set
            CandidateWords cw(sp.seed, sp.env_offset + (uint64_t)i, (uint32_t)k);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t c = min(c0 + u, n_comp - 1);
                const double d = (double)draw_action(cw, sp, n_envs, i, c / na, c % na, act_dim) - m0[u];
                s1[u] += d, s2[u] += d * d;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s1[u] = wave_sum_all(s1[u]), s2[u] = wave_sum_all(s2[u]);
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t c = c0 + u;
                if (c >= n_comp) continue;
                const int64_t e = ((int64_t)(c / na) * n_envs + i) * na + c % na;
                const double mu = s1[u] / m;
                mean_out[e] = (float)(m0[u] + mu);
                if (std_out) std_out[e] = (float)sqrt(fmax(s2[u] / m - mu * mu, 0.0));
            }
        }
    }
}

int launch_sample_candidates(const CandidateSpec& sp, int64_t n_envs, int32_t n_cand, int32_t horizon, int act_dim, void* actions_out,
                             int action_dtype, hipStream_t s) {
    dim3 grid((unsigned)((n_envs * n_cand + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(sample_candidates_kernel<CandidateSpec>, grid, dim3(kBlock), 0, s, sp, n_envs, n_cand, horizon, act_dim, actions_out,
                       action_dtype);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}
int launch_sample_candidates_sigma(const CandidateSpecMap& sp, int64_t n_envs, int32_t n_cand, int32_t horizon, int act_dim, void* actions_out,
                                   hipStream_t s) {
    dim3 grid((unsigned)((n_envs * n_cand + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(sample_candidates_kernel<CandidateSpecMap>, grid, dim3(kBlock), 0, s, sp, n_envs, n_cand, horizon, act_dim, actions_out,
                       (int)EMEI_ACT_F32);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}
int launch_plan_finish(const void* partials, const CandidateSpec& sp, int64_t n_envs, int32_t n_cand, int32_t horizon, int act_dim,
                       void* best_action, int action_dtype, void* best_sequence, double* best_return, int32_t* best_index,
                       int32_t* best_length, hipStream_t s) {
    dim3 grid((unsigned)((n_envs + kBlock / kWave - 1) / (kBlock / kWave)));
    hipLaunchKernelGGL(plan_finish_kernel, grid, dim3(kBlock), 0, s, (const PlanPartial*)partials, sp, n_envs, n_cand, horizon, act_dim,
                       best_action, action_dtype, best_sequence, best_return, best_index, best_length);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}
int launch_plan_mppi_finish(const void* partials, double* returns, const CandidateSpec& sp, int64_t n_envs, int32_t n_cand, int32_t horizon,
                            int act_dim, double temperature, float* nominal_out, double* best_return, int32_t* best_index, double* ess,
                            hipStream_t s) {
    dim3 grid((unsigned)((n_envs + kBlock / kWave - 1) / (kBlock / kWave)));
    hipLaunchKernelGGL(plan_mppi_finish_kernel, grid, dim3(kBlock), 0, s, (const PlanPartial*)partials, returns, sp, n_envs, n_cand, horizon,
                       act_dim, temperature, nominal_out, best_return, best_index, ess);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}
int launch_plan_cem_finish(const void* partials, double* returns, const CandidateSpec& sp, const float* sigma_map, int64_t n_envs,
                           int32_t n_cand, int32_t n_elites, int32_t horizon, int act_dim, float* mean_out, float* std_out,
                           double* best_return, int32_t* best_index, double* elite_return, hipStream_t s) {
    dim3 grid((unsigned)((n_envs + kBlock / kWave - 1) / (kBlock / kWave)));
    if (sigma_map)
        hipLaunchKernelGGL(plan_cem_finish_kernel<CandidateSpecMap>, grid, dim3(kBlock), 0, s, (const PlanPartial*)partials, returns,
                           CandidateSpecMap(sp, sigma_map), n_envs, n_cand, n_elites, horizon, act_dim, mean_out, std_out, best_return,
                           best_index, elite_return);
    else
        hipLaunchKernelGGL(plan_cem_finish_kernel<CandidateSpec>, grid, dim3(kBlock), 0, s, (const PlanPartial*)partials, returns, sp, n_envs,
                           n_cand, n_elites, horizon, act_dim, mean_out, std_out, best_return, best_index, elite_return);
    return hipGetLastError() == hipSuccess ? EMEI_OK : EMEI_ERR_HIP;
}

}  // namespace emei
