"""The loop emei_mpc_policy fuses, written against the public API as it was before the fused call existed (policy.PolicyNoise,
Engine.plan_policy, Engine.step): the oracle of tests/test_gpu_mpc_policy.py.

Per control step t, in the order of the header's normative text:
  1. plan_policy(H, K, policy, noise_t, discount, temperature) from the envs' current states, noise_t = the call's noise under the
     seed (base + t * stride) mod 2^64;
  2. the action: the best candidate's first action (act="best"), or the weighted mean of the first actions (act="mean"; discrete
     envs: mean >= 0.5);
  3. step(action, auto_reset).
"""
import torch

MASK64 = 2**64 - 1


def mpc_policy_loop(eng, T, H, K, policy, make_noise, base_seed, stride=None, act="best", temperature=None, discount=1.0, auto_reset=False):
    """make_noise(seed) -> a policy.PolicyNoise of the call's mode under that seed.
    -> (actions [T, N], obs [T, N, obs_dim], reward [T, N], done [T, N], plan_return [T, N], plan_index [T, N][, ess [T, N] with a
    temperature]); the engine is stepped T times."""
    stride = H if stride is None else stride
    acts, obs, rew, done, pret, pidx, ess = [], [], [], [], [], [], []
    for t in range(T):
        noise_t = make_noise((int(base_seed) + t * int(stride)) & MASK64)
        out = eng.plan_policy(H, K, policy, noise_t, discount=discount, temperature=temperature, ess=temperature is not None)
        best, r, k = out[:3]
        if act == "mean":
            mean = out[3].reshape(eng.n_envs)
            a = (mean >= 0.5).to(torch.int64) if eng.act_dim == 0 else mean.clone()
        else:
            a = best.reshape(eng.n_envs).clone()
        o, rw, d = eng.step(a, auto_reset=auto_reset)
        acts.append(a), obs.append(o), rew.append(rw), done.append(d), pret.append(r), pidx.append(k)
        if temperature is not None:
            ess.append(out[-1])
    res = [acts, obs, rew, done, pret, pidx] + ([ess] if temperature is not None else [])
    return tuple(torch.stack(x) for x in res)
