"""The loop emei_mpc_cem fuses, written against the public API as it was before the fused call existed
(Engine.plan_cem(..., out=mean, out_sigma=std), Engine.step, clamp, shift, refill): the oracle of tests/test_gpu_mpc_cem.py.

Per control step t, in the order of the header's normative text:
  1. for j = 0 .. iterations - 1: clamp the mean to (lo, hi); on a continuous env with j = 0 set the per-entry std to `sigma`;
     plan_cem(H, K, n_elites, seed + t * iterations + j, nominal=mean, sigma=std, out=mean, out_sigma=std) from the envs' current
     states; floor the std at sigma_min.  The discrete envs have no std: plan_cem(..., nominal=mean, out=mean);
  2. the action: the mean's first entry (discrete envs: entry >= 0.5);
  3. step(action, auto_reset);
  4. envs that were done under auto-reset get `refill` everywhere, the others shift by one step with `refill` behind.
"""
import torch

from mpc_reference import MASK64, default_clamp, default_refill


def mpc_cem_loop(eng, T, H, K, n_elites, seed, nominal, iterations=1, sigma=None, sigma_min=0.0, discount=1.0, refill=None, clamp=None,
                 auto_reset=False):
    """-> (actions [T, N], obs [T, N, obs_dim], reward [T, N], done [T, N], plan_return [T, N], elite_return [T, N]); `nominal`
    (float32 [H, N] on the engine's device) is updated in place, the engine is stepped T times."""
    refill = default_refill(eng) if refill is None else refill
    lo, hi = default_clamp(eng) if clamp is None else clamp
    std = torch.empty_like(nominal) if eng.act_dim > 0 else None
    acts, obs, rew, done, pret, eret = [], [], [], [], [], []
    for t in range(T):
        for j in range(iterations):
            nominal.clamp_(min=lo, max=hi)
            s = (int(seed) + t * iterations + j) & MASK64
            if std is None:
                _, _, r, _, e = eng.plan_cem(H, K, n_elites, s, discount=discount, nominal=nominal, out=nominal, elite_return=True)
            else:
                if j == 0:
                    std.fill_(sigma)
                _, _, r, _, e = eng.plan_cem(H, K, n_elites, s, discount=discount, nominal=nominal, sigma=std, out=nominal,
                                             out_sigma=std, elite_return=True)
                std.clamp_(min=sigma_min)
        first = nominal[0].reshape(eng.n_envs)
        a = (first >= 0.5).to(torch.int64) if eng.act_dim == 0 else first.clone()
        o, rw, d = eng.step(a, auto_reset=auto_reset)
        was_reset = (d != 0) if auto_reset else torch.zeros_like(d, dtype=torch.bool)
        shifted = torch.full_like(nominal, refill)
        shifted[:-1] = nominal[1:]
        shifted[:, was_reset] = refill
        nominal.copy_(shifted)
        acts.append(a), obs.append(o), rew.append(rw), done.append(d), pret.append(r), eret.append(e)
    return tuple(torch.stack(x) for x in (acts, obs, rew, done, pret, eret))
