"""The loop emei_mpc_mppi fuses, written against the public API as it was before the fused call existed
(Engine.plan_mppi(..., out=nominal), Engine.step, clamp, shift, refill): the oracle of tests/test_gpu_mpc.py.

Per control step t, in the order of the header's normative text:
  1. clamp the nominal to (lo, hi);
  2. plan_mppi(H, K, seed + t, temperature, nominal=nominal, out=nominal) from the envs' current states;
  3. the action: the nominal's first entry (discrete envs: entry >= 0.5);
  4. step(action, auto_reset);
  5. envs that were done under auto-reset get `refill` everywhere, the others shift by one step with `refill` behind.
"""
import torch

MASK64 = 2**64 - 1


def default_refill(eng):
    return 0.5 if eng.act_dim == 0 else 0.0


def default_clamp(eng):
    return (0.05, 0.95) if eng.act_dim == 0 else (-3.0, 3.0)  # the ctrlrange of the InvertedPendulum (xml:23)


def mpc_loop(eng, T, H, K, seed, temperature, nominal, discount=1.0, sigma=None, refill=None, clamp=None, auto_reset=False):
    """-> (actions [T, N], obs [T, N, obs_dim], reward [T, N], done [T, N], plan_return [T, N], ess [T, N]); `nominal` (float32
    [H, N] on the engine's device) is updated in place, the engine is stepped T times."""
    refill = default_refill(eng) if refill is None else refill
    lo, hi = default_clamp(eng) if clamp is None else clamp
    acts, obs, rew, done, pret, ess = [], [], [], [], [], []
    for t in range(T):
        nominal.clamp_(min=lo, max=hi)
        _, r, _, e = eng.plan_mppi(H, K, (int(seed) + t) & MASK64, temperature, discount=discount, nominal=nominal, sigma=sigma,
                                   out=nominal, ess=True)
        first = nominal[0].reshape(eng.n_envs)
        a = (first >= 0.5).to(torch.int64) if eng.act_dim == 0 else first.clone()
        o, rw, d = eng.step(a, auto_reset=auto_reset)
        was_reset = (d != 0) if auto_reset else torch.zeros_like(d, dtype=torch.bool)
        shifted = torch.full_like(nominal, refill)
        shifted[:-1] = nominal[1:]
        shifted[:, was_reset] = refill
        nominal.copy_(shifted)
        acts.append(a), obs.append(o), rew.append(rw), done.append(d), pret.append(r), ess.append(e)
    return tuple(torch.stack(x) for x in (acts, obs, rew, done, pret, ess))
