"""Reference of emei_rollout_policy for the tests: the policy arithmetic in numpy, written from the normative text of
include/emei_hip.h, and the per-step loop against the API as it was before the call existed.

mlp_actions follows the text line by line: float64 accumulators, the terms added one at a time in ascending index order (numpy's
elementwise multiply and add are IEEE operations; the product of two widened float32 values is exact in float64, so nothing
depends on fusing), the hidden unit rounded to float32 before the ReLU, NaN handled as the text says.
"""
import numpy as np


def _f32(t):
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=np.float32)


def ctrl_range(env_name):
    """the ctrlrange of the candidate specification: +-3 for the InvertedPendulum family, +-1 otherwise"""
    single = env_name.endswith(("InvertedPendulumBalancing", "InvertedPendulumSwingUp"))  # ("...DoublePendulum..." does not end so)
    return (np.float32(-3.0), np.float32(3.0)) if single else (np.float32(-1.0), np.float32(1.0))


def mlp_logits(policy, x, order=None):
    """y [N, n_out] float64 of the normative text.  order: a permutation of the hidden units (of the inputs for an affine policy)
    in which the OUTPUT sum runs instead of ascending — for the test that shows the order matters."""
    w1, b1, w2, b2 = _f32(policy.w1), _f32(policy.b1), _f32(policy.w2), _f32(policy.b2)
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    with np.errstate(all="ignore"):
        if w1 is not None:
            h = np.empty((n, w1.shape[0]), np.float32)
            for j in range(w1.shape[0]):
                z = np.full(n, np.float64(b1[j]))
                for k in range(w1.shape[1]):
                    z = z + np.float64(w1[j, k]) * x[:, k].astype(np.float64)
                hj = z.astype(np.float32)
                h[:, j] = np.where(hj > np.float32(0), hj, np.float32(0))  # NaN > 0 is false: 0
        else:
            h = x
        y = np.empty((n, w2.shape[0]), np.float64)
        idx = range(h.shape[1]) if order is None else order
        for q in range(w2.shape[0]):
            acc = np.full(n, np.float64(b2[q]))
            for j in idx:
                acc = acc + np.float64(w2[q, j]) * h[:, j].astype(np.float64)
            y[:, q] = acc
    return y


def mlp_actions(policy, x, lo, hi, discrete, order=None):
    """actions of `policy` on the float32 rows x [N, obs_dim]: int64 [N] (discrete), float32 [N, act_dim] (continuous)."""
    y = mlp_logits(policy, x, order)
    if discrete:
        return (y[:, 0] >= 0.0).astype(np.int64)  # NaN >= 0 is false: 0
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        if getattr(policy, "out", "clip") == "tanh":
            lo64, hi64 = np.float64(lo), np.float64(hi)
            return (0.5 * (hi64 + lo64) + 0.5 * (hi64 - lo64) * np.tanh(y)).astype(np.float32)
        a = y.astype(np.float32)
        a = np.where(a >= lo, a, lo)  # fmaxf(a, lo): NaN gives lo
        return np.where(a <= hi, a, hi).astype(np.float32)  # fminf(., hi)


def policy_loop(eng, T, policy, auto_reset):
    """The loop emei_rollout_policy replaces, against get_obs / step / episode_init_obs / get_counters:
    -> dict(actions [T, N(, act_dim)], obs, reward, done, seen [T, N, obs_dim]: the rows the policy was shown), numpy arrays."""
    import torch

    lo, hi = ctrl_range(eng.env_name)
    discrete = eng.act_dim == 0
    cur = eng.get_obs().to(torch.float32)
    _, epi = eng.get_counters()
    acts, obs, rew, done, seen = [], [], [], [], []
    for _ in range(int(T)):
        x = cur.cpu().numpy()
        a = mlp_actions(policy, x, lo, hi, discrete)
        if not discrete and eng.act_dim == 1:
            a = a[:, 0]
        o, r, d = eng.step(torch.as_tensor(np.ascontiguousarray(a), device=eng.device), auto_reset=auto_reset)
        seen.append(x), acts.append(a), obs.append(o.cpu().numpy()), rew.append(r.cpu().numpy()), done.append(d.cpu().numpy())
        cur = o.clone()
        dd = d != 0
        if auto_reset and bool(dd.any()):  # the policy must see what reset() returned for the finished envs
            epi = epi + dd.to(torch.int64)
            idx = torch.nonzero(dd).reshape(-1)
            cur[idx] = eng.episode_init_obs(idx, epi[idx])
    return dict(actions=np.stack(acts), obs=np.stack(obs), reward=np.stack(rew), done=np.stack(done), seen=np.stack(seen))
