"""Reference of emei_rollout_policy_noisy for the tests: the noise clause in numpy, written from the normative text of
include/emei_hip.h on top of policy_reference.mlp_logits (the deterministic sums) and shooting_reference (the word stream, u01, the
exact Box-Muller normal), and the per-step loop extended with it.

A noise description is any object with `mode` in {"gauss", "head", "eps"} and `seed`, plus
  gauss: std [n_out] float32;  head: ws, bs, log_std_min, log_std_max;  eps: epsilon.
"""
import numpy as np

import policy_reference as PR
import shooting_reference as SR

M64 = 2 ** 64


def key(seed, t):
    """the key of step t: seed + t (mod 2^64)"""
    return (int(seed) + int(t)) % M64


def noise_words(seed, t, g, n_words):
    """W[m] of step t for the global env indices g [N]: candidate k = 0 under the key seed + t -> [n_words, N] uint32"""
    return SR.words(key(seed, t), np.asarray(g, np.uint64), np.array([0], np.uint64), n_words)[:, :, 0]


def pair_of(q):
    """component q reads the Box-Muller pair p = q >> 1, its cosine (0) or sine (1) half"""
    return q >> 1, q & 1


def normals_exact(seed, t, g, n_out):
    """z [N, n_out] float64, unrounded: z_q = sqrt(-2 ln u1) (cos, sin)(2 pi turns)[q & 1] of (W[2p], W[2p + 1]), p = q >> 1, with
    u1 = (field(W[2p]) + 1) / 2^24 and turns = field(W[2p + 1]) / 2^24"""
    w = noise_words(seed, t, g, 2 * ((n_out + 1) // 2))
    z = np.empty((w.shape[1], n_out), np.float64)
    for q in range(n_out):
        p, half = pair_of(q)
        a, b = SR.field(w[2 * p]).astype(np.float64), SR.field(w[2 * p + 1]).astype(np.float64)
        rad, ang = np.sqrt(-2.0 * np.log((a + 1.0) * 2.0 ** -24)), 2.0 * np.pi * (b * 2.0 ** -24)
        z[:, q] = rad * (np.sin(ang) if half else np.cos(ang))
    return z


def eps_greedy_flags(seed, t, g, epsilon):
    """(explore, coin) [N] bool: u(W[0]) < (float)epsilon, u(W[1]) < 0.5f"""
    u = SR.u01(noise_words(seed, t, g, 2))
    return u[0] < np.float32(epsilon), u[1] < np.float32(0.5)


def head_scale(policy, noise, x):
    """s [N, n_out] float32 of GAUSS_HEAD: l_q is y_q's sum with (ws, bs) in the place of (w2, b2), over the same h"""
    head = type("Head", (), dict(w1=policy.w1, b1=policy.b1, w2=noise.ws, b2=noise.bs))
    lq = PR.mlp_logits(head, x)
    with np.errstate(all="ignore"):
        lq = np.minimum(np.maximum(lq, np.float64(np.float32(noise.log_std_min))), np.float64(np.float32(noise.log_std_max)))
        return np.exp(lq).astype(np.float32)


def scale(policy, noise, x):
    if noise.mode == "head":
        return head_scale(policy, noise, x)
    return np.broadcast_to(np.asarray(noise.std, np.float32)[None, :], (np.asarray(x).shape[0], len(noise.std)))


def output_clause(y, out, lo, hi):
    """the continuous output clause of emei_rollout_policy on float64 y: CLIP (NaN gives lo) or TANH"""
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        if out == "tanh":
            lo64, hi64 = np.float64(lo), np.float64(hi)
            return (0.5 * (hi64 + lo64) + 0.5 * (hi64 - lo64) * np.tanh(y)).astype(np.float32)
        a = y.astype(np.float32)
        a = np.where(a >= lo, a, lo)
        return np.where(a <= hi, a, hi).astype(np.float32)


def noisy_logits(policy, noise, x, z):
    """(y + (double)s * (double)z, y, s): the noise term joins the ascending sum last; z [N, n_out] float32"""
    y = PR.mlp_logits(policy, x)
    s = scale(policy, noise, x)
    with np.errstate(all="ignore"):
        return y + s.astype(np.float64) * np.asarray(z, np.float32).astype(np.float64), y, s


def noisy_actions(policy, noise, x, lo, hi, discrete, z=None, flags=None):
    """the actions of step t on the float32 rows x [N, obs_dim]: continuous envs take the step's normals z [N, n_out] float32,
    discrete envs its (explore, coin) flags"""
    if discrete:
        greedy = PR.mlp_logits(policy, x)[:, 0] >= 0.0
        explore, coin = flags
        return np.where(explore, coin, greedy).astype(np.int64)
    return output_clause(noisy_logits(policy, noise, x, z)[0], getattr(policy, "out", "clip"), lo, hi)


def noisy_policy_loop(eng, T, policy, noise, draws, auto_reset, g):
    """policy_reference.policy_loop with the noise clause: draws(t) -> z [N(, act_dim)] float32 for the continuous envs (the
    device's normals, PolicyNoise.draws); the discrete flags come from the CPU Philox over the global env indices g."""
    import torch

    lo, hi = PR.ctrl_range(eng.env_name)
    discrete = eng.act_dim == 0
    cur = eng.get_obs().to(torch.float32)
    _, epi = eng.get_counters()
    acts, obs, rew, done, seen = [], [], [], [], []
    for t in range(int(T)):
        x = cur.cpu().numpy()
        if discrete:
            a = noisy_actions(policy, noise, x, lo, hi, True, flags=eps_greedy_flags(noise.seed, t, g, noise.epsilon))
        else:
            z = draws(t).cpu().numpy().reshape(x.shape[0], -1)
            a = noisy_actions(policy, noise, x, lo, hi, False, z=z)
            if eng.act_dim == 1:
                a = a[:, 0]
        o, r, d = eng.step(torch.as_tensor(np.ascontiguousarray(a), device=eng.device), auto_reset=auto_reset)
        seen.append(x), acts.append(a), obs.append(o.cpu().numpy()), rew.append(r.cpu().numpy()), done.append(d.cpu().numpy())
        cur = o.clone()
        dd = d != 0
        if auto_reset and bool(dd.any()):
            epi = epi + dd.to(torch.int64)
            idx = torch.nonzero(dd).reshape(-1)
            cur[idx] = eng.episode_init_obs(idx, epi[idx])
    return dict(actions=np.stack(acts), obs=np.stack(obs), reward=np.stack(rew), done=np.stack(done), seen=np.stack(seen))
