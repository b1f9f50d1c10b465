"""emei_rollout_policy_deep / emei_evaluate_policies_deep on the GPU (pend_policy_rollout_deep_kernel, body_policy_rollout_deep_kernel,
pend_policy_eval_deep_kernel, body_policy_eval_deep_kernel): the two-hidden-layer network inside the rollout and population launches.

Shapes: N = 70 (a full wave and a ragged one) and N = 130 (three one-wave blocks), T = 12 under auto-reset with TimeLimits of 4 to 6
steps, so every env crosses a reset inside the call; env_index_offset 4000.

1. Embedding.  A one-layer MLPPolicy(w2, b2, w1, b1) is rewritten as a deep net: first layer rows (e_k, -e_k) with zero biases, so
   h1 = (relu(x_k), relu(-x_k)) exactly, one of each pair zero; second layer w2'[i, 2k] = w1[i, k], w2'[i, 2k + 1] = -w1[i, k] with
   b2' = b1; third layer = (w2, b2).  Every ascending sum of the deep net then has the one-layer sum's terms in order with zeros
   between them (a zero can only change the sign of a zero sum, which the ReLU and the clip erase), so the deep launch must equal the
   one-layer launch — pinned to the CPU references by tests/test_gpu_policy*.py — in every output bit.
2. The per-step loop with the DeepMLPPolicy itself as the callable (torch float64, pinned to an independent numpy restatement by
   tests/test_policy_deep_reference.py): bit for bit under CLIP and on the discrete env, with and without noise.  TANH and the log-std
   head are teacher-forced on the rows the policy saw and held to the bounds of tests/test_gpu_policy.py:test_tanh_mode and
   tests/test_gpu_policy_noise.py:test_head_teacher_forced.
3. Replay through rollout(), 4. chunking and sharding with noise, 5. the population against the replay route of
   tests/test_gpu_policy_population.py, 6. the kernel ids."""
import functools
import types

import numpy as np
import pytest

import policy_noise_reference as NR
import policy_reference as PR
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BODY = dict(freq_rate=4, real_time_scale=0.002)
OFFSET = 4000
T = 12
CASES = {
    "cartpole": dict(env="CartPoleSwingUp", kw=dict(max_episode_steps=5)),  # discrete, 4-state family
    "ip": dict(env="ReboundInvertedPendulumSwingUp", kw=dict(max_episode_steps=6)),  # continuous, 4-state family, ctrlrange +-3
    "idp": dict(env="ReboundInvertedDoublePendulumSwingUp", kw=dict(max_episode_steps=6, init_noise=0.05)),
    "cheetah": dict(env="HalfCheetahRunning", kw=dict(max_episode_steps=4, init_noise=0.1, **BODY)),
    "hopper-rk4": dict(env="HopperRunning", kw=dict(integrator="rk4", max_episode_steps=5, init_noise=0.01, **BODY)),  # the RK4 body kernel
}
EPSILON = 0.25
SEED = 2 ** 64 - 3  # seed + t wraps inside the call


def _engine(case, n, **over):
    from emei_amd.engine import Engine

    kw = dict(seed=11, env_index_offset=OFFSET)
    kw.update(CASES[case]["kw"])
    kw.update(over)
    eng = Engine(CASES[case]["env"], n, **kw)
    eng.reset(11)
    return eng


def _rand(rng, *s):
    return (rng.standard_normal(s) * 1.5 / np.sqrt(s[-1])).astype(np.float32)


def _one_layer_weights(eng, hidden, seed):
    rng = np.random.default_rng(seed)
    n_out = max(eng.act_dim, 1)
    return types.SimpleNamespace(w2=_rand(rng, n_out, hidden), b2=_rand(rng, n_out), w1=_rand(rng, hidden, eng.obs_dim), b1=_rand(rng, hidden))


def _embed(w):
    """the deep net that computes the one-layer net w with zero terms between its terms (module docstring, 1.)"""
    hidden, obs_dim = w.w1.shape
    w1 = np.zeros((2 * obs_dim, obs_dim), np.float32)
    w1[0::2] = np.eye(obs_dim, dtype=np.float32)
    w1[1::2] = -np.eye(obs_dim, dtype=np.float32)
    w2 = np.zeros((hidden, 2 * obs_dim), np.float32)
    w2[:, 0::2] = w.w1
    w2[:, 1::2] = -w.w1
    return types.SimpleNamespace(w1=w1, b1=np.zeros(2 * obs_dim, np.float32), w2=w2, b2=w.b1.copy(), w3=w.w2.copy(), b3=w.b2.copy())


def _deep_weights(eng, h1, h2, seed):
    rng = np.random.default_rng(seed)
    n_out = max(eng.act_dim, 1)
    return types.SimpleNamespace(w1=_rand(rng, h1, eng.obs_dim), b1=_rand(rng, h1), w2=_rand(rng, h2, h1), b2=_rand(rng, h2),
                                 w3=_rand(rng, n_out, h2), b3=_rand(rng, n_out))


def _deep(w, out="clip"):
    from emei_amd.policy import DeepMLPPolicy

    return DeepMLPPolicy(w.w3, w.b3, w.w2, w.b2, w.w1, w.b1, out=out)


def _noise(eng, mode="std", hidden_in=None):
    """(PolicyNoise, its description for tests/policy_noise_reference.py): std per component / epsilon by the env kind, or the head"""
    from emei_amd.policy import PolicyNoise

    n_out = max(eng.act_dim, 1)
    if eng.act_dim == 0:
        return PolicyNoise(SEED, epsilon=EPSILON), types.SimpleNamespace(mode="eps", seed=SEED, epsilon=EPSILON)
    if mode == "head":
        rng = np.random.default_rng(5 + hidden_in)
        ws = (rng.standard_normal((n_out, hidden_in)) * 2.0 / np.sqrt(hidden_in)).astype(np.float32)
        bs = (rng.standard_normal(n_out) - 1.0).astype(np.float32)
        rg = (-3.0, 0.5)
        return (PolicyNoise(SEED, log_std_head=(ws, bs), log_std_range=rg),
                types.SimpleNamespace(mode="head", seed=SEED, ws=ws, bs=bs, log_std_min=rg[0], log_std_max=rg[1]))
    std = (0.1 + 0.3 * np.arange(1, n_out + 1, dtype=np.float32) / n_out).astype(np.float32)
    return PolicyNoise(SEED, std=std), types.SimpleNamespace(mode="gauss", seed=SEED, std=std)


def _rewind(eng):
    eng.unfreeze()
    eng.freeze()


def _end(eng):
    steps, epi = eng.get_counters()
    return dict(state=eng.get_state().cpu().numpy(), steps=steps.cpu().numpy(), episode=epi.cpu().numpy(),
                compact=eng.compact_done().cpu().numpy())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _np(ts):
    return dict(zip(("actions", "obs", "reward", "done"), (t.cpu().numpy() for t in ts)))


def _assert_same_run(a, b, what):
    for k in ("actions", "obs", "reward", "done"):
        assert _same(a[k], b[k]), (what, k)
    for k in ("state", "steps", "episode", "compact"):
        assert _same(a["end"][k], b["end"][k]), (what, k)


def _expected_kernel(case):
    from emei_amd import _lib as L

    if case in ("cartpole", "ip"):
        return L.KERNEL_PEND_POLICY_DEEP
    return L.KERNEL_BODY_POLICY_DEEP_RK4 if CASES[case]["kw"].get("integrator") == "rk4" else L.KERNEL_BODY_POLICY_DEEP


def _launch(eng, pol, steps, noise=None, auto_reset=True):
    r = _np(eng.rollout_policy(steps, pol, auto_reset=auto_reset, noise=noise))
    r["kernel"], r["end"] = eng.last_kernel(), _end(eng)
    return r


# ------------------------------------------------------------------------------------------------ 1. the embedding
@functools.lru_cache(maxsize=None)
def _embedding_run(case, n):
    """one frozen start: the one-layer launch and the deep launch of its embedding, without and with noise"""
    from emei_amd.policy import MLPPolicy

    eng = _engine(case, n)
    w = _one_layer_weights(eng, 7, 300 + len(case))
    one, deep = MLPPolicy(w.w2, w.b2, w.w1, w.b1), _deep(_embed(w))
    assert (deep.hidden1, deep.hidden2) == (2 * eng.obs_dim, 7)
    eng.freeze()
    res = {}
    for noisy in (False, True):
        for name, pol in (("one", one), ("deep", deep)):
            _rewind(eng)
            res[name, noisy] = _launch(eng, pol, T, _noise(eng)[0] if noisy else None)
    eng.close()
    return res


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("n", [70, 130])
@pytest.mark.parametrize("case", list(CASES))
def test_embedding_equals_the_one_layer_launch(case, n, noisy):
    from emei_amd import _lib as L

    r = _embedding_run(case, n)
    one, deep = r["one", noisy], r["deep", noisy]
    _assert_same_run(deep, one, "embedding")
    assert deep["kernel"] == _expected_kernel(case) and one["kernel"] in (15, 16, 17, 18, 19, 20) and "deep" in L.kernel_name(deep["kernel"])
    assert one["done"].any()  # envs crossed a reset inside the call
    assert np.isfinite(one["obs"]).all()
    if noisy:  # ... and the noise did something
        assert not _same(one["actions"], r["one", False]["actions"])


@pytest.mark.parametrize("n", [70, 130])
@pytest.mark.parametrize("case", list(CASES))
def test_embedding_equals_the_one_layer_population(case, n):
    from emei_amd.policy import DeepPolicyPopulation, MLPPolicy, PolicyPopulation

    eng = _engine(case, n)
    ws = [_one_layer_weights(eng, 7, 400 + 10 * p + len(case)) for p in range(3)]
    one = PolicyPopulation.from_policies([MLPPolicy(w.w2, w.b2, w.w1, w.b1) for w in ws])
    deep = DeepPolicyPopulation.from_policies([_deep(_embed(w)) for w in ws])
    want = [t.cpu().numpy() for t in eng.evaluate_policies(one, T, discount=0.97, final_obs=True)]
    got = [t.cpu().numpy() for t in eng.evaluate_policies(deep, T, discount=0.97, final_obs=True)]
    eng.close()
    assert got[0].shape == (3, n) and np.array_equal(got[1], want[1])
    if case == "cheetah":  # its wave-mates may differ between the two block shapes: the bound of tests/test_gpu_policy_population.py
        print(f"{case}: returns rel_err {rel_err(got[0], want[0]):.3e} (bound 1e-9), final_obs rel_err {rel_err(got[2], want[2]):.3e} (bound 2^-23)")
        assert rel_err(got[0], want[0]) <= 1e-9 and rel_err(got[2], want[2]) <= 2.0 ** -23
    else:
        assert _same(got[0], want[0]) and _same(got[2], want[2])
    if case != "cartpole":  # (two-valued actions from near-identical starts: members of the discrete case may well act alike)
        assert len({got[0][p].tobytes() for p in range(3)}) == 3  # the members are told apart


# ------------------------------------------------------------------------------------------------ 2. the per-step loop, 3. replay
def _loop(eng, pol, steps, noise):
    """reset's observation, policy(obs) as the callable, step, and the episode_init_obs rule on done envs (what datasets.collect
    does with a lambda): -> the launch's four outputs and the rows the policy saw"""
    cur = eng.get_obs().to(torch.float32)
    _, epi = eng.get_counters()
    acts, obs, rew, done, seen = [], [], [], [], []
    for t in range(steps):
        a = pol(cur) if noise is None else pol(cur, noise, t)
        o, r, d = eng.step(a, auto_reset=True)
        seen.append(cur.cpu().numpy()), acts.append(a.cpu().numpy()), obs.append(o.cpu().numpy()), rew.append(r.cpu().numpy())
        done.append(d.cpu().numpy())
        cur = o.clone()
        dd = d != 0
        if bool(dd.any()):
            epi = epi + dd.to(torch.int64)
            idx = torch.nonzero(dd).reshape(-1)
            cur[idx] = eng.episode_init_obs(idx, epi[idx])
    return dict(actions=np.stack(acts), obs=np.stack(obs), reward=np.stack(rew), done=np.stack(done), seen=np.stack(seen), end=_end(eng))


@functools.lru_cache(maxsize=None)
def _parity_run(case, n, h1, h2, steps, noisy):
    eng = _engine(case, n)
    pol = _deep(_deep_weights(eng, h1, h2, 500 + h1 + h2 + len(case))).bind(eng)
    noise = _noise(eng)[0].bind(eng) if noisy else None
    eng.freeze()
    res = dict(loop=_loop(eng, pol, steps, noise))
    _rewind(eng)
    res["fused"] = _launch(eng, pol, steps, noise)
    _rewind(eng)
    o2, r2, d2 = eng.rollout(torch.as_tensor(res["fused"]["actions"], device=eng.device), auto_reset=True)
    res["replay"] = dict(actions=res["fused"]["actions"], obs=o2.cpu().numpy(), reward=r2.cpu().numpy(), done=d2.cpu().numpy(), end=_end(eng))
    eng.close()
    return res


PARITY = [(c, n, h1, h2, T, noisy) for c, n in (("cartpole", 130), ("cheetah", 70)) for h1, h2 in ((1, 1), (5, 3), (64, 64))
          for noisy in (False, True)] + \
         [("cartpole", 70, 5, 3, T, True), ("cheetah", 130, 5, 3, T, True),
          ("cheetah", 70, 256, 256, 4, False),  # the LDS cap beside the solver's slots, once
          ("cartpole", 130, 256, 7, T, False)]


@pytest.mark.parametrize("case,n,h1,h2,steps,noisy", PARITY)
def test_parity_with_the_per_step_loop_and_replay(case, n, h1, h2, steps, noisy):
    r = _parity_run(case, n, h1, h2, steps, noisy)
    loop, fused = r["loop"], r["fused"]
    assert fused["actions"].dtype == (np.int64 if case == "cartpole" else np.float32)
    _assert_same_run(fused, loop, "loop")
    _assert_same_run(fused, r["replay"], "replay")
    assert fused["kernel"] == _expected_kernel(case)
    if steps == T:
        assert fused["done"].any()  # the TimeLimit ran out inside the call
    if case == "cheetah" and h1 > 1:
        a = fused["actions"]
        assert (np.abs(a) < 1).any() and len(np.unique(a)) > a.size // 4  # not all on the clip


def _numpy_deep(w, rows):
    """(the pseudo one-layer policy (w2, b2, w3, b3) over h1, h1 [N, hidden1] float32): tests/policy_reference.py's ascending sums serve
    the deep net once the first layer is applied — its hidden layer is the deep net's second, its input the deep net's h1"""
    first = types.SimpleNamespace(w1=None, b1=None, w2=w.w1, b2=w.b1)
    z = PR.mlp_logits(first, rows).astype(np.float32)
    h1 = np.where(z > np.float32(0), z, np.float32(0))
    return types.SimpleNamespace(w1=w.w2, b1=w.b2, w2=w.w3, b2=w.b3), h1


def _seen(eng, x0, obs, done, epi0):
    """the rows the policy saw: x_0, then every emitted row, or the new episode's first observation after an auto-reset"""
    seen = torch.cat([x0[None], obs[:-1]]).clone()
    if bool((done[:-1] != 0).any()):
        t_idx, e_idx = torch.nonzero(done[:-1] != 0, as_tuple=True)
        episodes = epi0[None, :].to(torch.int64) + torch.cumsum((done != 0).to(torch.int64), dim=0)
        seen[t_idx + 1, e_idx] = eng.episode_init_obs(e_idx, episodes[t_idx, e_idx])
    return seen.cpu().numpy()


@pytest.mark.parametrize("mode,out", [("none", "tanh"), ("head", "clip"), ("head", "tanh")])
@pytest.mark.parametrize("case,n,h1,h2", [("ip", 130, 5, 3), ("cheetah", 70, 64, 64), ("hopper-rk4", 70, 64, 33)])
def test_tanh_and_the_log_std_head_teacher_forced(case, n, h1, h2, mode, out):
    """TANH: within ONE float32 spacing at max(|lo|, |hi|) of the numpy clause (tests/test_gpu_policy.py:test_tanh_mode).  The head
    (tests/test_gpu_policy_noise.py:test_head_teacher_forced): under CLIP |a - a_ref| <= 2^-23 (s_ref |z| + |y_ref|) + the smallest
    subnormal; under TANH the one spacing plus half * 2^-23 * s_ref |z|.  Replay holds bit for bit in every mode."""
    eng = _engine(case, n)
    w = _deep_weights(eng, h1, h2, 600 + h1 + len(case))
    pol = _deep(w, out)
    noise, nref = _noise(eng, "head", h2) if mode == "head" else (None, None)
    eng.freeze()
    _, epi0 = eng.get_counters()
    x0 = eng.get_obs().to(torch.float32)
    act, obs, rew, done = eng.rollout_policy(T, pol, auto_reset=True, noise=noise)
    assert eng.last_kernel() == _expected_kernel(case)
    seen = _seen(eng, x0, obs, done, epi0)
    z = np.stack([noise.draws(eng, t).cpu().numpy().reshape(n, -1) for t in range(T)]) if noise is not None else None
    _rewind(eng)
    o2, r2, d2 = eng.rollout(act, auto_reset=True)
    for a, b in ((obs, o2), (rew, r2), (done, d2)):
        assert _same(a.cpu().numpy(), b.cpu().numpy())
    eng.close()
    lo, hi = PR.ctrl_range(CASES[case]["env"])
    rows = seen.reshape(-1, seen.shape[-1])
    pseudo, h1_rows = _numpy_deep(w, rows)
    got = act.cpu().numpy().reshape(T, n, -1)
    spacing = float(np.spacing(np.float32(max(abs(lo), abs(hi)))))
    if mode == "none":
        want = NR.output_clause(PR.mlp_logits(pseudo, h1_rows), out, lo, hi).reshape(got.shape)
        tol = spacing
    else:
        yn, y, s = NR.noisy_logits(pseudo, nref, h1_rows, z.reshape(rows.shape[0], -1))
        want = NR.output_clause(yn, out, lo, hi).reshape(got.shape)
        sz = (s.astype(np.float64) * np.abs(z.reshape(s.shape)).astype(np.float64)).reshape(got.shape)
        if out == "clip":
            tol = 2.0 ** -23 * (sz + np.abs(y).reshape(got.shape)) + float(np.finfo(np.float32).smallest_subnormal)
        else:
            tol = spacing + 0.5 * (float(hi) - float(lo)) * 2.0 ** -23 * sz
        assert s.min() >= np.float32(np.exp(-3.0)) and s.max() <= np.float32(np.exp(0.5)) and len(np.unique(s)) > 10
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{case} {mode} {out}: max |a - ref| = {err.max():.3e}, max err / bound = {(err / tol).max():.3f}, {np.mean(err > 0):.4f} differ")
    assert (err <= tol).all(), float((err - tol).max())
    assert (np.abs(got) <= hi).all() and (np.abs(got) < hi).any()


# ------------------------------------------------------------------------------------------------ 4. chunking and sharding
@pytest.mark.parametrize("a,b", [(5, 7)])
@pytest.mark.parametrize("case,n", [("cartpole", 130), ("cheetah", 70)])
def test_chunking_with_noise(case, n, a, b):
    """(a + b, seed) against (a, seed) then (b, seed + a).  It holds where (float)get_obs() equals the row the last step emitted:
    asserted first, as tests/test_gpu_policy_noise.py does."""
    from emei_amd.policy import PolicyNoise

    eng = _engine(case, n, max_episode_steps=0)  # no TimeLimit: nothing is reset between the chunks
    pol = _deep(_deep_weights(eng, 5, 3, 700))
    noise, nref = _noise(eng)
    kw = dict(epsilon=EPSILON) if eng.act_dim == 0 else dict(std=nref.std)
    eng.freeze()
    whole = [t.cpu().numpy() for t in eng.rollout_policy(a + b, pol, noise=noise)]
    end_whole = _end(eng)
    _rewind(eng)
    first = [t.cpu().numpy() for t in eng.rollout_policy(a, pol, noise=PolicyNoise(nref.seed, **kw))]
    getter = eng.get_obs().to(torch.float32).cpu().numpy()
    assert _same(getter, first[1][-1]), "precondition: the getter's row is the emitted row"
    second = [t.cpu().numpy() for t in eng.rollout_policy(b, pol, noise=PolicyNoise(nref.seed + a, **kw))]
    for w, x, y in zip(whole, first, second):
        assert _same(w, np.concatenate([x, y]))
    end = _end(eng)
    for k in end:
        assert _same(end[k], end_whole[k]), k
    _rewind(eng)  # the second chunk under the FIRST chunk's seed is another trajectory: the key of step t is seed + t
    eng.rollout_policy(a, pol, noise=PolicyNoise(nref.seed, **kw))
    other = eng.rollout_policy(b, pol, noise=PolicyNoise(nref.seed, **kw))[0].cpu().numpy()
    assert not _same(other, second[0])
    eng.close()


@pytest.mark.parametrize("case", ["cartpole", "cheetah"])
def test_shard_invariance_with_noise(case):
    """envs [0, 64) and [64, 128) as two engines with env_index_offset against one engine of 128"""
    outs = []
    for n, offs in ((128, (OFFSET,)), (64, (OFFSET, OFFSET + 64))):
        parts = []
        for off in offs:
            eng = _engine(case, n, env_index_offset=off)
            pol = _deep(_deep_weights(eng, 5, 3, 800))
            parts.append([t.cpu().numpy() for t in eng.rollout_policy(T, pol, auto_reset=True, noise=_noise(eng)[0])] + [_end(eng)["state"][None]])
            eng.close()
        outs.append([np.concatenate([p[k] for p in parts], axis=1) for k in range(5)])
    assert outs[0][3].any()  # some env was reset: the reset stream is part of what is compared
    for x, y in zip(*outs):
        assert _same(x, y)
    assert not _same(outs[0][0][:, :64], outs[0][0][:, 64:])  # the halves draw different noise


# ------------------------------------------------------------------------------------------------ 5. the population
@pytest.mark.parametrize("case,n,h1,h2", [("cartpole", 130, 5, 3), ("ip", 70, 64, 33), ("cheetah", 70, 5, 3), ("hopper-rk4", 70, 5, 3)])
def test_population_equals_the_replay_of_its_members(case, n, h1, h2):
    """evaluate_policies(DeepPolicyPopulation) against rollout_policy(H, pop[p], auto_reset=False) replayed through
    evaluate_sequences: the relation tests/test_gpu_policy_population.py pins for one layer, with its HalfCheetah tolerance; and the
    handle's state, counters, done mask and last kernel are what they were."""
    from emei_amd.policy import DeepPolicyPopulation

    H, P = T, 3
    eng = _engine(case, n, max_episode_steps=0)
    pop = DeepPolicyPopulation.from_policies([_deep(_deep_weights(eng, h1, h2, 900 + p)) for p in range(P)]).bind(eng)
    start = eng.get_state().clone()
    acts = []
    for p in range(P):
        eng.set_state(start)
        acts.append(eng.rollout_policy(H, pop[p], auto_reset=False)[0])
    cand = torch.stack(acts, dim=2).contiguous()  # [H, N, P(, act_dim)]
    eng.set_state(start)
    e_ret, e_L, e_fo = eng.evaluate_sequences(cand, discount=0.97, final_obs=True)
    e_ret, e_L, e_fo = e_ret.T.cpu().numpy(), e_L.T.cpu().numpy(), e_fo.transpose(0, 1).contiguous().cpu().numpy()
    eng.set_state(start)
    eng.rollout_policy(3, pop[0], auto_reset=False)  # counters and a last kernel that are not the initial ones
    before = (_end(eng), eng.last_kernel())
    ret, L, fo = (t.cpu().numpy() for t in eng.evaluate_policies(pop, H, discount=0.97, start_state=start, final_obs=True))
    after = (_end(eng), eng.last_kernel())
    assert before[1] == after[1] == _expected_kernel(case)
    for k in before[0]:
        assert _same(before[0][k], after[0][k]), k
    single = eng.evaluate_policies(pop[1], H, discount=0.97, start_state=start)[0].cpu().numpy()  # one DeepMLPPolicy: a population of one
    eng.close()
    assert ret.shape == (P, n) and ret.dtype == np.float64 and L.dtype == np.int32 and fo.shape == (P, n, fo.shape[2])
    assert np.array_equal(L, e_L)
    if case == "cheetah":
        print(f"{case}: returns rel_err {rel_err(ret, e_ret):.3e} (bound 1e-9), final_obs rel_err {rel_err(fo, e_fo):.3e} (bound 2^-23)")
        assert rel_err(ret, e_ret) <= 1e-9 and rel_err(fo, e_fo) <= 2.0 ** -23
        assert rel_err(single[0], ret[1]) <= 1e-9
    else:
        assert _same(ret, e_ret) and _same(fo, e_fo)
        assert _same(single[0], ret[1])
    if case != "cartpole":  # as in the embedding test
        assert len({ret[p].tobytes() for p in range(P)}) == P  # the members are told apart


# ------------------------------------------------------------------------------------------------ 6. kernel ids, untouched paths
def test_kernel_ids_and_the_one_layer_paths_in_one_process():
    from emei_amd import _lib as L
    from emei_amd.policy import MLPPolicy

    seen = {}
    for case in CASES:
        eng = _engine(case, 70)
        w = _one_layer_weights(eng, 5, 1)
        deep, one = _deep(_deep_weights(eng, 5, 3, 2)), MLPPolicy(w.w2, w.b2, w.w1, w.b1)
        noise = _noise(eng)[0]
        ids = []
        for pol, nz in ((deep, None), (one, None), (deep, noise), (one, noise), (deep, None)):
            eng.rollout_policy(3, pol, noise=nz)
            ids.append(eng.last_kernel())
        eng.close()
        assert ids[0] == ids[2] == ids[4] == _expected_kernel(case), (case, ids)  # one deep kernel, with or without noise
        assert ids[1] in L.POLICY_KERNEL_NAMES and ids[3] in L.POLICY_NOISY_KERNEL_NAMES, (case, ids)
        seen[case] = ids[0]
    assert set(seen.values()) == {L.KERNEL_PEND_POLICY_DEEP, L.KERNEL_BODY_POLICY_DEEP, L.KERNEL_BODY_POLICY_DEEP_RK4} == {21, 22, 23}
