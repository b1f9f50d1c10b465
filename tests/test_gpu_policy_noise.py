"""emei_rollout_policy_noisy on the GPU (pend_policy_rollout_noisy_kernel / body_policy_rollout_noisy_kernel) against
tests/policy_noise_reference.py.

Shapes as tests/test_gpu_policy.py: N = 130 for the 4-state family (two full waves and a ragged one), N = 70 for the bodies,
env_index_offset 4000, short TimeLimits so that auto-resets happen inside T.  T = 19 with hidden in {0, 5, 64} on one env of each
family, (19, 64) and (7, 0) on the others (the HalfCheetah: T = 6: six components, two Philox blocks).  The two sweep cases use a
seed three below 2^64, so that seed + t wraps inside the call.  A case runs once and is shared by the tests that read it.

Stream identity pins key, counter, k = 0, g and the component mapping against the sampling kernel without a host transcendental.
Parity (a per-component std under CLIP, epsilon-greedy): everything equals the per-step loop bit for bit, the loop's normals being the
device's (PolicyNoise.draws), its discrete flags the CPU Philox's.  Replay holds in every mode.  GAUSS_HEAD is not pinned bit for bit:
teacher-forced on the rows the policy saw it lies within a derived bound (see test_head_teacher_forced)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import policy_noise_reference as NR
import policy_reference as PR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BODY = dict(freq_rate=4, real_time_scale=0.002)
OFFSET = 4000
CASES = {
    "cartpole-balancing": dict(env="CartPoleBalancing", n=130, kw={}, bias=3.0),
    "cartpole-swingup-tl5": dict(env="CartPoleSwingUp", n=130, kw=dict(max_episode_steps=5), seed=2 ** 64 - 3),
    "ip-rebound-swingup": dict(env="ReboundInvertedPendulumSwingUp", n=130, kw=dict(max_episode_steps=6)),  # ctrlrange +-3
    "ip-boundary-balancing-rk4": dict(env="BoundaryInvertedPendulumBalancing", n=70, kw=dict(integrator="rk4", init_noise=0.2, max_episode_steps=9)),
    "idp-ref": dict(env="ReboundInvertedDoublePendulumSwingUp", n=70, kw=dict(max_episode_steps=6, init_noise=0.05), seed=2 ** 64 - 3),
    "idp-f32": dict(env="ReboundInvertedDoublePendulumSwingUp", n=70, kw=dict(max_episode_steps=6, init_noise=0.05, precision="f32")),
    "cheetah": dict(env="HalfCheetahRunning", n=70, kw=dict(max_episode_steps=4, init_noise=0.1, **BODY), T=6),
    "hopper": dict(env="HopperRunning", n=70, kw=dict(max_episode_steps=5, init_noise=0.01, **BODY)),
}
EPSILON = 0.25
SWEEP = ("cartpole-swingup-tl5", "idp-ref")
SHAPES = [(c, 19, h) for c in SWEEP for h in (0, 5, 64)] + \
         [(c, min(T, CASES[c].get("T", T)), h) for c in CASES if c not in SWEEP for T, h in ((19, 64), (7, 0))]
CONTINUOUS = [c for c in CASES if not CASES[c]["env"].startswith("CartPole")]
STREAM_CASES = ("ip-rebound-swingup", "hopper", "cheetah")


def _seed(case):
    return CASES[case].get("seed", 77 + len(case))


def _engine(case, **over):
    from emei_amd.engine import Engine

    c = CASES[case]
    kw = dict(seed=11, env_index_offset=OFFSET)
    kw.update(c["kw"])
    kw.update(over)
    n = kw.pop("n", c["n"])
    eng = Engine(c["env"], n, **kw)
    eng.reset(11)
    return eng


def _policy(eng, case, hidden, out="clip", zero=False):
    """(MLPPolicy on the device, the same weights as numpy arrays for the reference); zero: the affine policy y = 0"""
    from emei_amd.policy import MLPPolicy

    rng = np.random.default_rng(1000 + 17 * hidden + len(case))
    n_out = max(eng.act_dim, 1)
    f = lambda *s: (rng.standard_normal(s) * 1.5 / np.sqrt(s[-1])).astype(np.float32)
    b2 = f(n_out).reshape(n_out) + np.float32(CASES[case].get("bias", 0.0))
    if zero:
        w = dict(w2=np.zeros((n_out, eng.obs_dim), np.float32), b2=np.zeros(n_out, np.float32), w1=None, b1=None)
    elif hidden == 0:
        w = dict(w2=f(n_out, eng.obs_dim), b2=b2, w1=None, b1=None)
    else:
        w = dict(w2=f(n_out, hidden), b2=b2, w1=f(hidden, eng.obs_dim), b1=f(hidden).reshape(hidden))
    return MLPPolicy(out=out, **w), types.SimpleNamespace(out=out, **w)


def _noise(eng, case, mode, hidden):
    """(PolicyNoise, its description for the reference).  mode: "gauss" (a std per component) / "sigma" (one std, std NULL) /
    "head" / "eps" / "zero" (std 0 or epsilon 0)"""
    from emei_amd.policy import PolicyNoise

    seed, n_out = _seed(case), max(eng.act_dim, 1)
    if eng.act_dim == 0:
        eps = 0.0 if mode == "zero" else EPSILON
        return PolicyNoise(seed, epsilon=eps), types.SimpleNamespace(mode="eps", seed=seed, epsilon=eps)
    if mode == "head":
        rng = np.random.default_rng(5 + hidden)
        n_in = hidden if hidden else eng.obs_dim
        ws = (rng.standard_normal((n_out, n_in)) * 2.0 / np.sqrt(n_in)).astype(np.float32)  # wide enough to reach the clamp's ends
        bs = (rng.standard_normal(n_out) - 1.0).astype(np.float32)
        rg = (-3.0, 0.5)
        return (PolicyNoise(seed, log_std_head=(ws, bs), log_std_range=rg),
                types.SimpleNamespace(mode="head", seed=seed, ws=ws, bs=bs, log_std_min=rg[0], log_std_max=rg[1]))
    if mode == "gauss":
        std = (0.1 + 0.3 * np.arange(1, n_out + 1, dtype=np.float32) / n_out).astype(np.float32)
        return PolicyNoise(seed, std=std), types.SimpleNamespace(mode="gauss", seed=seed, std=std)
    sigma = {"sigma": 0.125, "zero": 0.0}[mode]
    return PolicyNoise(seed, std=sigma), types.SimpleNamespace(mode="gauss", seed=seed, std=np.full(n_out, sigma, np.float32))


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


def _g(n, offset=OFFSET):
    return np.arange(offset, offset + n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _run(case, T, hidden, auto_reset, mode="gauss", out="clip", loop=True):
    """one start, frozen: [the per-step loop,] the noisy launch, the rows the policy saw and its draws, the replay"""
    eng = _engine(case)
    pol, ref = _policy(eng, case, hidden, out, zero=mode == "sigma")
    noise, nref = _noise(eng, case, mode, hidden)
    noise.bind(eng)
    eng.freeze()
    _, epi0 = eng.get_counters()
    res = dict(x0=eng.get_obs().to(torch.float32).cpu().numpy(), ref=ref, nref=nref, discrete=eng.act_dim == 0, env=eng.env_name)
    if loop:
        res["loop"] = NR.noisy_policy_loop(eng, T, ref, nref, lambda t: noise.draws(eng, t), auto_reset, _g(eng.n_envs))
        res["loop_end"] = _end(eng)
        _rewind(eng)
    act, obs, rew, done = eng.rollout_policy(T, pol, auto_reset=auto_reset, noise=noise)
    res["kernel"] = eng.last_kernel()
    res["fused"] = _np((act, obs, rew, done))
    res["fused_end"] = _end(eng)
    # the rows the policy saw: x_0, then every emitted row, or the new episode's first observation after an auto-reset
    seen = torch.cat([torch.as_tensor(res["x0"], device=eng.device)[None], obs[:-1]]).clone()
    if auto_reset and bool((done[:-1] != 0).any()):
        t_idx, e_idx = torch.nonzero(done[:-1] != 0, as_tuple=True)
        episodes = epi0[None, :].to(torch.int64) + torch.cumsum((done != 0).to(torch.int64), dim=0)
        seen[t_idx + 1, e_idx] = eng.episode_init_obs(e_idx, episodes[t_idx, e_idx])
    res["seen"] = seen.cpu().numpy()
    if eng.act_dim > 0:
        res["z"] = np.stack([noise.draws(eng, t).cpu().numpy().reshape(eng.n_envs, -1) for t in range(T)])
    _rewind(eng)
    o2, r2, d2 = eng.rollout(act, auto_reset=auto_reset)
    res["replay"] = dict(obs=o2.cpu().numpy(), reward=r2.cpu().numpy(), done=d2.cpu().numpy())
    res["replay_end"] = _end(eng)
    eng.close()
    return res


def _expected_kernel(case):
    from emei_amd import _lib as L

    if CASES[case]["n"] == 130:
        return L.KERNEL_PEND_POLICY_NOISY
    return L.KERNEL_BODY_POLICY_NOISY_RK4 if CASES[case]["kw"].get("integrator") == "rk4" else L.KERNEL_BODY_POLICY_NOISY


# ------------------------------------------------------------------------------------------------ 1. the stream
@pytest.mark.parametrize("case", STREAM_CASES)
def test_stream_identity(case):
    """y = 0 and std = 0.125: actions_out[t] IS candidate 0 of sample_candidates(1, 1, seed + t, zeros, 0.125), bit for bit; and
    8 * actions_out lies within boxmuller's bound (tests/test_gpu_device_math.py: 1.6e-6) of the exact normal of (seed, t, g)"""
    T = CASES[case].get("T", 19)
    eng = _engine(case)
    pol, _ = _policy(eng, case, 0, zero=True)
    noise, nref = _noise(eng, case, "sigma", 0)
    act = eng.rollout_policy(T, pol, auto_reset=True, noise=noise)[0]
    assert eng.last_kernel() == _expected_kernel(case)
    zeros = torch.zeros((1, eng.n_envs) + eng._act_tail, dtype=torch.float32, device=eng.device)
    n_out = max(eng.act_dim, 1)
    for t in range(T):
        want = eng.sample_candidates(1, 1, nref.seed + t, nominal=zeros, sigma=0.125)[0, :, 0]
        assert _same(act[t].cpu().numpy(), want.cpu().numpy()), t
    a = act.cpu().numpy().reshape(T, eng.n_envs, n_out)
    exact = np.stack([NR.normals_exact(nref.seed, t, _g(eng.n_envs), n_out) for t in range(T)])
    err = np.abs(8.0 * a.astype(np.float64) - exact)
    print(f"{case}: max |8 a - z_exact| = {err.max():.3e} (bound 1.6e-6)")
    assert err.max() <= 1.6e-6
    assert len(np.unique(a)) > a.size // 2  # distinct per step, env and component
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. parity, 3. replay
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("case,T,hidden", SHAPES)
def test_parity_with_the_per_step_loop(case, T, hidden, auto_reset):
    r = _run(case, T, hidden, auto_reset)
    loop, fused = r["loop"], r["fused"]
    want_act = loop["actions"] if r["discrete"] else loop["actions"].astype(np.float32)
    assert fused["actions"].shape == want_act.shape and _same(fused["actions"], want_act)
    for k in ("obs", "reward", "done"):
        assert _same(fused[k], loop[k]), k
    for k in ("state", "steps", "episode", "compact"):
        assert _same(r["fused_end"][k], r["loop_end"][k]), k
    assert r["kernel"] == _expected_kernel(case)
    assert _same(r["seen"], loop["seen"])  # the rows rebuilt from the outputs are the rows the loop's policy was shown
    if auto_reset and T > CASES[case]["kw"].get("max_episode_steps", T):
        assert fused["done"].any()  # the TimeLimit ran out inside T: the noise stream runs across a reset
    if r["discrete"] and T == 19:  # exploration happened: the actions part from the greedy ones where the flags say so
        n = fused["actions"].shape[1]
        flags = [NR.eps_greedy_flags(r["nref"].seed, t, _g(n), EPSILON) for t in range(T)]
        explore = np.stack([f[0] for f in flags])
        assert 0.15 < explore.mean() < 0.35
        greedy = np.stack([PR.mlp_actions(r["ref"], r["seen"][t], -1, 1, True) for t in range(T)])
        assert (fused["actions"] != greedy).any() and np.array_equal(fused["actions"][~explore], greedy[~explore])


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("case,T,hidden", SHAPES)
def test_replaying_the_actions_reproduces_the_outputs(case, T, hidden, auto_reset):
    r = _run(case, T, hidden, auto_reset)
    for k in ("obs", "reward", "done"):
        assert _same(r["fused"][k], r["replay"][k]), k
    for k in ("state", "steps", "episode", "compact"):
        assert _same(r["fused_end"][k], r["replay_end"][k]), k


@pytest.mark.parametrize("mode,out", [("gauss", "tanh"), ("head", "clip"), ("head", "tanh")])
@pytest.mark.parametrize("case", CONTINUOUS)
def test_replay_in_the_modes_that_are_not_pinned(case, mode, out):
    r = _run(case, CASES[case].get("T", 19), 64, True, mode, out, False)
    for k in ("obs", "reward", "done"):
        assert _same(r["fused"][k], r["replay"][k]), k
    for k in ("state", "steps", "episode", "compact"):
        assert _same(r["fused_end"][k], r["replay_end"][k]), k


# ------------------------------------------------------------------------------------------------ 4. the log-std head
@pytest.mark.parametrize("hidden", [64, 0])
@pytest.mark.parametrize("out", ["clip", "tanh"])
@pytest.mark.parametrize("case", CONTINUOUS)
def test_head_teacher_forced(case, out, hidden):
    """The numpy clause on the rows the policy saw, with the device's normals.  The device's float64 exp is accurate to a few
    float64 ulps, so s differs from the reference's by at most one float32 ulp of s (the rounding to float32 can flip), and the
    final float32 rounding of y + s z can flip by one spacing: under CLIP |a - a_ref| <= 2^-23 (s_ref |z| + |y_ref|) + the smallest
    subnormal.  Under TANH: test_gpu_policy.py's one spacing at max(|lo|, |hi|), plus half * 2^-23 * s_ref |z| (|d tanh| <= 1)."""
    T = min(CASES[case].get("T", 19), 19 if hidden else 7)
    r = _run(case, T, hidden, True, "head", out, False)
    f, seen, z = r["fused"], r["seen"], r["z"]
    lo, hi = PR.ctrl_range(r["env"])
    rows = seen.reshape(-1, seen.shape[-1])
    yn, y, s = NR.noisy_logits(r["ref"], r["nref"], rows, z.reshape(rows.shape[0], -1))
    want = NR.output_clause(yn, out, lo, hi).reshape(z.shape)
    got = f["actions"].reshape(z.shape)
    sz = (s.astype(np.float64) * np.abs(z.reshape(s.shape)).astype(np.float64)).reshape(z.shape)
    if out == "clip":
        tol = 2.0 ** -23 * (sz + np.abs(y).reshape(z.shape)) + float(np.finfo(np.float32).smallest_subnormal)
    else:
        tol = float(np.spacing(np.float32(max(abs(lo), abs(hi))))) + 0.5 * (float(hi) - float(lo)) * 2.0 ** -23 * sz
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{case} {out} hidden={hidden}: max |a - ref| = {err.max():.3e}, max err / bound = {(err / tol).max():.3f}, "
          f"{np.mean(err > 0):.4f} of the entries differ")
    assert (err <= tol).all(), float((err - tol).max())
    # the head is exercised: its scale stays inside the clamp and varies over the rows
    assert s.min() >= np.float32(np.exp(-3.0)) and s.max() <= np.float32(np.exp(0.5)) and len(np.unique(s)) > 10


# ------------------------------------------------------------------------------------------------ 5. zero noise
@pytest.mark.parametrize("case", ["cartpole-balancing", "ip-rebound-swingup", "hopper", "ip-boundary-balancing-rk4"])
def test_zero_noise_is_the_deterministic_rollout(case):
    eng = _engine(case)
    pol, _ = _policy(eng, case, 64)
    noise, _ = _noise(eng, case, "zero", 64)
    eng.freeze()
    det = _np(eng.rollout_policy(19, pol, auto_reset=True))
    det_end = _end(eng)
    _rewind(eng)
    got = _np(eng.rollout_policy(19, pol, auto_reset=True, noise=noise))
    assert eng.last_kernel() == _expected_kernel(case)
    for k in det:
        assert np.array_equal(got[k], det[k]), k
    end = _end(eng)
    for k in end:
        assert np.array_equal(end[k], det_end[k]), k
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. chunking
@pytest.mark.parametrize("a,b", [(1, 6), (8, 11)])
@pytest.mark.parametrize("case", SWEEP)
def test_chunking(case, a, b):
    """(a + b, seed) against (a, seed) then (b, seed + a).  It holds where (float)get_obs() equals the row the last step emitted:
    asserted first, as tests/test_gpu_policy.py does."""
    from emei_amd.policy import PolicyNoise

    eng = _engine(case, max_episode_steps=0)  # no TimeLimit: nothing is reset between the chunks
    pol, _ = _policy(eng, case, 64)
    noise, nref = _noise(eng, case, "gauss", 64)
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
    # ... and the second chunk under the FIRST chunk's seed is another trajectory: the key of step t is seed + t
    _rewind(eng)
    eng.rollout_policy(a, pol, noise=PolicyNoise(nref.seed, **kw))
    other = eng.rollout_policy(b, pol, noise=PolicyNoise(nref.seed, **kw))[0].cpu().numpy()
    assert not _same(other, second[0])
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. shards
@pytest.mark.parametrize("case", ["cartpole-balancing", "ip-rebound-swingup", "idp-ref"])
def test_shard_invariance(case):
    """envs 64.. of the full run on a handle of their own with env_index_offset + 64: the same bits as the full run's columns 64.."""
    T, n = 19, CASES[case]["n"]
    full = _run(case, T, 64, True)
    eng = _engine(case, n=n - 64, env_index_offset=OFFSET + 64)
    pol, _ = _policy(eng, case, 64)
    noise, _ = _noise(eng, case, "gauss", 64)
    part = _np(eng.rollout_policy(T, pol, auto_reset=True, noise=noise))
    for k in part:
        assert _same(part[k], np.ascontiguousarray(full["fused"][k][:, 64:])), k
    assert _same(_end(eng)["state"], full["fused_end"]["state"][64:])
    assert part["done"].any()  # some env was reset: the reset stream is part of what is compared
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. NULL outputs
@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper"])
def test_null_outputs_one_at_a_time(case):
    from emei_amd import _lib as L
    from emei_amd.engine import _ACT_DTYPES, _ptr, _stream

    T = 7
    ref = _run(case, T, 0, True)
    full, full_end = ref["fused"], ref["fused_end"]
    eng = _engine(case)
    pol, _ = _policy(eng, case, 0)
    noise, _ = _noise(eng, case, "gauss", 0)
    pol.bind(eng), noise.bind(eng)
    eng.freeze()
    names = ("actions", "obs", "reward", "done")
    for skip in names:
        _rewind(eng)
        obs, rew, done = eng.alloc_outputs(T)
        act = torch.empty(full["actions"].shape, dtype=torch.int64 if eng.act_dim == 0 else torch.float32, device=eng.device)
        bufs = dict(actions=act, obs=obs, reward=rew, done=done)
        p = {k: (None if k == skip else _ptr(v)) for k, v in bufs.items()}
        ps, ns = pol.struct(), noise.struct()
        with torch.cuda.device(eng.device):
            L.check(L.lib().emei_rollout_policy_noisy(eng._h, T, C.byref(ps), C.byref(ns), p["actions"], _ACT_DTYPES[act.dtype], p["obs"],
                                                      p["reward"], p["done"], L.FLAG_AUTO_RESET, _stream()))
        torch.cuda.synchronize()
        for k in names:
            if k != skip:
                assert _same(bufs[k].cpu().numpy(), full[k]), (skip, k)
        end = _end(eng)
        for k in end:
            assert _same(end[k], full_end[k]), (skip, k)
    eng.close()


# ------------------------------------------------------------------------------------------------ 9. refusals that need a handle
def _raw_call(eng, pol, ns, T=3):
    from emei_amd import _lib as L
    from emei_amd.engine import _ACT_DTYPES, _ptr, _stream

    obs, rew, done = eng.alloc_outputs(T)
    dtype = torch.int64 if eng.act_dim == 0 else torch.float32
    act = torch.empty((T, eng.n_envs) + eng._act_tail, dtype=dtype, device=eng.device)
    ps = pol.bind(eng).struct()
    with torch.cuda.device(eng.device):
        rc = L.lib().emei_rollout_policy_noisy(eng._h, T, C.byref(ps), C.byref(ns), _ptr(act), _ACT_DTYPES[dtype], _ptr(obs), _ptr(rew),
                                               _ptr(done), 0, _stream())
    torch.cuda.synchronize()
    return rc, L.lib().emei_last_error().decode()


def test_the_mode_must_fit_the_env_kind():
    from emei_amd import _lib as L
    from emei_amd.policy import PolicyNoise

    for case, good, bad in (("cartpole-swingup-tl5", dict(epsilon=0.25), dict(std=0.1)), ("hopper", dict(std=0.1), dict(epsilon=0.25))):
        eng = _engine(case)
        pol, _ = _policy(eng, case, 5)
        before = _end(eng)
        with pytest.raises(ValueError, match="discrete envs"):  # PolicyNoise.bind, before the ABI is reached
            eng.rollout_policy(3, pol, noise=PolicyNoise(1, **bad))
        rc, msg = _raw_call(eng, pol, PolicyNoise(1, **bad).struct())  # ... and the ABI's own refusal
        assert rc == L.ERR_INVALID and msg.startswith("emei_rollout_policy_noisy:") and "noise.mode" in msg, msg
        if eng.act_dim > 0:  # the log-std head is a Gaussian mode too; a discrete env refuses it
            rc, msg = _raw_call(eng, pol, PolicyNoise(1, **good).struct())
            assert rc == L.OK, msg
        else:
            head = PolicyNoise(1, log_std_head=(np.zeros((1, 5), np.float32), np.zeros(1, np.float32))).bind(types.SimpleNamespace(
                act_dim=1, env_name="x", device=eng.device))
            rc, msg = _raw_call(eng, pol, head.struct())
            assert rc == L.ERR_INVALID and "noise.mode" in msg, msg
            after = _end(eng)
            assert all(_same(before[k], after[k]) for k in ("state", "steps", "episode"))
        eng.close()


def test_a_handle_with_peers_is_refused():
    eng = _engine("cartpole-swingup-tl5", n=128)
    pol, _ = _policy(eng, "cartpole-swingup-tl5", 5)
    noise, _ = _noise(eng, "cartpole-swingup-tl5", "gauss", 5)
    buf = torch.zeros((32, 128, 4), dtype=torch.float32, device=eng.device)
    eng.set_obs_peers([buf], 128, 0)
    before = _end(eng)
    with pytest.raises(NotImplementedError, match="emei_rollout_policy_noisy: observation peers"):
        eng.rollout_policy(7, pol, noise=noise)
    after = _end(eng)
    assert all(_same(before[k], after[k]) for k in ("state", "steps", "episode")) and not buf.any()
    eng.set_obs_peers([], 128, 0)
    eng.rollout_policy(7, pol, noise=noise)  # ... and served again without them
    eng.close()


# ------------------------------------------------------------------------------------------------ 10. collect
@pytest.mark.parametrize("name,kw,T", [("CartPoleBalancing-v0", dict(num_envs=130, max_episode_steps=30), 40),
                                       ("HopperRunning-v0", dict(num_envs=70, max_episode_steps=5), 12)])
def test_collect_with_noise_takes_the_one_launch_route(name, kw, T):
    import emei_amd
    from emei_amd import _lib as L, datasets
    from emei_amd.policy import PolicyNoise

    env_a, env_b = emei_amd.make(name, **kw), emei_amd.make(name, **kw)
    case = "cartpole-balancing" if name.startswith("CartPole") else "hopper"
    pol, _ = _policy(env_a.engine, case, 64)
    nkw = dict(epsilon=EPSILON) if name.startswith("CartPole") else dict(std=[0.1, 0.2, 0.3])
    data, info = datasets.collect(env_a, T, policy=pol, noise=PolicyNoise(9, **nkw), seed=3)
    assert env_a.engine.last_kernel() in (L.KERNEL_PEND_POLICY_NOISY, L.KERNEL_BODY_POLICY_NOISY, L.KERNEL_BODY_POLICY_NOISY_RK4)
    assert set(data) == set(datasets.DATASET_KEYS) and info["total_episode_num"] > 0
    N, eng = kw["num_envs"], env_b.engine
    # the same start (collect resets with the seed), the direct call
    env_b.reset(seed=3, options={"device_rng": True})
    _, epi0 = eng.get_counters()
    x0 = eng.get_obs().to(torch.float32)
    act, obs, rew, done = eng.rollout_policy(T, pol, auto_reset=True, noise=PolicyNoise(9, **nkw))
    em = lambda x: x.transpose(0, 1).reshape((N * T,) + tuple(x.shape[2:]))  # env-major rows, as collect lays them out
    a = act if act.dim() == 3 else act[..., None]
    assert _same(data["actions"].cpu().numpy(), em(a.to(torch.float32) if eng.act_dim else a).cpu().numpy())
    assert _same(data["next_observations"].cpu().numpy(), em(obs).cpu().numpy()) and _same(data["rewards"].cpu().numpy(), em(rew).cpu().numpy())
    # observations[t + 1] == next_observations[t] within an episode, the rebuilt first observation after a reset
    o = data["observations"].reshape(N, T, -1)
    no = data["next_observations"].reshape(N, T, -1)
    d = data["dones"].reshape(N, T) != 0
    assert torch.equal(o[:, 0], x0) and d.any()
    inside = ~d[:, :-1]
    assert torch.equal(o[:, 1:][inside], no[:, :-1][inside])
    e_idx, t_idx = torch.nonzero(d[:, :-1], as_tuple=True)
    episodes = epi0[:, None].to(torch.int64) + torch.cumsum(d.to(torch.int64), dim=1)
    assert torch.equal(o[e_idx, t_idx + 1], eng.episode_init_obs(e_idx, episodes[e_idx, t_idx]))
    # noise= with any other action source is refused
    for other in (dict(policy=lambda ob: pol(ob)), dict(actions=act), dict()):
        with pytest.raises(ValueError, match="noise="):
            datasets.collect(env_b, T, noise=PolicyNoise(9, **nkw), **other)
    # the env-level call takes it too
    out = env_a.rollout_policy(5, pol, noise=PolicyNoise(9, **nkw))
    assert out[2].dtype == torch.bool and out[4].shape[:2] == (5, N)


def test_last_kernel_reports_the_new_ids():
    from emei_amd import _lib as L

    got = {c: _run(c, T, h, False)["kernel"] for c, T, h in SHAPES if h == 64}
    assert set(got.values()) == {L.KERNEL_PEND_POLICY_NOISY, L.KERNEL_BODY_POLICY_NOISY, L.KERNEL_BODY_POLICY_NOISY_RK4} == {18, 19, 20}
    for c, k in got.items():
        assert k == _expected_kernel(c) and "noisy" in L.kernel_name(k), c


def test_the_callable_is_the_launch():
    """MLPPolicy.__call__(obs, noise, t) on the rows the policy saw gives the launch's actions (CLIP, a given std; the discrete envs)"""
    for case in ("cartpole-balancing", "hopper"):
        r = _run(case, 7, 0, True)
        eng = _engine(case)
        pol, _ = _policy(eng, case, 0)
        noise, _ = _noise(eng, case, "gauss", 0)
        pol.bind(eng), noise.bind(eng)
        for t in range(7):
            a = pol(torch.as_tensor(r["seen"][t], device=eng.device), noise, t)
            assert _same(a.cpu().numpy(), r["fused"]["actions"][t]), (case, t)
        with pytest.raises(ValueError, match="together"):
            pol(torch.as_tensor(r["seen"][0], device=eng.device), noise)
        eng.close()
