"""emei_rollout_policy on the GPU (pend_policy_rollout_kernel / body_policy_rollout_kernel) against tests/policy_reference.py.

Shapes: N = 130 for the 4-state family (one 256-thread block: two full waves and a ragged one of 2 lanes), N = 70 for the bodies (a full
wave and a ragged one), T in {1, 7, 8, 19} and hidden in {0, 1, 5, 64} in full on one env of each family, (19, 64) and (7, 0) on the
others (the HalfCheetah: T = 6).  A case runs once (the loop, the one launch, the replay) and is shared by the tests that read it.

Parity (CLIP and the discrete envs): actions, observations, rewards, done codes, the state, the counters and compact_done() equal the
per-step loop bit for bit.  Replay (either out mode): rollout(actions_out) from the same start gives the other three outputs bit for
bit.  TANH: the device's float64 tanh is not pinned; the action rounds a float64 value that is accurate to a few float64 ulps on either
side, so the two float32 results lie within ONE float32 spacing at max(|lo|, |hi|) — a derived bound, not a measurement."""
import ctypes as C
import functools

import numpy as np
import pytest

import policy_reference as PR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BODY = dict(freq_rate=4, real_time_scale=0.002)
CASES = {
    # terminal resets at staggered times: a large positive bias pushes one way, the pole falls within ~10 steps
    "cartpole-balancing": dict(env="CartPoleBalancing", n=130, kw={}, bias=3.0),
    "cartpole-swingup-tl5": dict(env="CartPoleSwingUp", n=130, kw=dict(max_episode_steps=5)),  # every lane truncates at once
    "cartpole-swingup-rk4": dict(env="CartPoleSwingUp", n=130, kw=dict(ode_method="rk4", max_episode_steps=11)),
    "ip-rebound-swingup": dict(env="ReboundInvertedPendulumSwingUp", n=130, kw=dict(max_episode_steps=6)),  # its own 4-state kernel
    "ip-boundary-balancing-rk4": dict(env="BoundaryInvertedPendulumBalancing", n=70, kw=dict(integrator="rk4", init_noise=0.2, max_episode_steps=9)),
    "idp-ref": dict(env="ReboundInvertedDoublePendulumSwingUp", n=70, kw=dict(max_episode_steps=6, init_noise=0.05)),
    "idp-f32": dict(env="ReboundInvertedDoublePendulumSwingUp", n=70, kw=dict(max_episode_steps=6, init_noise=0.05, precision="f32")),
    "cheetah": dict(env="HalfCheetahRunning", n=70, kw=dict(max_episode_steps=4, init_noise=0.1, **BODY), T=6),
    "hopper-noise": dict(env="HopperRunning", n=70, kw=dict(max_episode_steps=5, init_noise=0.01, obs_noise=0.01, **BODY)),
}
SWEEP = ("cartpole-swingup-tl5", "idp-ref")
SHAPES = [(c, T, h) for c in SWEEP for T in (1, 7, 8, 19) for h in (0, 1, 5, 64)] + \
         [(c, min(T, CASES[c].get("T", T)), h) for c in CASES if c not in SWEEP for T, h in ((19, 64), (7, 0))]
TANH_CASES = [c for c in CASES if not CASES[c]["env"].startswith("CartPole")]


def _engine(case, **over):
    from emei_amd.engine import Engine

    c = CASES[case]
    kw = dict(seed=11, env_index_offset=4000)
    kw.update(c["kw"])
    kw.update(over)
    n = kw.pop("n", c["n"])
    eng = Engine(c["env"], n, **kw)
    eng.reset(11)
    return eng


def _policy(eng, case, hidden, out="clip"):
    """(MLPPolicy on the device, the same weights as numpy arrays for the reference)"""
    from emei_amd.policy import MLPPolicy

    rng = np.random.default_rng(1000 + 17 * hidden + len(case))
    n_out = max(eng.act_dim, 1)
    f = lambda *s: (rng.standard_normal(s) * 1.5 / np.sqrt(s[-1])).astype(np.float32)
    b2 = f(n_out).reshape(n_out) + np.float32(CASES[case].get("bias", 0.0))
    if hidden == 0:
        w = dict(w2=f(n_out, eng.obs_dim), b2=b2, w1=None, b1=None)
    else:
        w = dict(w2=f(n_out, hidden), b2=b2, w1=f(hidden, eng.obs_dim), b1=f(hidden).reshape(hidden))
    pol = MLPPolicy(out=out, **w)
    ref = type("Ref", (), dict(w, out=out))
    return pol, ref


def _rewind(eng):
    """back to the frozen start, which stays frozen (unfreeze() gives the snapshot up)"""
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


@functools.lru_cache(maxsize=None)
def _run(case, T, hidden, auto_reset, out="clip"):
    eng = _engine(case)
    pol, ref = _policy(eng, case, hidden, out)
    eng.freeze()
    x0 = eng.get_obs().to(torch.float32).cpu().numpy()
    res = dict(x0=x0)
    if out == "clip":  # the tanh mode is not pinned bit for bit: its trajectories may part from a host loop's
        res["loop"] = PR.policy_loop(eng, T, ref, auto_reset)
        res["loop_end"] = _end(eng)
        _rewind(eng)
    act, obs, rew, done = eng.rollout_policy(T, pol, auto_reset=auto_reset)
    res["kernel"] = eng.last_kernel()
    res["fused"] = dict(actions=act.cpu().numpy(), obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), done=done.cpu().numpy())
    res["fused_end"] = _end(eng)
    _rewind(eng)
    o2, r2, d2 = eng.rollout(act, auto_reset=auto_reset)
    res["replay"] = dict(obs=o2.cpu().numpy(), reward=r2.cpu().numpy(), done=d2.cpu().numpy())
    res["replay_end"] = _end(eng)
    res["ref"], res["discrete"], res["env"] = ref, eng.act_dim == 0, eng.env_name
    eng.close()
    return res


def _expected_kernel(case):
    from emei_amd import _lib as L

    kw = CASES[case]["kw"]
    if CASES[case]["n"] == 130:
        return L.KERNEL_PEND_POLICY
    return L.KERNEL_BODY_POLICY_RK4 if kw.get("integrator") == "rk4" else L.KERNEL_BODY_POLICY


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
    if T == 19:  # the case does what it is there for
        d = fused["done"]
        if auto_reset or case == "cartpole-balancing":
            assert d.any()
        if case == "cartpole-balancing":
            first = np.argmax(d != 0, axis=0)
            assert (d & 1).any(axis=0).mean() > 0.9 and len(np.unique(first)) >= 2  # terminal, at staggered times
        if case == "cartpole-swingup-tl5" and auto_reset:
            assert (d[4] == 2).all() and (d[9] == 2).all() and not d[:4].any()


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("case,T,hidden", SHAPES)
def test_replaying_the_actions_reproduces_the_outputs(case, T, hidden, auto_reset):
    r = _run(case, T, hidden, auto_reset)
    for k in ("obs", "reward", "done"):
        assert _same(r["fused"][k], r["replay"][k]), k
    for k in ("state", "steps", "episode", "compact"):
        assert _same(r["fused_end"][k], r["replay_end"][k]), k


@pytest.mark.parametrize("case", TANH_CASES)
def test_tanh_mode(case):
    T = CASES[case].get("T", 19)
    r = _run(case, T, 64, False, "tanh")
    f = r["fused"]
    for k in ("obs", "reward", "done"):  # replay holds in every out mode
        assert _same(f[k], r["replay"][k]), k
    seen = np.concatenate([r["x0"][None], f["obs"][:-1]])  # no auto-reset: the policy saw x_0, then every emitted row
    lo, hi = PR.ctrl_range(r["env"])
    want = PR.mlp_actions(r["ref"], seen.reshape(-1, seen.shape[-1]), lo, hi, False).reshape(f["actions"].shape)
    tol = np.spacing(np.float32(max(abs(lo), abs(hi))))
    err = np.abs(f["actions"].astype(np.float64) - want.astype(np.float64))
    print(f"{case}: max |action - reference| = {err.max():.3e} (bound {tol:.3e}), {np.mean(err > 0):.3f} of the entries differ")
    assert err.max() <= tol
    assert (np.abs(f["actions"]) <= hi).all() and (np.abs(f["actions"]) < hi).any()


@pytest.mark.parametrize("case", SWEEP)
def test_chunking(case):
    """(7, 12) against 19.  It holds where (float)get_obs() equals the row the last step emitted: asserted first."""
    eng = _engine(case, max_episode_steps=0)  # no TimeLimit: nothing is reset between the chunks
    pol, _ = _policy(eng, case, 64)
    eng.freeze()
    whole = [t.cpu().numpy() for t in eng.rollout_policy(19, pol)]
    end_whole = _end(eng)
    _rewind(eng)
    first = [t.cpu().numpy() for t in eng.rollout_policy(7, pol)]
    getter = eng.get_obs().to(torch.float32).cpu().numpy()
    assert _same(getter, first[1][-1]), "precondition: the getter's row is the emitted row"
    second = [t.cpu().numpy() for t in eng.rollout_policy(12, pol)]
    for w, a, b in zip(whole, first, second):
        assert _same(w, np.concatenate([a, b]))
    end = _end(eng)
    for k in end:
        assert _same(end[k], end_whole[k]), k
    eng.close()


@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-noise"])
def test_null_outputs_one_at_a_time(case):
    from emei_amd import _lib as L
    from emei_amd.engine import _ACT_DTYPES, _ptr, _stream

    T = 7
    full = _run(case, T, 5, True)["fused"]
    eng = _engine(case)
    pol, _ = _policy(eng, case, 5)
    pol.bind(eng)
    eng.freeze()
    names = ("actions", "obs", "reward", "done")
    for skip in names:
        _rewind(eng)
        obs, rew, done = eng.alloc_outputs(T)
        act = torch.empty(full["actions"].shape, dtype=torch.int64 if eng.act_dim == 0 else torch.float32, device=eng.device)
        bufs = dict(actions=act, obs=obs, reward=rew, done=done)
        p = {k: (None if k == skip else _ptr(v)) for k, v in bufs.items()}
        ps = pol.struct()
        with torch.cuda.device(eng.device):
            L.check(L.lib().emei_rollout_policy(eng._h, T, C.byref(ps), p["actions"], _ACT_DTYPES[act.dtype], p["obs"], p["reward"],
                                                p["done"], L.FLAG_AUTO_RESET, _stream()))
        torch.cuda.synchronize()
        for k in names:
            if k != skip:
                assert _same(bufs[k].cpu().numpy(), full[k]), (skip, k)
    eng.close()


def test_last_kernel_reports_the_new_ids():
    from emei_amd import _lib as L

    got = {c: _run(c, T, h, False)["kernel"] for c, T, h in SHAPES if h in (0, 64) and T >= 6}
    assert set(got.values()) == {L.KERNEL_PEND_POLICY, L.KERNEL_BODY_POLICY, L.KERNEL_BODY_POLICY_RK4} == {15, 16, 17}
    for c, k in got.items():
        assert k == _expected_kernel(c) and "policy" in L.kernel_name(k), c


def test_the_clip_is_exercised():
    """over the continuous cases the CLIP parity covers, actions lie both inside the ctrlrange and on its bounds"""
    inside = clipped = 0
    for c, T, h in SHAPES:
        r = _run(c, T, h, True)
        if not r["discrete"]:
            lo, hi = PR.ctrl_range(r["env"])
            a = r["fused"]["actions"]
            inside += int(((a > lo) & (a < hi)).sum())
            clipped += int(((a == lo) | (a == hi)).sum())
    assert inside > 100 and clipped > 100, (inside, clipped)


def test_a_handle_with_peers_is_refused():
    eng = _engine("cartpole-swingup-tl5", n=128)
    pol, _ = _policy(eng, "cartpole-swingup-tl5", 5)
    buf = torch.zeros((32, 128, 4), dtype=torch.float32, device=eng.device)
    eng.set_obs_peers([buf], 128, 0)
    before = _end(eng)
    with pytest.raises(NotImplementedError, match="emei_rollout_policy: observation peers"):
        eng.rollout_policy(7, pol)
    after = _end(eng)
    assert all(_same(before[k], after[k]) for k in ("state", "steps", "episode")) and not buf.any()
    eng.set_obs_peers([], 128, 0)
    eng.rollout_policy(7, pol)  # ... and served again without them
    eng.close()


@pytest.mark.parametrize("case", ["cartpole-balancing", "idp-ref"])
def test_shard_invariance(case):
    """envs [0, 64) and [64, 128) as two engines with env_index_offset against one engine of 128"""
    T = 19
    outs = []
    for n, offs in ((128, (4000,)), (64, (4000, 4064))):
        parts = []
        for off in offs:
            eng = _engine(case, n=n, env_index_offset=off)
            pol, _ = _policy(eng, case, 64)
            parts.append([t.cpu().numpy() for t in eng.rollout_policy(T, pol, auto_reset=True)] + [_end(eng)["state"][None]])
            eng.close()
        outs.append([np.concatenate([p[k] for p in parts], axis=1) for k in range(5)])
    assert outs[0][3].any()  # some env was reset: the reset stream is part of what is compared
    for a, b in zip(*outs):
        assert _same(a, b)


@pytest.mark.parametrize("name,kw,T", [("CartPoleBalancing-v0", dict(num_envs=130, max_episode_steps=30), 40),
                                       ("HopperRunning-v0", dict(num_envs=70, max_episode_steps=5), 12)])
def test_collect_takes_the_one_launch_route(name, kw, T):
    """datasets.collect(policy=MLPPolicy) equals collect with the same object behind a lambda (the per-step loop), key for key"""
    import emei_amd
    from emei_amd import _lib as L, datasets

    env_a, env_b = emei_amd.make(name, **kw), emei_amd.make(name, **kw)
    case = "cartpole-balancing" if name.startswith("CartPole") else "hopper-noise"
    pol, _ = _policy(env_a.engine, case, 64)
    da, ia = datasets.collect(env_a, T, policy=pol, seed=3)
    fused_ids = (L.KERNEL_PEND_POLICY, L.KERNEL_BODY_POLICY, L.KERNEL_BODY_POLICY_RK4)
    assert env_a.engine.last_kernel() in fused_ids
    pol.bind(env_b.engine)
    db, ib = datasets.collect(env_b, T, policy=lambda o: pol(o), seed=3)
    assert env_b.engine.last_kernel() not in fused_ids
    assert set(da) == set(db) == set(datasets.DATASET_KEYS) and ia == ib and ia["total_episode_num"] > 0
    for k in da:
        assert da[k].dtype == db[k].dtype and _same(da[k].cpu().numpy(), db[k].cpu().numpy()), k
    obs, rew, term, trunc, act = env_a.rollout_policy(5, pol)  # the env-level call: rollout's conventions plus the actions
    assert term.dtype == torch.bool and trunc.dtype == torch.bool and obs.shape[:2] == act.shape[:2] == rew.shape == (5, kw["num_envs"])
