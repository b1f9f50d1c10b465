"""emei_mpc_policy on the GPU (Engine.mpc_policy / HipEnv.mpc_policy / datasets.collect(mpc=dict(planner="policy"))).

The yardstick is the loop the call fuses, written against the API as it stood before (tests/mpc_policy_reference.py: a PolicyNoise
per control step, plan_policy, the action, step).  Two engines of the same configuration start from the same state and reset key; one
runs the fused call, the other the loop.  The header specifies the call as that loop bit for bit, so EVERY comparison here is exact
(torch.equal): actions, observations, rewards, done codes, every step's best return, best index and effective sample size, the final
state and counters, and compact_done().  Two anchors do not go through plan_policy at all: with one candidate the actions are
rollout_policy's, and rollout() replays the actions into the other outputs.

The last test launches every compiled configuration (tests/kernel_matrix.py:ROWS).  kernel_matrix.ENTRY_POINTS is not extended for it:
that table is pinned at its 16 entries by tests/test_kernel_matrix.py, so this file carries its own table of which rows the call
serves (the 16 four-state rows and the 16 InvertedDoublePendulum rows) and which it refuses (the other 32)."""
import numpy as np
import pytest

import kernel_matrix as KM
import mpc_policy_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 2 ** 64 - 9  # of the noise: seed + t * stride wraps inside the call
NAMES = ("actions", "obs", "reward", "done", "plan_return", "plan_index", "ess")
CART, PEND, IDP = "CartPoleSwingUp", "ReboundInvertedPendulumSwingUp", "BoundaryInvertedDoublePendulumSwingUp"


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


def _pair(name, N, **kw):
    return _engine(name, N, seed=7, **kw), _engine(name, N, seed=7, **kw)


def _state0(eng, seed=11):
    """start rows near the env's reset distribution, the same for both engines"""
    s = np.random.default_rng(seed).uniform(-0.05, 0.05, (eng.n_envs, eng.state_dim))
    if eng.env_name == "CartPoleSwingUp":
        s[:, 2] += np.pi
    if "InvertedPendulumSwingUp" in eng.env_name:
        s[:, 1] += np.pi
    return s


def _policy(eng, hidden, out="clip", seed=21, nan=False):
    from emei_amd.policy import MLPPolicy

    rng = np.random.default_rng(seed + hidden)
    r = lambda *s: (rng.standard_normal(s) * 1.5 / np.sqrt(s[-1])).astype(np.float32)
    n_out = max(eng.act_dim, 1)
    if hidden == 0:
        w = dict(w2=r(n_out, eng.obs_dim), b2=r(n_out))
    else:
        w = dict(w2=r(n_out, hidden), b2=r(n_out), w1=r(hidden, eng.obs_dim), b1=r(hidden))
    if nan:
        w["w2"][0, 0] = np.nan
    return MLPPolicy(out=out, **w)


def _noise_maker(eng, **over):
    """seed -> PolicyNoise of the env's kind: epsilon-greedy on the discrete envs, a Gaussian std on the continuous ones"""
    from emei_amd.policy import PolicyNoise

    kw = over or (dict(epsilon=0.3) if eng.act_dim == 0 else dict(std=0.4))
    return lambda seed: PolicyNoise(seed, **kw)


def _start(engs, state, reset_seed=3):
    for e in engs:
        e.reset(reset_seed)  # the key of the device reset generator, episode counters to 0
        e.set_state(state)


def _snapshot(eng):
    steps, epi = eng.get_counters()
    return {"state": eng.get_state(), "steps": steps, "episode": epi, "compact_done": eng.compact_done()}


def _first_difference(got, want):
    """the first differing quantity in the order that locates a fault: the plan of step 0, then the rest"""
    for key in ("plan_return", "plan_index", "ess", "actions"):
        if key in want and not torch.equal(got[key][0], want[key][0]):
            return f"{key}[0]: {got[key][0].tolist()} != {want[key][0].tolist()}"
    for key in ("actions", "plan_return", "plan_index", "ess", "obs", "reward", "done", "state", "steps", "episode", "compact_done"):
        if key not in want and key not in got:
            continue
        if got[key].shape != want[key].shape or got[key].dtype != want[key].dtype or not torch.equal(got[key], want[key]):
            return f"{key}: {got[key].tolist()} != {want[key].tolist()}"
    return None


def _assert_equal(a, b, what):
    diff = _first_difference(a, b)
    assert diff is None, f"{what}: {diff}"


def _run_both(fused, loop, T, H, K, policy, make_noise, state, seed=SEED, stride=None, start=True, **kw):
    """the fused call on `fused`, the loop on `loop`, from the same state -> (fused results, loop results) as dicts"""
    if start:
        _start((fused, loop), state)
    a = dict(zip(NAMES, fused.mpc_policy(T, H, K, policy, make_noise(seed), seed_stride=stride, diagnostics=True, **kw)))
    b = dict(zip(NAMES, R.mpc_policy_loop(loop, T, H, K, policy, make_noise, seed, stride=stride, **kw)))
    a.update(_snapshot(fused)), b.update(_snapshot(loop))
    return a, b


# N = 3: the block's last wave has no env; N = 5: two blocks.  K: the deterministic policy alone, fewer candidates than lanes, exactly
# one pass, three passes with a ragged last one.  hidden 0: the affine policy.
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("name", [CART, PEND])
def test_shape_sweep_equals_the_loop(name, N):
    fused, loop = _pair(name, N)
    state, mk = _state0(fused), _noise_maker(fused)
    for hidden in (0, 8):
        pol = _policy(fused, hidden)
        for K in (1, 5, 64, 130):
            for H, T, act in ((1, 1, "best"), (3, 7, "mean"), (3, 1, "best"), (1, 7, "mean"), (3, 7, "best")):
                kw = dict(act=act, temperature=0.7 if act == "mean" or K == 64 else None, discount=0.97)
                a, b = _run_both(fused, loop, T, H, K, pol, mk, state, **kw)
                _assert_equal(a, b, f"{name} N={N} hidden={hidden} K={K} H={H} T={T} act={act}")
                assert a["actions"].dtype == (torch.int64 if fused.act_dim == 0 else torch.float32)
                assert a["plan_index"].dtype == torch.int32 and fused.last_kernel() == 24  # EMEI_KERNEL_PEND_MPC_POLICY
    assert bool(torch.isfinite(a["plan_return"]).all()) and bool(((a["plan_index"] >= 0) & (a["plan_index"] < 130)).all())


@pytest.mark.parametrize("name,kw", [
    (CART, dict(precision="f32")), (PEND, dict(precision="f32")), (CART, dict(ode_method="rk4")), (CART, dict(freq_rate=2)),
    ("BoundaryInvertedPendulumBalancing", dict(freq_rate=2))], ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_four_state_kernel_variants_equal_the_loop(name, kw):
    fused, loop = _pair(name, 3, **kw)
    for act in ("best", "mean"):
        a, b = _run_both(fused, loop, 7, 3, 70, _policy(fused, 8), _noise_maker(fused), _state0(fused), act=act, temperature=0.7)
        _assert_equal(a, b, f"{name} {kw} {act}")
    assert fused.last_kernel() == 24


@pytest.mark.parametrize("kw", [dict(), dict(integrator="semi_implicit_euler"), dict(integrator="rk4"), dict(precision="f32"),
                                dict(precision="f32", integrator="rk4")], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "euler")
@pytest.mark.parametrize("name", KM.DP)
def test_double_pendulum_equals_the_loop(name, kw):
    fused, loop = _pair(name, 3, **kw)
    for act in ("best", "mean"):
        a, b = _run_both(fused, loop, 7, 3, 70, _policy(fused, 8), _noise_maker(fused), _state0(fused), act=act, temperature=0.7,
                         auto_reset=True)
        _assert_equal(a, b, f"{name} {kw} {act}")
    assert fused.last_kernel() == 25 and tuple(a["obs"].shape) == (7, 3, 6)  # EMEI_KERNEL_BODY_MPC_POLICY


def _threshold_rows():
    """CartPoleBalancing: envs 0 and 1 leave |x| < 2.4 with their first step whatever the action (x moves by 0.02 * x_dot per step),
    env 2 stays"""
    s = np.zeros((3, 4))
    s[0, :2] = (2.39, 2.0)
    s[1, :2] = (-2.39, -2.0)
    s[2, 2] = 0.01
    return s


@pytest.mark.parametrize("auto_reset", [True, False])
def test_termination_truncation_and_reset_equal_the_loop(auto_reset):
    from emei_amd import _lib as L

    fused, loop = _pair("CartPoleBalancing", 3)
    pol, mk = _policy(fused, 8), _noise_maker(fused)
    a, b = _run_both(fused, loop, 8, 3, 70, pol, mk, _threshold_rows(), act="mean", temperature=0.7, auto_reset=auto_reset)
    _assert_equal(a, b, f"auto_reset={auto_reset}")
    done = a["done"].cpu().numpy()
    assert np.array_equal(done[0, :2], [L.DONE_TERMINAL, L.DONE_TERMINAL])
    assert np.array_equal(a["compact_done"].cpu().numpy(), np.nonzero(done[-1])[0])
    if not auto_reset:
        return
    assert int(a["episode"].max()) > 0 and np.array_equal(a["episode"].cpu().numpy(), (done != 0).sum(0))
    tl_f, tl_l = _pair("CartPoleBalancing", 3, max_episode_steps=3)
    a, b = _run_both(tl_f, tl_l, 8, 3, 70, pol, mk, _threshold_rows(), act="best", auto_reset=True)
    _assert_equal(a, b, "max_episode_steps=3")
    codes = set(a["done"].cpu().numpy().ravel().tolist())
    assert L.DONE_TERMINAL in codes and L.DONE_TRUNCATED in codes and int(a["episode"].max()) > 0


@pytest.mark.parametrize("stride", [None, 1])
def test_chunking(stride):
    H = 3
    one, two = _pair(CART, 3)
    pol, mk, state = _policy(one, 8), _noise_maker(one), _state0(one)
    _start((one, two), state)
    kw = dict(act="mean", temperature=0.7, seed_stride=stride, auto_reset=True, diagnostics=True)
    whole = one.mpc_policy(7, H, 70, pol, mk(SEED), **kw)
    first = two.mpc_policy(3, H, 70, pol, mk(SEED), **kw)
    second = two.mpc_policy(4, H, 70, pol, mk((SEED + 3 * (H if stride is None else stride)) & R.MASK64), **kw)
    a = dict(zip(NAMES, whole))
    b = dict(zip(NAMES, (torch.cat((x, y)) for x, y in zip(first, second))))
    a.update(_snapshot(one)), b.update(_snapshot(two))
    _assert_equal(a, b, f"7 = 3 + 4, stride={stride}")


def test_sharding():
    whole = _engine(CART, 6, seed=7)
    parts = [_engine(CART, 3, seed=7, env_index_offset=off) for off in (0, 3)]
    pol, mk, state = _policy(whole, 8), _noise_maker(whole), _state0(whole)
    _start((whole,), state)
    kw = dict(act="mean", temperature=0.7, auto_reset=True, diagnostics=True)
    a = dict(zip(NAMES, whole.mpc_policy(5, 3, 70, pol, mk(SEED), **kw)))
    a.update(_snapshot(whole))
    outs = []
    for p, rows in zip(parts, (state[:3], state[3:])):
        _start((p,), rows)
        o = dict(zip(NAMES, p.mpc_policy(5, 3, 70, pol, mk(SEED), **kw)))
        o.update(_snapshot(p))
        outs.append(o)
    for key in NAMES:
        assert torch.equal(a[key], torch.cat((outs[0][key], outs[1][key]), dim=1)), key
    for key in ("state", "steps", "episode"):
        assert torch.equal(a[key], torch.cat((outs[0][key], outs[1][key]))), key
    assert torch.equal(a["compact_done"], torch.cat((outs[0]["compact_done"], outs[1]["compact_done"] + 3)))


@pytest.mark.parametrize("auto_reset", [False, True])
def test_anchors_outside_plan_policy(auto_reset):
    """K = 1 is the deterministic policy: rollout_policy's actions; and rollout() replays any call's actions into its other outputs"""
    fused, other = _pair(CART, 5)
    pol, mk, state = _policy(fused, 8), _noise_maker(fused), _state0(fused)
    _start((fused, other), state)
    act, obs, rew, done = fused.mpc_policy(6, 3, 1, pol, mk(SEED), auto_reset=auto_reset)
    want = other.rollout_policy(6, pol, auto_reset=auto_reset)
    for name, x, y in zip(("actions", "obs", "reward", "done"), (act, obs, rew, done), want):
        assert torch.equal(x, y), name
    _start((fused, other), state)
    act, obs, rew, done = fused.mpc_policy(6, 3, 70, pol, mk(SEED), act="mean", temperature=0.7, auto_reset=auto_reset)
    for name, x, y in zip(("obs", "reward", "done"), (obs, rew, done), other.rollout(act, auto_reset=auto_reset)):
        assert torch.equal(x, y), name
    a, b = _snapshot(fused), _snapshot(other)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_noise_and_output_modes_equal_the_loop():
    fused, loop = _pair(PEND, 3)
    state = _state0(fused)
    rng = np.random.default_rng(4)
    ws, bs = (rng.standard_normal((1, 8)) * 0.3).astype(np.float32), np.array([-1.0], np.float32)
    for out, over in (("tanh", dict(std=0.4)), ("clip", dict(log_std_head=(ws, bs), log_std_range=(-3.0, 0.5))),
                      ("tanh", dict(log_std_head=(ws, bs), log_std_range=(-3.0, 0.5))), ("clip", dict(std=[0.25]))):
        a, b = _run_both(fused, loop, 5, 3, 70, _policy(fused, 8, out=out), _noise_maker(fused, **over), state, act="mean", temperature=0.7)
        _assert_equal(a, b, f"out={out} {sorted(over)}")


def test_non_finite_inputs_do_not_fault_and_candidate_zero_takes_no_noise():
    fused, loop = _pair(PEND, 3)
    state, pol = _state0(fused), _policy(fused, 8)
    for std in (float("inf"), float("nan")):
        a, b = _run_both(fused, loop, 3, 3, 70, pol, _noise_maker(fused, std=[std]), state, act="best")
        _assert_equal(a, b, f"std={std}")
    # candidate 0 is unaffected by the std: with K = 1 any std gives the deterministic policy's episode
    _start((fused, loop), state)
    x = fused.mpc_policy(4, 3, 1, pol, _noise_maker(fused, std=[float("nan")])(SEED))
    y = loop.mpc_policy(4, 3, 1, pol, _noise_maker(fused, std=[0.1])(SEED + 5))
    assert all(torch.equal(p, q) for p, q in zip(x, y))
    a, b = _run_both(fused, loop, 3, 3, 70, _policy(fused, 8, nan=True), _noise_maker(fused), state, act="mean", temperature=0.7)
    _assert_equal(a, b, "a NaN weight")
    torch.cuda.synchronize()


SERVED = ("cartpole", "ip_staged", "dp")  # the families emei_mpc_mppi serves: the four-state kernels and the InvertedDoublePendulum


@pytest.mark.parametrize("row", [r for r in KM.ROWS if not r.extra], ids=lambda r: r.id)
def test_every_compiled_configuration(row):
    from emei_amd import _lib as L

    N, T, H, K = 130, 2, 2, 3
    kw = dict(row.kw, seed=5, init_noise=0.05 if row.family != "cartpole" else 0.0)
    fused, loop = _engine(row.env, N, **kw), _engine(row.env, N, **kw)
    pol, mk = _policy(fused, 8), _noise_maker(fused)
    fused.reset(9), loop.reset(9)
    if row.family not in SERVED:
        with pytest.raises(NotImplementedError, match="steps on the body kernels"):
            fused.mpc_policy(T, H, K, pol, mk(SEED))
        return
    a, b = _run_both(fused, loop, T, H, K, pol, mk, None, start=False, act="mean", temperature=0.7, discount=0.97, auto_reset=True)
    _assert_equal(a, b, row.id)
    assert fused.last_kernel() == (L.KERNEL_BODY_MPC_POLICY if row.body else L.KERNEL_PEND_MPC_POLICY)


def test_the_matrix_table_of_this_file():
    rows = [r for r in KM.ROWS if not r.extra]
    served = [r for r in rows if r.family in SERVED]
    assert len(rows) == 64 and len(served) == 32 and sum(r.body for r in served) == 16


def test_refusals_with_a_handle():
    from emei_amd.policy import DeepMLPPolicy, PolicyNoise

    eng = _engine(CART, 3, seed=7)
    pol, mk = _policy(eng, 8), _noise_maker(eng)
    with pytest.raises(AssertionError, match="emei_mpc_policy: call reset"):
        eng.mpc_policy(2, 3, 5, pol, mk(1))
    eng.reset(0)
    with pytest.raises(ValueError, match="discrete"):
        eng.mpc_policy(2, 3, 5, pol, PolicyNoise(1, std=0.1))
    with pytest.raises(ValueError, match="needs a temperature"):
        eng.mpc_policy(2, 3, 5, pol, mk(1), act="mean")
    deep = DeepMLPPolicy(*(torch.zeros(s) for s in ((1, 6), (1,), (6, 5), (6,), (5, 4), (5,))))
    with pytest.raises(NotImplementedError, match="plan_policy"):
        eng.mpc_policy(2, 3, 5, deep, mk(1))
    assert eng.mpc_policy(2, 3, 5, pol, mk(1))[0].shape == (2, 3)  # a valid call succeeds behind the refusals
    noisy = _engine(IDP, 2, obs_noise=1e-3)
    noisy.reset(0)
    with pytest.raises(NotImplementedError, match="emei_mpc_policy: .*observation noise"):
        noisy.mpc_policy(2, 3, 5, _policy(noisy, 8), _noise_maker(noisy)(1))
    clean = _engine(IDP, 2)
    clean.reset(0)
    assert clean.mpc_policy(2, 3, 5, _policy(clean, 8), _noise_maker(clean)(1))[1].shape == (2, 2, 6)
    torch.cuda.synchronize()


def test_hipenv_pass_through_and_collect():
    import emei_amd
    from emei_amd import datasets

    def make():
        return emei_amd.make("CartPoleBalancing-v0", num_envs=4, freq_rate=2)

    env, twin = make(), make()
    pol, mk = _policy(env.engine, 8), _noise_maker(env.engine)
    for e in (env, twin):
        e.reset(seed=3, options={"device_rng": True})
    kw = dict(act="mean", temperature=0.7, auto_reset=True)
    act, obs, rew, term, trunc = env.mpc_policy(12, 3, 20, pol, mk(SEED), **kw)
    a2, o2, r2, d2 = twin.engine.mpc_policy(12, 3, 20, pol, mk(SEED), **kw)
    assert torch.equal(act, a2) and torch.equal(obs, o2) and torch.equal(rew, r2)
    assert term.dtype == torch.bool and torch.equal(term, (d2 & 1).bool()) and torch.equal(trunc, (d2 & 2).bool())
    assert bool(term.any())  # a random policy at freq_rate = 2 drops the pole within twelve steps
    # collect: the zoo schema, the transitions of the direct call under collect's own bookkeeping, structured as the "mppi" path's
    spec = dict(planner="policy", horizon=3, n_candidates=20, policy=pol, noise=mk(SEED), act="mean", temperature=0.7)
    data, info = datasets.collect(make(), 12, mpc=spec, seed=3)
    ref, rinfo = datasets.collect(make(), 12, mpc=dict(horizon=3, n_candidates=20, temperature=0.7), seed=3)
    assert tuple(data) == datasets.DATASET_KEYS == tuple(ref) and set(info) == set(rinfo)
    for key in datasets.DATASET_KEYS:
        assert data[key].shape == ref[key].shape and data[key].dtype == ref[key].dtype, key
    em = lambda x: x.transpose(0, 1).reshape((4 * 12,) + tuple(x.shape[2:]))
    assert torch.equal(data["next_observations"], em(obs)) and torch.equal(data["rewards"], em(rew))
    assert torch.equal(data["actions"], em(act[..., None])) and torch.equal(data["dones"], em((d2 != 0).float()))
    assert torch.equal(data["timeouts"], em(trunc.float())) and info["total_sample_num"] == 48 and info["total_episode_num"] == int((d2 != 0).sum())
    prev_done = torch.zeros_like(d2, dtype=torch.bool)
    prev_done[1:] = d2[:-1] != 0
    keep = ~em(prev_done)
    shifted = torch.empty_like(obs)
    shifted[1:] = obs[:-1]
    keep[::12] = False  # row 0 of every env is reset()'s observation
    assert torch.equal(data["observations"][keep], em(shifted)[keep])
    with pytest.raises(ValueError, match="'mppi', 'cem' or 'policy'"):
        datasets.collect(make(), 2, mpc=dict(planner="ilqr", horizon=3, n_candidates=4))
