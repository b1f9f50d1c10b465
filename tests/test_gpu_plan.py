"""emei_evaluate_sequences on the GPU (Engine.evaluate_sequences / HipEnv.evaluate_action_sequences).

The oracle is the composition the call replaces: a handle of N * K envs holding the start states tiled K times runs
emei_rollout with the same actions, and NumPy recomputes the contract from its float32 rewards, terminal bits and observations
(ret = sum_{t < L} discount^t * r_t in float64 step order, L = first terminal step + 1 or H, final_obs = the observation of step
L - 1).  The fused call must give the same bits."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MUJOCO = {"dt": 0.002, "fr": 4}  # half_cheetah.py:12, hopper.py:20


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


def _actions(eng, H, N, K, seed):
    g = torch.Generator(device=eng.device).manual_seed(seed)
    if eng.act_dim == 0:
        return torch.randint(0, 2, (H, N, K), generator=g, device=eng.device, dtype=torch.uint8)
    return torch.rand((H, N, K, eng.act_dim), generator=g, device=eng.device) * 2 - 1


def _expected(obs, rew, done, gamma):
    """the contract, from a rollout's outputs [H, M(, obs_dim)]"""
    H, M = rew.shape
    term = (done & 1).astype(bool)
    L = np.where(term.any(0), term.argmax(0) + 1, H).astype(np.int32)
    ret, g = np.zeros(M), 1.0
    for t in range(H):
        ret = np.where(t < L, ret + g * rew[t].astype(np.float64), ret)
        g = g * gamma
    return ret, L, obs[L - 1, np.arange(M)]


def _compose(name, s0, acts, gamma, **kw):
    """rollout of N * K envs from the tiled start states -> the contract's (ret, len, final_obs), [N, K] shaped"""
    H, N, K = acts.shape[:3]
    big = _engine(name, N * K, **kw)
    big.set_state(np.repeat(s0, K, axis=0))
    obs, rew, done = big.rollout(acts.reshape((H, N * K) + tuple(acts.shape[3:])).contiguous())
    ret, L, fo = _expected(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), gamma)
    big.close()
    return ret.reshape(N, K), L.reshape(N, K), fo.reshape(N, K, -1)


# (env, engine kwargs, N, K, H, discount): all 12 ids; both precisions; CartPole's rk4; the three MuJoCo integrators on the
# cheetah and the InvertedPendulum's body path; freq_rate 1 and 2 (4 on the MuJoCo bodies); discount 1 and 0.99; N not a
# multiple of 64, N * K just above a wave (65) and a block (257), H = 1, K = 1
CASES = [
    ("CartPoleSwingUp", dict(precision="ref"), 5, 13, 60, 1.0),
    ("CartPoleSwingUp", dict(precision="f32", freq_rate=2), 100, 3, 40, 0.99),
    ("CartPoleSwingUp", dict(precision="ref", ode_method="rk4"), 257, 1, 30, 0.99),
    ("CartPoleSwingUp", dict(precision="f32", ode_method="rk4", freq_rate=2), 1, 257, 25, 1.0),
    ("CartPoleSwingUp", dict(precision="ref"), 70, 4, 1, 0.99),
    ("CartPoleBalancing", dict(precision="ref"), 64, 8, 120, 0.99),
    ("CartPoleBalancing", dict(precision="f32", freq_rate=2), 33, 5, 80, 1.0),
    ("ReboundInvertedPendulumBalancing", dict(precision="ref"), 40, 6, 50, 0.99),
    ("ReboundInvertedPendulumBalancing", dict(precision="f32"), 40, 6, 50, 1.0),
    ("BoundaryInvertedPendulumBalancing", dict(precision="ref", freq_rate=2), 21, 7, 40, 1.0),
    ("ReboundInvertedPendulumSwingUp", dict(precision="ref", integrator="rk4"), 20, 5, 30, 0.99),
    ("BoundaryInvertedPendulumSwingUp", dict(precision="f32", integrator="semi_implicit_euler"), 13, 5, 30, 1.0),
    ("ReboundInvertedDoublePendulumBalancing", dict(precision="ref"), 16, 8, 40, 0.99),
    ("BoundaryInvertedDoublePendulumBalancing", dict(precision="f32", freq_rate=2), 9, 8, 30, 1.0),
    ("ReboundInvertedDoublePendulumSwingUp", dict(precision="ref", integrator="rk4"), 10, 7, 20, 1.0),
    ("BoundaryInvertedDoublePendulumSwingUp", dict(precision="ref"), 65, 1, 25, 0.99),
    ("HalfCheetahRunning", dict(precision="ref", freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"]), 5, 16, 12, 0.99),
    ("HalfCheetahRunning", dict(precision="f32", freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"],
                                integrator="semi_implicit_euler"), 4, 17, 10, 1.0),
    ("HalfCheetahRunning", dict(precision="ref", freq_rate=2, real_time_scale=MUJOCO["dt"], integrator="rk4"), 3, 22, 6, 1.0),
    ("HopperRunning", dict(precision="ref", freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"], integrator="rk4"), 6, 11, 25, 0.99),
    ("HopperRunning", dict(precision="f32", freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"]), 7, 10, 25, 1.0),
]


@pytest.mark.parametrize("name,kw,N,K,H,gamma", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_equals_the_rollout_composition(name, kw, N, K, H, gamma):
    eng = _engine(name, N, **kw)
    eng.reset(seed=11 + N)
    s0 = eng.get_state().cpu().numpy()
    acts = _actions(eng, H, N, K, seed=N * 7 + K)
    ret, L, fo = eng.evaluate_sequences(acts, discount=gamma, final_obs=True)
    ret, L, fo = ret.cpu().numpy(), L.cpu().numpy(), fo.cpu().numpy()
    e_ret, e_L, e_fo = _compose(name, s0, acts, gamma, **kw)
    assert ret.shape == (N, K) and L.shape == (N, K) and L.dtype == np.int32 and fo.shape == (N, K, eng.obs_dim)
    assert np.array_equal(L, e_L)
    if name == "HalfCheetahRunning":
        # a cheetah lane with three constraint blocks borrows an LDS slot from a wave-mate, so which solver it runs
        # depends on the wave's other lanes.  The candidates sit on the same waves as the composition's envs, but the bound the
        # project states for that lending across launch shapes is the cheetah's cross-path one, not bit equality
        assert rel_err(ret, e_ret) <= 1e-9
        assert rel_err(fo, e_fo) <= 1e-9
    else:
        assert np.array_equal(ret, e_ret), np.abs(ret - e_ret).max()
        assert np.array_equal(fo, e_fo, equal_nan=True)
    assert eng.solver_cap_hits() == 0


def test_cartpole_balancing_every_wave_ends_early():
    """Random sequences fail the balancing task within a few dozen steps: every wave leaves its loop early (ballot), and the
    lengths and returns are still those of the full-length composition."""
    N, K, H = 128, 64, 400
    eng = _engine("CartPoleBalancing", N)
    eng.reset(seed=3)
    s0 = eng.get_state().cpu().numpy()
    acts = _actions(eng, H, N, K, seed=5)
    ret, L = eng.evaluate_sequences(acts, discount=0.99)
    ret, L = ret.cpu().numpy(), L.cpu().numpy()
    assert L.max() < H
    e_ret, e_L, _ = _compose("CartPoleBalancing", s0, acts, 0.99)
    assert np.array_equal(L, e_L) and np.array_equal(ret, e_ret)


def test_reference_trajectories(cartpole_golden):
    """Tied to the reference through the golden file: three 1000-step swing-up trajectories, summed up to the first terminal."""
    g = cartpole_golden
    tags = [f"traj_swingup_fr1_seed{s}" for s in range(3)]
    s0 = np.stack([g[t + "_states"][0] for t in tags])
    acts = np.stack([g[t + "_actions"] for t in tags], axis=1)[:, :, None]  # [1000, 3, 1]
    eng = _engine("CartPoleSwingUp", 3, freq_rate=1, real_time_scale=0.02, precision="ref")
    eng.set_state(s0)
    ret, L = eng.evaluate_sequences(torch.as_tensor(acts, device=eng.device).to(torch.uint8))
    ret, L = ret.cpu().numpy()[:, 0], L.cpu().numpy()[:, 0]
    for k, t in enumerate(tags):
        term = g[t + "_terminal"].astype(bool)
        want_L = int(np.argmax(term)) + 1 if term.any() else len(term)
        assert L[k] == want_L, t
        assert rel_err(ret[k], g[t + "_reward"][:want_L].astype(np.float64).sum()) <= 1e-5, t


@pytest.mark.parametrize("name", ["swingup", "balancing"])
@pytest.mark.parametrize("fr,dt", [(1, 0.02), (4, 0.02), (2, 0.01)])
def test_reference_one_step_rows(cartpole_golden, name, fr, dt):
    g = cartpole_golden
    s0, act = g[f"onestep_{name}_state"], g[f"onestep_{name}_action"]
    tag = f"onestep_{name}_fr{fr}_dt{dt}"
    ok = ~g[tag + "_raised"]
    eng = _engine({"swingup": "CartPoleSwingUp", "balancing": "CartPoleBalancing"}[name], len(s0), freq_rate=fr,
                  real_time_scale=dt, precision="ref")
    eng.set_state(s0)
    a = torch.as_tensor(np.asarray(act)[None, :, None], device=eng.device).to(torch.int64)
    ret, L = eng.evaluate_sequences(a)
    assert (L.cpu().numpy() == 1).all()
    assert rel_err(ret.cpu().numpy()[ok, 0], g[tag + "_reward"][ok]) <= 1e-5


@pytest.mark.parametrize("name,kw", [
    ("CartPoleSwingUp", dict(max_episode_steps=9)),
    ("HopperRunning", dict(max_episode_steps=6, freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"])),
])
def test_handle_untouched(name, kw):
    """state, counters, a following auto-reset rollout and a freeze / unfreeze round trip: the same bits with and without
    an intervening call"""
    N = 96
    a, b = _engine(name, N, seed=4, **kw), _engine(name, N, seed=4, **kw)
    step_acts = _actions(a, 20, N, 1, seed=9)[:, :, 0].contiguous()
    for e in (a, b):
        e.reset(seed=4)
        e.rollout(step_acts[:7], auto_reset=True)
        e.freeze()
        e.rollout(step_acts[7:12], auto_reset=True)
    a.evaluate_sequences(_actions(a, 15, N, 3, seed=2), discount=0.9, final_obs=True)
    assert torch.equal(a.get_state(), b.get_state())
    for x, y in zip(a.get_counters(), b.get_counters()):
        assert torch.equal(x, y)
    outs = [e.rollout(step_acts, auto_reset=True) for e in (a, b)]
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    for e in (a, b):
        e.unfreeze()
    assert torch.equal(a.get_state(), b.get_state())
    outs = [e.rollout(step_acts, auto_reset=True) for e in (a, b)]
    for x, y in zip(*outs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name,kw", [
    ("CartPoleSwingUp", dict(precision="f32")),
    ("ReboundInvertedDoublePendulumSwingUp", dict()),
    ("HopperRunning", dict(freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"], integrator="euler")),
])
def test_start_state_argument_equals_set_state(name, kw):
    N, K, H = 50, 6, 20
    eng = _engine(name, N, **kw)
    eng.reset(seed=1)
    g = torch.Generator(device=eng.device).manual_seed(2)
    rows = eng.get_state() + 0.05 * torch.randn((N, eng.state_dim), generator=g, device=eng.device, dtype=torch.float64)
    acts = _actions(eng, H, N, K, seed=3)
    given = eng.evaluate_sequences(acts, 0.97, start_state=rows, final_obs=True)
    assert not torch.equal(eng.get_state(), rows)
    eng.set_state(rows)
    current = eng.evaluate_sequences(acts, 0.97, final_obs=True)
    for x, y in zip(given, current):
        assert torch.equal(x, y)


def test_env_surface_numpy_and_tensor():
    import emei_amd

    env = emei_amd.make("CartPoleSwingUp-v0")
    env.reset(seed=0)
    acts = np.random.default_rng(0).integers(0, 2, size=(30, 1, 8))
    ret, L = env.evaluate_action_sequences(acts, discount=0.99)
    assert isinstance(ret, np.ndarray) and ret.shape == (1, 8) and ret.dtype == np.float64 and L.dtype == np.int32
    ret_t, L_t, fo = env.evaluate_action_sequences(torch.as_tensor(acts, device=env.engine.device), 0.99, final_obs=True)
    assert torch.equal(ret_t.cpu(), torch.as_tensor(ret)) and torch.equal(L_t.cpu(), torch.as_tensor(L))
    assert fo.shape == (1, 8, 4)
    fresh = emei_amd.make("CartPoleSwingUp-v0")
    with pytest.raises(AssertionError):
        fresh.evaluate_action_sequences(acts)


def test_argument_checks_on_a_handle():
    eng = _engine("HopperRunning", 4)
    eng.reset(seed=0)
    good = _actions(eng, 3, 4, 2, seed=0)
    with pytest.raises(ValueError):
        eng.evaluate_sequences(good[:, :3])  # N mismatch
    with pytest.raises(ValueError):
        eng.evaluate_sequences(good.to(torch.float64))  # dtype
    with pytest.raises(ValueError):
        eng.evaluate_sequences(good, discount=0.0)
    with pytest.raises(ValueError):
        eng.evaluate_sequences(good, start_state=torch.zeros(4, eng.state_dim, device=eng.device))  # float32 rows


def test_capture_replays_the_same_result():
    N, K, H = 256, 16, 50
    eng = _engine("CartPoleSwingUp", N)
    eng.reset(seed=8)
    acts = _actions(eng, H, N, K, seed=1)
    want = eng.evaluate_sequences(acts, 0.99, final_obs=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = eng.evaluate_sequences(acts, 0.99, final_obs=True)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
