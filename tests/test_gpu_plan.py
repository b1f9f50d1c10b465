"""emei_evaluate_sequences on the GPU (Engine.evaluate_sequences / HipEnv.evaluate_action_sequences).

The oracle is the composition the call replaces: a handle of N * K envs holding the start states tiled K times runs
emei_rollout with the same actions, and NumPy recomputes the contract from its float32 rewards, terminal bits and observations
(ret = sum_{t < L} discount^t * r_t in float64 step order, L = first terminal step + 1 or H, final_obs = the observation of step
L - 1).  The fused call must give the same bits.  The contract itself is held to the CPU oracle in
tests/test_gpu_plan_oracle.py; the edges of it at the end of this file (action dtypes, terminal steps around the action
prefetch chunk, configured handles, odd start rows, three-block cheetah lanes) mostly use the composition too."""
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


# ------------------------------------------------------------------------------------------------ contract edges
import plan_reference as P  # noqa: E402  (host-made inputs shared with the oracle tests)


def _plan(eng, acts, gamma, **kw):
    return tuple(x.cpu().numpy() for x in eng.evaluate_sequences(acts, discount=gamma, final_obs=True, **kw))


@pytest.mark.parametrize("H", [7, 8, 9, 17])
@pytest.mark.parametrize("name", ["CartPoleSwingUp", "CartPoleBalancing"])
def test_integer_action_dtypes_agree(name, H):
    """pend_plan_kernel<Env, uint8_t / int32_t / int64_t> are three instantiations whose 8-step action prefetch strides 1, 4 and
    8 bytes: the same sequences in each dtype, horizons around the prefetch chunk, give the same bits and those of the rollout
    composition."""
    N, K, gamma = 37, 7, 0.97
    s0, a8 = P.cartpole_inputs(name, N, K, H, seed=40 + H, spread=0.12)
    eng = _engine(name, N)
    eng.set_state(s0)
    dev = torch.as_tensor(a8, device=eng.device)
    outs = {dt: eng.evaluate_sequences(dev.to(dt), discount=gamma, final_obs=True) for dt in (torch.uint8, torch.int32, torch.int64)}
    for dt in (torch.int32, torch.int64):
        for x, y in zip(outs[dt], outs[torch.uint8]):
            assert torch.equal(x, y), dt
    e_ret, e_L, e_fo = _compose(name, s0, dev, gamma)
    ret, L, fo = (x.cpu().numpy() for x in outs[torch.int32])
    assert np.array_equal(L, e_L) and np.array_equal(ret, e_ret) and np.array_equal(fo, e_fo)
    if name == "CartPoleBalancing" and H == 17:
        assert (e_L < H).any() and (e_L == H).any()


def _edge_lengths(H):
    return {v for v in (7, 8, 9, H - 1, H) if v <= H}


@pytest.mark.parametrize("H", [8, 9, 16, 17])
@pytest.mark.parametrize("name,spread", [("CartPoleBalancing", 0.12), ("ReboundInvertedDoublePendulumBalancing", 0.04)])
def test_terminal_steps_at_the_prefetch_chunk_edges(name, spread, H):
    """Terminal steps on both sides of the 8-step action chunk of pend_plan_kernel and at the end of the horizon, and the same
    steps in body_plan_kernel (whose lanes store their results at their last counted step): start rows spread so that the
    EXPECTED lengths — the rollout composition's — include 7, 8, 9, H - 1 and H."""
    N, K, gamma = 37, 7, 0.95
    build = P.cartpole_inputs if name.startswith("CartPole") else P.pendulum_inputs
    s0, acts = build(name, N, K, 17, seed=2, spread=spread)
    eng = _engine(name, N)
    eng.set_state(s0)
    dev = torch.as_tensor(acts[:H], device=eng.device).contiguous()
    e_ret, e_L, e_fo = _compose(name, s0, dev, gamma)
    assert _edge_lengths(H) <= set(e_L.ravel().tolist()), sorted(set(e_L.ravel().tolist()))
    ret, L, fo = _plan(eng, dev, gamma)
    assert np.array_equal(L, e_L) and np.array_equal(ret, e_ret) and np.array_equal(fo, e_fo)
    assert eng.solver_cap_hits() == 0


@pytest.mark.parametrize("name,kw,noise", [
    ("HopperRunning", dict(freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"], integrator="rk4"), True),
    # an InvertedPendulum with observation noise steps as a body (ipend_model.h), a plain euler one on the staged 4-state kernel,
    # and those two agree to 1e-6, not bit for bit (test_gpu_integrators.py:71): rk4 keeps both handles on the same kernel
    ("ReboundInvertedPendulumBalancing", dict(integrator="rk4"), True),
    ("CartPoleBalancing", dict(), False),  # classic control has no observation noise: TimeLimit and auto-reset only
])
def test_configured_handle_equals_plain_handle(name, kw, noise):
    """emei_hip.h: "No observation noise; TimeLimit counters, truncation and auto-reset are not consulted".  A handle configured
    with observation noise, reset noise, a TimeLimit shorter than the horizon, whose counters an auto-reset rollout has advanced
    past several truncations, gives the bits of a plain handle holding the same state."""
    N, K, H, mes, gamma = 37, 7, 16, 5, 0.95
    fam = P.FAMILY[name][0]
    s0, acts = P.BUILDERS[fam](name, N, K, H, seed=23)
    cfg = dict(kw, max_episode_steps=mes, seed=6)
    if noise:
        cfg.update(obs_noise=0.05, init_noise=0.01)
    a, b = _engine(name, N, **cfg), _engine(name, N, **kw)
    a.reset(seed=6)
    _, _, done = a.rollout(torch.as_tensor(acts[:, :, 0], device=a.device).contiguous(), auto_reset=True)
    assert bool((done & 2).any())  # truncations happened: the TimeLimit is live on this handle
    a.set_state(s0, reset_counters=False)
    assert int(a.get_counters()[0].max()) > 0 and int(a.get_counters()[1].max()) > 0
    b.set_state(s0)
    dev = torch.as_tensor(acts, device=a.device)
    got, want = a.evaluate_sequences(dev, gamma, final_obs=True), b.evaluate_sequences(dev, gamma, final_obs=True)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert int(want[1].max()) > mes
    # ... and from start_state rows, with the handle's own state elsewhere
    a.reset(seed=7)
    given = a.evaluate_sequences(dev, gamma, start_state=torch.as_tensor(s0, device=a.device), final_obs=True)
    for x, y in zip(given, want):
        assert torch.equal(x, y)


def _odd_rows(name, rng, N):
    """ordinary rows with NaN, +-inf, beyond-threshold and on-threshold rows at scattered places of the first wave(s)"""
    fam, variant = P.FAMILY[name]
    s0, _ = P.BUILDERS[fam](name, N, 1, 1, seed=int(rng.integers(1 << 30)))
    ix, ith = (0, 2) if fam == "cartpole" else (0, 1)  # (x, theta) in the state row
    # cartpole.py: Balancing ends at |x| >= 2.4 or |theta| >= 12 degrees, SwingUp at |x| >= 5 (its theta rows: large angles);
    # inverted_pendulum.py: the rail at |x| = 2 and cos(theta) = 0.9
    x_thr, th_thr = {"balancing": (2.4, 12 * 2 * np.pi / 360), "swingup": (5.0, 4 * np.pi)}[variant] if fam == "cartpole" \
        else (2.0, float(np.arccos(0.9)))
    odd = {}
    for n, (col, val) in enumerate([(ix, np.nan), (ith, np.nan), (3, np.nan), (ix, np.inf), (ix, -np.inf), (ith, np.inf), (3, -np.inf),
                                    (ix, 1.5 * x_thr), (ix, -1.5 * x_thr), (ith, 2 * th_thr), (ith, -2 * th_thr), (ix, x_thr),
                                    (ix, -x_thr), (ith, th_thr), (ith, -th_thr)]):
        odd[2 + 4 * n] = (col, val)  # rows 2, 6, ..., 58: K = 3 candidates each, ordinary rows between them in the same wave
    rows = s0.copy()
    for r, (col, val) in odd.items():
        rows[r, col] = val
    return s0, rows, np.array(sorted(odd))


@pytest.mark.parametrize("name", ["CartPoleBalancing", "CartPoleSwingUp", "BoundaryInvertedPendulumBalancing"])
def test_odd_start_rows(name):
    """start_state rows that are NaN, +-inf, already beyond a terminal threshold or exactly on it, mixed with ordinary rows inside
    one wave: every candidate equals the rollout composition (NaN where it has NaN), and the ordinary rows' candidates have the
    bits of a launch without the odd neighbours."""
    N, K, H, gamma = 70, 3, 12, 0.95
    rng = np.random.default_rng(5)
    plain, rows, odd = _odd_rows(name, rng, N)
    eng = _engine(name, N)
    eng.reset(seed=1)  # the handle's own state is not what is scored
    acts = _actions(eng, H, N, K, seed=4)
    ret, L, fo = _plan(eng, acts, gamma, start_state=torch.as_tensor(rows, device=eng.device))
    with np.errstate(all="ignore"):
        e_ret, e_L, e_fo = _compose(name, rows, acts, gamma)
    assert np.array_equal(L, e_L)
    assert np.array_equal(ret, e_ret, equal_nan=True) and np.array_equal(fo, e_fo, equal_nan=True)
    assert np.isnan(fo[odd[:3]]).any(axis=(1, 2)).all()  # the NaN rows did reach the kernel
    ret0, L0, fo0 = _plan(eng, acts, gamma, start_state=torch.as_tensor(plain, device=eng.device))
    keep = np.setdiff1d(np.arange(N), odd)
    assert np.array_equal(ret[keep], ret0[keep]) and np.array_equal(L[keep], L0[keep]) and np.array_equal(fo[keep], fo0[keep])
    assert np.isfinite(ret0).all()


def test_three_block_cheetah_lanes_vs_oracle():
    """Cheetah lanes with exactly three constraint blocks (cheetah_model.h: `donor`) in a plan launch: states drawn as
    test_gpu_cheetah.py:test_lanes_with_three_row_blocks_vs_oracle draws them, K = 3 candidates each over H = 2 env-steps, against
    the oracle and the contract with the bounds of test_gpu_plan_oracle.py.  The call returns no float64 state to hold to 1e-9:
    ret is a float64 sum of float32 rewards."""
    from oracle import oracle as O

    rng = np.random.default_rng(31)
    q = rng.normal(0, 0.15, (30000, 9))
    q[:, 1] = rng.uniform(-0.45, 0.1, len(q))  # low: several points on the floor
    q[:, 2] = rng.normal(0, 0.4, len(q))
    q[: len(q) // 4, 3:] = rng.uniform(-1.3, 1.3, (len(q) // 4, 6))
    pool = np.concatenate([q, rng.normal(0, 1.5, q.shape)], axis=1)
    nb = np.array([bin(int(m)).count("1") for m in O.planar_row_mask("cheetah", pool)])
    pick = np.concatenate([np.nonzero(nb == 3)[0][:300], np.nonzero(nb >= 4)[0][:80], np.nonzero(nb <= 2)[0][:263]])
    assert (nb[pick] == 3).sum() == 300 and (nb[pick] >= 4).sum() == 80
    s0 = pool[rng.permutation(pick)]
    N, K, H, gamma = len(s0), 3, 2, 0.97
    kw = dict(freq_rate=2, real_time_scale=0.002)
    acts = rng.uniform(-1.2, 1.2, (H, N, K, 6)).astype(np.float32)
    obs, rew, term = P.oracle_steps("HalfCheetahRunning", kw, np.repeat(s0, K, axis=0), acts.reshape(H, N * K, 6))
    w_ret, w_L, w_fo = P.contract(obs, rew, term, gamma)
    eng = _engine("HalfCheetahRunning", N, **kw)
    eng.set_state(s0)
    ret, L, fo = _plan(eng, torch.as_tensor(acts, device=eng.device), gamma)
    assert np.array_equal(L.ravel(), w_L) and (w_L == H).all()
    ratio = np.abs(ret.ravel() - w_ret) / P.ret_bound(rew, w_L, gamma, P.TOL_R["cheetah"])
    assert ratio.max() <= 1.0, ratio.max()
    assert rel_err(fo.reshape(N * K, -1), w_fo) <= P.TOL_OBS
    assert eng.solver_cap_hits() == 0
