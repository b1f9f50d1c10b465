"""GPU parity of the CartPole kernels (through the C ABI) against the golden vectors generated from
the reference and against the CPU oracle.  Tolerance (BASELINE.json north_star): 1e-5 relative on
float32 trajectories (relative down to |ref| = 1e-3, conftest.rel_err), terminal masks bit-exact."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RTOL = 1e-5
ENV = {"swingup": "CartPoleSwingUp", "balancing": "CartPoleBalancing"}


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


@pytest.mark.parametrize("name", ["swingup", "balancing"])
@pytest.mark.parametrize("fr,dt", [(1, 0.02), (4, 0.02), (2, 0.01)])
@pytest.mark.parametrize("precision", ["ref", "f32"])
@pytest.mark.parametrize("adtype", ["uint8", "int64"])
def test_onestep_vs_golden(cartpole_golden, name, fr, dt, precision, adtype):
    g = cartpole_golden
    s0, act = g[f"onestep_{name}_state"], g[f"onestep_{name}_action"]
    tag = f"onestep_{name}_fr{fr}_dt{dt}"
    ok = ~g[tag + "_raised"]
    eng = _engine(ENV[name], len(s0), freq_rate=fr, real_time_scale=dt, precision=precision)
    eng.set_state(s0)
    a = torch.as_tensor(act, device=eng.device).to(getattr(torch, adtype))
    obs, rew, done = eng.step(a)
    obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
    nxt, gr, gt = g[tag + "_next"], g[tag + "_reward"], g[tag + "_terminal"]
    # REF (the default, float64 like the reference) meets the north-star 1e-5 on every row; the float32
    # fast mode is held to 1e-5 on states an episode visits and to 1e-4 on the |theta| ~ 600 rad rows,
    # where float32(theta) itself carries 3e-5 rad
    # The float32 mode's error is the rounding of O(1) float32 intermediates (6e-8 absolute), whatever the size of the
    # result: its assertions are absolute below |ref| = 1 (floor 1.0) and say so; REF is relative down to 1e-3.
    tol, fl = (RTOL, 1e-3) if precision == "ref" else (1e-4, 1.0)
    assert rel_err(obs[ok], nxt[ok], floor=fl) <= tol
    assert rel_err(rew[ok], gr[ok], floor=fl) <= tol
    near = ok & (np.abs(s0[:, 2]) < 15.0) & (np.abs(s0[:, 3]) < 20.0)
    assert rel_err(obs[near], nxt[near], floor=fl) <= RTOL
    # masks: bit-exact wherever the float32/float64 observation is not within tolerance of a threshold
    thr = 5.0 if name == "swingup" else 2.4
    margin = np.abs(np.abs(nxt[:, 0]) - thr) < 1e-4
    if name == "balancing":
        margin |= np.abs(np.abs(nxt[:, 2]) - 12 * 2 * np.pi / 360) < 1e-5
    chk = ok & (~margin if precision == "f32" else np.ones_like(ok))
    assert np.array_equal(done[chk] & 1, gt[chk].astype(np.uint8))
    assert not (done & 2).any()  # no TimeLimit configured -> never truncated (base_control.py:80)
    if precision == "ref":
        st = eng.get_state().cpu().numpy()
        assert rel_err(st[ok], nxt[ok], floor=1e-30) <= 1e-9  # float64 state: ~bitwise


@pytest.mark.parametrize("name", ["swingup", "balancing"])
@pytest.mark.parametrize("fr", [1, 4])
def test_trajectory_ref_precision(cartpole_golden, name, fr):
    """All 1000 open-loop steps (beyond the first terminal, like the reference which never resets)."""
    g = cartpole_golden
    tags = [f"traj_{name}_fr{fr}_seed{s}" for s in range(4)]
    s0 = np.stack([g[t + "_states"][0] for t in tags])
    acts = np.stack([g[t + "_actions"] for t in tags], axis=1)  # [T,4]
    eng = _engine(ENV[name], 4, freq_rate=fr, real_time_scale=0.02, precision="ref")
    eng.set_state(s0)
    obs, rew, done = eng.rollout(torch.as_tensor(acts, device=eng.device).to(torch.uint8))
    obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
    for k, t in enumerate(tags):
        assert rel_err(obs[:, k], g[t + "_states"][1:]) <= RTOL, t
        assert rel_err(rew[:, k], g[t + "_reward"]) <= RTOL, t
        assert np.array_equal(done[:, k] & 1, g[t + "_terminal"].astype(np.uint8)), t


@pytest.mark.parametrize("name", ["swingup", "balancing"])
def test_trajectory_f32_until_first_terminal(cartpole_golden, name):
    """float32 fast mode (NOT the default): the swing-up pendulum is chaotic, so float32 state rounding
    grows by ~1e5 over a 20 s trajectory; the mode is held to 1e-4 over the first 40 steps only.  The
    REF precision above is the one that meets 1e-5 over all 1000 steps."""
    g = cartpole_golden
    for fr in (1, 4):
        for s in range(4):
            t = f"traj_{name}_fr{fr}_seed{s}"
            term = g[t + "_terminal"]
            first = int(np.argmax(term)) + 1 if term.any() else 200
            first = min(first, 40)
            eng = _engine(ENV[name], 1, freq_rate=fr, precision="f32")
            eng.set_state(g[t + "_states"][:1])
            a = torch.as_tensor(g[t + "_actions"][:first, None], device=eng.device).to(torch.int32)
            obs, rew, done = eng.rollout(a)
            assert rel_err(obs.cpu().numpy()[:, 0], g[t + "_states"][1 : first + 1]) <= 1e-4, t


@pytest.mark.parametrize("precision", ["ref", "f32"])
def test_rollout_equals_repeated_step(precision):
    N, T = 1000, 37  # ragged: not a multiple of the wave or block size
    eng_a = _engine("CartPoleSwingUp", N, freq_rate=2, precision=precision, max_episode_steps=20, seed=5)
    eng_b = _engine("CartPoleSwingUp", N, freq_rate=2, precision=precision, max_episode_steps=20, seed=5)
    eng_a.reset(5)
    eng_b.reset(5)
    acts = torch.randint(0, 2, (T, N), device=eng_a.device, dtype=torch.uint8)
    obs, rew, done = eng_a.rollout(acts, auto_reset=True)
    for t in range(T):
        o, r, d = eng_b.step(acts[t], auto_reset=True)
        assert torch.equal(o, obs[t]) and torch.equal(r, rew[t]) and torch.equal(d, done[t])
    assert torch.equal(eng_a.get_state(), eng_b.get_state())
    assert (done & 2).any()  # truncation happened (max_episode_steps=20 < T)


def test_step_before_reset_asserts():
    eng = _engine("CartPoleSwingUp", 8)
    with pytest.raises(AssertionError, match="Call reset before using step method"):
        eng.step(torch.zeros(8, dtype=torch.uint8, device=eng.device))


# ------------------------------------------------------------------------------------------------
def _oracle_autoreset_rollout(variant, s0, acts, seed, offset, max_steps, fr=1, dt=0.02):
    from conftest import oracle_autoreset_rollout

    return oracle_autoreset_rollout(variant, s0, acts, seed, offset + np.arange(acts.shape[1]), max_steps, fr, dt)


@pytest.mark.parametrize("name", ["swingup", "balancing"])
def test_autoreset_rollout_vs_oracle(name):
    """Device-side reset (Philox) + TimeLimit against the oracle, step for step, over several episodes."""
    from oracle import oracle as O

    N, T, seed, off, max_steps = 192, 160, 11, 1000, 50
    eng = _engine(ENV[name], N, precision="ref", max_episode_steps=max_steps, seed=seed, env_index_offset=off)
    eng.reset(seed)
    s0 = eng.get_state().cpu().numpy()
    ref0 = np.stack([O.cartpole_init_f32(name, seed, off + i, 0) for i in range(N)]).astype(np.float64)
    assert np.array_equal(s0, ref0)  # the uniform init is exact arithmetic: bit-identical
    acts = np.random.default_rng(5).integers(2, size=(T, N))
    obs, rew, done = eng.rollout(torch.as_tensor(acts, device=eng.device).to(torch.uint8), auto_reset=True)
    o_obs, o_rew, o_done, o_st = _oracle_autoreset_rollout(name, s0, acts, seed, off, max_steps)
    assert np.array_equal(done.cpu().numpy(), o_done)
    assert (o_done & 2).any() and ((o_done & 1).any() or name == "swingup")
    assert rel_err(obs.cpu().numpy(), o_obs) <= RTOL
    assert rel_err(rew.cpu().numpy(), o_rew) <= RTOL
    assert rel_err(eng.get_state().cpu().numpy(), o_st, floor=1e-30) <= 1e-9


def test_compact_done_sorted_indices():
    N = 1000  # ragged last wave
    eng = _engine("CartPoleBalancing", N, max_episode_steps=0, seed=3)
    eng.reset(3)
    acts = torch.randint(0, 2, (40, N), device=eng.device, dtype=torch.uint8)
    obs, rew, done = eng.rollout(acts)  # no reset: once terminal, mostly stays terminal
    idx = eng.compact_done().cpu().numpy()
    want = np.nonzero(done[-1].cpu().numpy())[0]
    assert np.array_equal(idx, want) and len(want) > 0 and np.all(np.diff(idx) > 0)
    eng.reset(4)
    eng.step(acts[0])
    assert eng.compact_done().numel() == 0  # nobody is done one step after reset


def test_compact_done_beyond_one_pass_of_the_compaction_kernel():
    """above 65 536 envs the compaction kernel's loop runs a second pass: the indices (not only their count) against
    torch.nonzero, with a ragged last wave"""
    N = 65536 + 64 + 3
    eng = _engine("CartPoleBalancing", N, max_episode_steps=0, seed=3)
    eng.reset(3)
    acts = torch.randint(0, 2, (40, N), device=eng.device, dtype=torch.uint8)
    _, _, done = eng.rollout(acts)
    idx = eng.compact_done()
    want = torch.nonzero(done[-1]).flatten().to(torch.int32)
    assert torch.equal(idx, want)
    assert int((want >= 65536).sum()) > 0 and int((want < 65536).sum()) > 0  # done envs in both passes


def test_freeze_unfreeze_restores_state():
    eng = _engine("CartPoleSwingUp", 256, seed=1)
    eng.reset(1)
    acts = torch.randint(0, 2, (8, 256), device=eng.device, dtype=torch.uint8)
    eng.rollout(acts[:4])
    with pytest.raises(AssertionError):
        eng.unfreeze()  # not frozen yet
    eng.freeze()
    snap = eng.get_state().clone()
    a = eng.rollout(acts[4:])
    eng.unfreeze()
    assert torch.equal(eng.get_state(), snap)
    b = eng.rollout(acts[4:])
    assert all(torch.equal(x, y) for x, y in zip(a, b))  # query-then-continue gives the same future


@pytest.mark.parametrize("name", ["swingup", "balancing"])
def test_stateless_batch_functions_vs_golden(cartpole_golden, name):
    """get_batch_reward / get_batch_terminal / get_batch_next_obs on the reference's own float64 rows, EVERY golden row:
    the *_io entry points take float64 observations unnarrowed (cartpole.py:124-129,145-151 compute on float64 arrays),
    so no row needs a mask: rewards 1e-5, terminal bits equal — including |theta| ~ 600 rad, x within 1e-7 of a
    threshold, NaN and inf rows."""
    from emei_amd import engine as E

    g = cartpole_golden
    obs = g[f"batch_{name}_obs"]
    o64 = torch.as_tensor(obs, dtype=torch.float64, device="cuda")
    rew, term = E.batch_reward(ENV[name], o64), E.batch_terminal(ENV[name], o64)
    assert rew.dtype == torch.float64
    assert rel_err(rew.cpu().numpy(), g[f"batch_{name}_reward"][:, 0]) <= RTOL
    assert np.array_equal(term.cpu().numpy(), g[f"batch_{name}_terminal"][:, 0])
    # float32 rows (the round-1 entry points): exact for the float32 argument they are given
    from oracle import oracle as O

    o32 = torch.as_tensor(obs, dtype=torch.float32, device="cuda")
    a32 = o32.double().cpu().numpy()
    r32 = E.batch_reward(ENV[name], o32)
    assert r32.dtype == torch.float32 and rel_err(r32.cpu().numpy(), O.cartpole_reward(name, a32)) <= 2e-7
    assert np.array_equal(E.batch_terminal(ENV[name], o32).cpu().numpy(), O.cartpole_terminal(name, a32))
    # get_batch_next_obs: one step from float64 observations == golden one-step next state, every row the reference computed
    s0, act = g[f"onestep_{name}_state"], g[f"onestep_{name}_action"]
    ok = ~g[f"onestep_{name}_fr4_dt0.02_raised"]
    nxt = E.batch_next_obs(ENV[name], torch.as_tensor(s0, dtype=torch.float64, device="cuda"),
                           torch.as_tensor(act, device="cuda"), 0.02, 4, "ref")
    assert nxt.dtype == torch.float64
    assert rel_err(nxt.cpu().numpy()[ok], g[f"onestep_{name}_fr4_dt0.02_next"][ok]) <= RTOL


def test_bad_arguments_raise():
    eng = _engine("CartPoleSwingUp", 64)
    eng.reset(0)
    with pytest.raises(ValueError):
        eng.step(torch.zeros(63, dtype=torch.uint8, device=eng.device))  # wrong shape
    with pytest.raises(ValueError):
        eng.step(torch.zeros(64, dtype=torch.float32, device=eng.device))  # float action on a discrete env
    with pytest.raises(ValueError):
        eng.set_state(np.zeros((64, 3)))
    with pytest.raises(ValueError):
        _engine("CartPoleSwingUp", 0)
    with pytest.raises(ValueError):
        _engine("CartPoleSwingUp", 8, freq_rate=0)
    with pytest.raises(ValueError):
        _engine("NoSuchEnv", 8)


# ------------------------------------------------------------------------------------------------
# BASELINE full size (65 536 envs): size-independent properties
def test_full_size_properties():
    N, T = 65536, 96
    acts = torch.randint(0, 2, (T, N), device="cuda", dtype=torch.uint8)
    a = _engine("CartPoleSwingUp", N, max_episode_steps=1000, seed=9)
    a.reset(9)
    obs, rew, done = a.rollout(acts, auto_reset=True)
    # (1) chunking invariance: 96 fused steps == 3 launches of 32 (staged path) == one of 96
    b = _engine("CartPoleSwingUp", N, max_episode_steps=1000, seed=9)
    b.reset(9)
    parts = [b.rollout(acts[k : k + 32].contiguous(), auto_reset=True) for k in range(0, T, 32)]
    assert torch.equal(torch.cat([p[0] for p in parts]), obs) and torch.equal(torch.cat([p[2] for p in parts]), done)
    assert torch.equal(a.get_state(), b.get_state())
    # (2) sharding invariance: two half-size shards with the global env offset reproduce the whole
    h = N // 2
    halves = []
    for r in range(2):
        e = _engine("CartPoleSwingUp", h, max_episode_steps=1000, seed=9, env_index_offset=r * h)
        e.reset(9)
        halves.append(e.rollout(acts[:, r * h : (r + 1) * h].contiguous(), auto_reset=True))
    assert torch.equal(torch.cat([halves[0][0], halves[1][0]], dim=1), obs)
    assert torch.equal(torch.cat([halves[0][2], halves[1][2]], dim=1), done)
    # (3) compaction count == number of done flags of the last step; rewards in [0,1]; obs finite
    assert a.compact_done().numel() == int((done[-1] != 0).sum())
    assert float(rew.min()) >= 0.0 and float(rew.max()) <= 1.0 and bool(torch.isfinite(obs).all())
    # (4) terminal flag <=> |x| >= 5 on the float32 observation away from the threshold
    x = obs[..., 0].abs()
    clear = (x - 5.0).abs() > 1e-4
    assert torch.equal(((done & 1) != 0)[clear], (x >= 5.0)[clear])


def test_step_launches_are_graph_capturable():
    """The ABI launch functions neither allocate nor synchronise: K per-step launches captured into one
    hipGraph replay to exactly the fused rollout's results, and keep advancing the state on each replay."""
    N, K = 4096, 24
    a = _engine("CartPoleSwingUp", N, max_episode_steps=10, seed=6)
    b = _engine("CartPoleSwingUp", N, max_episode_steps=10, seed=6)
    a.reset(6)
    b.reset(6)
    acts = torch.randint(0, 2, (K, N), device=a.device, dtype=torch.uint8)
    graph, obs, rew, done = a.capture_step_graph(acts, auto_reset=True)  # capture does not execute the launches
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        r_obs, r_rew, r_done = b.rollout(acts, auto_reset=True)
        assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(a.get_state(), b.get_state())


@pytest.mark.parametrize("n", [64, 128, 192, 320])
def test_partial_last_block_with_the_tile_barrier(n):
    """The staged SwingUp kernel's waves meet at a workgroup barrier once per tile (Env::kTileBarrier); a shard of 1, 2, 3 or 5 waves leaves
    the last 256-thread block partly empty — its absent waves return before the first barrier and must not be waited for.  Rollout ==
    repeated step, bit for bit, and the staged kernel is what ran."""
    from emei_amd import _lib
    from emei_amd.engine import Engine

    T = 48
    a, b = Engine("CartPoleSwingUp", n, max_episode_steps=20, seed=2), Engine("CartPoleSwingUp", n, max_episode_steps=20, seed=2)
    a.reset(2), b.reset(2)
    acts = torch.randint(0, 2, (T, n), device=a.device, dtype=torch.uint8)
    obs, rew, done = a.rollout(acts, auto_reset=True)
    assert a.last_kernel() == _lib.KERNEL_PEND_STAGED_FREQ1
    for t in range(T):
        o, r, d = b.step(acts[t], auto_reset=True)
        assert torch.equal(o, obs[t]) and torch.equal(r, rew[t]) and torch.equal(d, done[t])
    assert torch.equal(a.get_state(), b.get_state())
