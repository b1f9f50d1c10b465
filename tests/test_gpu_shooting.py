"""emei_sample_candidates / emei_plan_shooting on the GPU (Engine.sample_candidates / Engine.plan_shooting /
HipEnv.plan_random_shooting).

Two yardsticks.  The candidates are held to the NumPy restatement of their specification (tests/shooting_reference.py).  The
planner is held to its definition: for the candidates emei_sample_candidates writes out, emei_evaluate_sequences' returns
(whose own tests tie them to the rollout and to the CPU oracle) arg-maxed with the planner's order."""
import numpy as np
import pytest

import shooting_reference as S
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MUJOCO = {"dt": 0.002, "fr": 4}  # half_cheetah.py:12, hopper.py:20
RANGE = {"ReboundInvertedPendulumBalancing": (-3.0, 3.0), "HopperRunning": (-1.0, 1.0), "HalfCheetahRunning": (-1.0, 1.0)}
OFFSET = (1 << 32) + 7  # env_index_offset: the global env index reaches the second counter word


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


def _globals(N, offset):
    return np.arange(N, dtype=np.uint64) + np.uint64(offset)


# ------------------------------------------------------------------------------------------------ a. the candidates
# H = 1, 4, 5, 9: one word, a whole Philox block, one past it, one past the 8-step prefetch chunk; N * K = 65 and 257
SHAPES = [(5, 13), (257, 1), (1, 257)]


@pytest.mark.parametrize("H", [1, 4, 5, 9])
@pytest.mark.parametrize("N,K", SHAPES)
def test_discrete_candidates_equal_the_spec(N, K, H):
    eng = _engine("CartPoleSwingUp", N, env_index_offset=OFFSET)
    g = _globals(N, OFFSET)
    want = S.discrete(0xC0FFEE + H, g, K, H)
    assert np.array_equal(want, S.discrete_top_bit(0xC0FFEE + H, g, K, H))
    prob = np.random.default_rng(H).uniform(0, 1, (H, N)).astype(np.float32)
    prob[0, 0], prob[-1, -1] = 0.0, 1.0
    want_p = S.discrete(0xC0FFEE + H, g, K, H, prob=prob)
    for dt in (torch.uint8, torch.int32, torch.int64):
        got = eng.sample_candidates(H, K, 0xC0FFEE + H, dtype=dt)
        assert got.dtype == dt and tuple(got.shape) == (H, N, K)
        assert np.array_equal(got.cpu().numpy(), want.astype(got.cpu().numpy().dtype)), dt
        got = eng.sample_candidates(H, K, 0xC0FFEE + H, nominal=torch.as_tensor(prob, device=eng.device), dtype=dt)
        assert np.array_equal(got.cpu().numpy(), want_p.astype(got.cpu().numpy().dtype)), dt
    assert eng.sample_candidates(H, K, 1).dtype == torch.int64  # the dtype step() takes
    assert not np.array_equal(eng.sample_candidates(H, K, 1).cpu().numpy(), want)  # another seed, other sequences (>= 65 draws)


@pytest.mark.parametrize("H", [1, 4, 5, 9])
@pytest.mark.parametrize("name,A", [("ReboundInvertedPendulumBalancing", 1), ("HopperRunning", 3), ("HalfCheetahRunning", 6)])
def test_continuous_candidates_equal_the_spec(name, A, H):
    """act_dim 3 and 6: a step's components cross a Philox block (and, in the Gaussian mode, a Box-Muller pair straddles steps)"""
    lo, hi = RANGE[name]
    for N, K in SHAPES[:2]:
        eng = _engine(name, N, env_index_offset=OFFSET)
        assert eng.act_dim == A
        g = _globals(N, OFFSET)
        seed = (0xABCDEF << 20) + 31 * H + A
        got = eng.sample_candidates(H, K, seed)
        assert got.dtype == torch.float32 and tuple(got.shape) == (H, N, K) + ((A,) if A > 1 else ())
        got = got.cpu().numpy().reshape(H, N, K, A)
        assert np.array_equal(got, S.uniform(seed, g, K, H, A, lo, hi))  # bit for bit
        rng = np.random.default_rng(A * 100 + H)
        mean = rng.uniform(0.8 * lo, 0.8 * hi, (H, N, A)).astype(np.float32)
        for sigma in (0.05, 0.3 * hi, 2.0 * hi):  # 2 hi: most draws clip
            z = eng.sample_candidates(H, K, seed, nominal=torch.as_tensor(mean.reshape(H, N, A) if A > 1 else mean[..., 0],
                                                                          device=eng.device), sigma=sigma)
            z = z.cpu().numpy().reshape(H, N, K, A).astype(np.float64)
            ref = S.gaussian_exact(seed, g, K, H, A, lo, hi, mean, sigma)
            # sigma * (the bound tests/test_gpu_device_math.py asserts for boxmuller) + one float32 rounding of a value <= 3
            err = np.abs(z - ref).max()
            print(f"{name} H={H} N={N} K={K} sigma={sigma}: max |action - exact| = {err:.3e}, bound {sigma * 1.6e-6 + 4e-7:.3e}")
            assert err <= sigma * 1.6e-6 + 4e-7
            assert z.min() >= lo and z.max() <= hi
        eng.close()


# ------------------------------------------------------------------------------------------------ b. the planner's definition
def _nominal(eng, H, N, seed):
    rng = np.random.default_rng(seed)
    if eng.act_dim == 0:
        return torch.as_tensor(rng.uniform(0, 1, (H, N)).astype(np.float32), device=eng.device), None
    lo, hi = (-3.0, 3.0) if "InvertedPendulum" in eng.env_name and "Double" not in eng.env_name else (-1.0, 1.0)
    shape = (H, N, eng.act_dim) if eng.act_dim > 1 else (H, N)
    return torch.as_tensor(rng.uniform(0.5 * lo, 0.5 * hi, shape).astype(np.float32), device=eng.device), 0.4 * hi


def _check_definition(eng, H, K, seed, gamma, nominal=None, sigma=None, start_state=None, dtype=None, cheetah=False):
    """plan_shooting against evaluate_sequences on sample_candidates -> (cand, ret, L, outputs) as NumPy"""
    N = eng.n_envs
    cand = eng.sample_candidates(H, K, seed, nominal=nominal, sigma=sigma, dtype=dtype)
    ret, L = eng.evaluate_sequences(cand, discount=gamma, start_state=start_state)
    act, bret, idx, seq, blen = eng.plan_shooting(H, K, seed, discount=gamma, nominal=nominal, sigma=sigma, start_state=start_state,
                                                  sequence=True, length=True, dtype=dtype)
    assert act.dtype == cand.dtype and seq.dtype == cand.dtype and bret.dtype == torch.float64
    assert idx.dtype == torch.int32 and blen.dtype == torch.int32
    tail = (eng.act_dim,) if eng.act_dim > 1 else ()
    assert tuple(act.shape) == (N,) + tail and tuple(seq.shape) == (H, N) + tail and tuple(idx.shape) == (N,)
    cand, ret, L, act, bret, idx, seq, blen = (x.cpu().numpy() for x in (cand, ret, L, act, bret, idx, seq, blen))
    rows = np.arange(N)
    assert (idx >= 0).all() and (idx < K).all()
    if cheetah:
        # the cheetah's constraint-slot lending makes a lane depend on its wave-mates at the 1e-9 level — the project's
        # one stated exception to lane independence, and the bound tests/test_gpu_plan.py uses for it
        best = ret.max(1)
        assert (np.abs(ret[rows, idx] - best) <= 1e-9 * np.maximum(np.abs(best), 1e-3)).all()
        assert rel_err(bret, ret[rows, idx]) <= 1e-9
    else:
        assert np.array_equal(idx, S.best_of(ret))
        if not np.isnan(ret).any():
            assert np.array_equal(idx, ret.argmax(1))  # the first maximum
        assert np.array_equal(bret, ret[rows, idx], equal_nan=True)  # bit for bit
        assert np.array_equal(blen, L[rows, idx])
    assert np.array_equal(act, cand[0, rows, idx])
    assert np.array_equal(seq, cand[:, rows, idx])
    return cand, ret, L, (act, bret, idx, seq, blen)


CH = dict(freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"])
# (env, engine kwargs, N, K, H, discount, start_state, nominal, dtype).  (5, 13) straddles waves, (64, 64) is whole waves, (3, 300)
# has an env on two blocks, (257, 1) and (1, 257) the degenerate reductions; H from 1 to 60
CASES = [
    ("CartPoleSwingUp", dict(precision="ref"), 5, 13, 60, 1.0, False, False, torch.uint8),
    ("CartPoleSwingUp", dict(precision="f32", freq_rate=2), 64, 64, 40, 0.99, True, True, torch.int32),
    ("CartPoleSwingUp", dict(precision="ref", ode_method="rk4"), 257, 1, 30, 0.99, False, True, torch.int64),
    ("CartPoleSwingUp", dict(precision="f32", ode_method="rk4", freq_rate=2), 1, 257, 25, 1.0, True, False, None),
    ("CartPoleSwingUp", dict(precision="ref"), 3, 300, 1, 0.99, False, False, None),
    ("CartPoleBalancing", dict(precision="ref"), 3, 300, 50, 0.99, False, False, torch.uint8),
    ("CartPoleBalancing", dict(precision="f32"), 64, 64, 9, 1.0, True, True, None),
    ("ReboundInvertedPendulumBalancing", dict(precision="ref"), 5, 13, 50, 0.99, False, True, None),
    ("BoundaryInvertedPendulumSwingUp", dict(precision="f32"), 64, 64, 17, 1.0, True, False, None),
    ("ReboundInvertedPendulumSwingUp", dict(precision="ref", integrator="rk4"), 5, 13, 30, 0.99, True, False, None),
    ("ReboundInvertedDoublePendulumBalancing", dict(precision="ref"), 3, 300, 40, 0.99, False, True, None),
    ("HalfCheetahRunning", dict(precision="ref", **CH), 5, 13, 12, 0.99, False, True, None),
    ("HopperRunning", dict(precision="f32", **CH), 5, 13, 25, 1.0, True, False, None),
    ("HopperRunning", dict(precision="ref", integrator="rk4", **CH), 3, 300, 10, 0.99, False, True, None),
]


@pytest.mark.parametrize("name,kw,N,K,H,gamma,start,nominal,dtype", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_planner_equals_its_definition(name, kw, N, K, H, gamma, start, nominal, dtype):
    eng = _engine(name, N, env_index_offset=3, **kw)
    eng.reset(seed=21 + N)
    st = None
    if start:
        g = torch.Generator(device=eng.device).manual_seed(5)
        st = eng.get_state() + 0.02 * torch.randn((N, eng.state_dim), generator=g, device=eng.device, dtype=torch.float64)
    nom, sigma = _nominal(eng, H, N, seed=K) if nominal else (None, None)
    cand, ret, L, _ = _check_definition(eng, H, K, 1000 * N + K, gamma, nominal=nom, sigma=sigma, start_state=st, dtype=dtype,
                                        cheetah=name == "HalfCheetahRunning")
    if K > 1:
        assert (cand[:, :, 0] != cand[:, :, 1]).any() or H == 1  # the candidates differ
    assert eng.solver_cap_hits() == 0


# ------------------------------------------------------------------------------------------------ c. ties
def test_ties_go_to_the_lowest_index():
    N, K = 70, 100  # an env's 100 candidates lie on two or three waves
    eng = _engine("CartPoleBalancing", N)
    eng.reset(seed=2)
    cand, ret, L, (act, bret, idx, seq, blen) = _check_definition(eng, 3, K, 77, 1.0)
    assert (ret == 3.0).all() and (idx == 0).all() and (bret == 3.0).all() and (blen == 3).all()
    # long enough for the candidates to fail, at different steps (the return is the number of steps survived: integers, so
    # maxima are shared often): still the first maximum
    cand, ret, L, (act, bret, idx, seq, blen) = _check_definition(eng, 200, K, 78, 1.0)
    assert len(np.unique(L)) > 3 and np.array_equal(ret, L.astype(np.float64))
    assert np.array_equal(idx, ret.argmax(1))


# ------------------------------------------------------------------------------------------------ d. NaN rows
@pytest.mark.parametrize("name", ["CartPoleSwingUp", "CartPoleBalancing", "BoundaryInvertedPendulumBalancing"])
def test_odd_start_rows(name):
    """NaN, +-inf, beyond-threshold and on-threshold start rows mixed with ordinary ones inside one wave (the rows
    tests/test_gpu_plan.py sends through the same kernels), plus rows that are NaN throughout"""
    from test_gpu_plan import _odd_rows

    N, K, H, gamma = 70, 3, 12, 0.95
    plain, rows, odd = _odd_rows(name, np.random.default_rng(5), N)
    rows[[3, 64]] = np.nan  # every coordinate: in the first wave and at the start of the second
    odd = np.union1d(odd, [3, 64])
    eng = _engine(name, N)
    eng.reset(seed=1)
    with np.errstate(all="ignore"):
        cand, ret, L, (act, bret, idx, seq, blen) = _check_definition(eng, H, K, 9, gamma, start_state=torch.as_tensor(rows, device=eng.device))
    all_nan = np.isnan(ret).all(1)
    if name == "CartPoleSwingUp":  # its reward is (cos theta + 1) / 2: a NaN row has NaN returns (the other two pay 1 per step)
        assert all_nan[[3, 64]].all()
    assert (idx[all_nan] == 0).all() and np.isnan(bret[all_nan]).all()
    assert not np.isnan(bret[~all_nan]).any()
    # the ordinary envs of the same waves: as without the odd neighbours
    _, _, _, (act0, bret0, idx0, seq0, blen0) = _check_definition(eng, H, K, 9, gamma, start_state=torch.as_tensor(plain, device=eng.device))
    keep = np.setdiff1d(np.arange(N), odd)
    assert np.array_equal(idx[keep], idx0[keep]) and np.array_equal(bret[keep], bret0[keep]) and np.array_equal(blen[keep], blen0[keep])
    assert np.array_equal(act[keep], act0[keep]) and np.isfinite(bret0).all()


# ------------------------------------------------------------------------------------------------ e. shard invariance
@pytest.mark.parametrize("name,kw,nominal", [("CartPoleSwingUp", dict(), True), ("HopperRunning", dict(CH), False)])
def test_shards_give_the_whole(name, kw, nominal):
    N, K, H = 128, 24, 15
    whole = _engine(name, N, env_index_offset=0, **kw)
    parts = [_engine(name, 64, env_index_offset=o, **kw) for o in (0, 64)]
    whole.reset(seed=6)
    st = whole.get_state()
    nom, sigma = _nominal(whole, H, N, seed=1) if nominal else (None, None)
    want = whole.plan_shooting(H, K, 99, discount=0.97, nominal=nom, sigma=sigma, start_state=st, sequence=True, length=True)
    got = []
    for p, sl in zip(parts, (slice(0, 64), slice(64, 128))):
        got.append(p.plan_shooting(H, K, 99, discount=0.97, nominal=None if nom is None else nom[:, sl].contiguous(), sigma=sigma,
                                   start_state=st[sl].contiguous(), sequence=True, length=True))
    for q, w in enumerate(want):
        cat = torch.cat([got[0][q], got[1][q]], dim=1 if q == 3 else 0)
        assert torch.equal(cat, w), q
    assert not torch.equal(want[2][:64], want[2][64:])  # the two halves do not simply repeat each other
    c = [p.sample_candidates(H, K, 99) for p in parts]
    assert torch.equal(torch.cat(c, dim=1), whole.sample_candidates(H, K, 99))


# ------------------------------------------------------------------------------------------------ f. the handle is untouched
@pytest.mark.parametrize("name,kw", [("CartPoleSwingUp", dict(max_episode_steps=9)), ("HopperRunning", dict(max_episode_steps=6, **CH))])
def test_handle_untouched(name, kw):
    N = 96
    a, b = _engine(name, N, seed=4, **kw), _engine(name, N, seed=4, **kw)
    g = torch.Generator(device=a.device).manual_seed(9)
    step_acts = torch.randint(0, 2, (20, N), generator=g, device=a.device, dtype=torch.uint8) if a.act_dim == 0 \
        else torch.rand((20, N, a.act_dim), generator=g, device=a.device) * 2 - 1
    for e in (a, b):
        e.reset(seed=4)
        e.rollout(step_acts[:7], auto_reset=True)
        e.freeze()
        e.rollout(step_acts[7:12], auto_reset=True)
    a.plan_shooting(15, 5, 123, discount=0.9, sequence=True, length=True)
    assert torch.equal(a.get_state(), b.get_state())
    for x, y in zip(a.get_counters(), b.get_counters()):
        assert torch.equal(x, y)
    outs = [e.rollout(step_acts, auto_reset=True) for e in (a, b)]  # auto-reset: the reset key is the handle's own still
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    for e in (a, b):
        e.unfreeze()
    assert torch.equal(a.get_state(), b.get_state())
    outs = [e.rollout(step_acts, auto_reset=True) for e in (a, b)]
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_capture_replays_the_same_result():
    N, K, H = 256, 16, 50
    eng = _engine("CartPoleSwingUp", N)
    eng.reset(seed=8)
    want = eng.plan_shooting(H, K, 31, discount=0.99, sequence=True, length=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one linear chain: plan, finish
        got = eng.plan_shooting(H, K, 31, discount=0.99, sequence=True, length=True)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)


def test_argument_checks_on_a_handle():
    eng = _engine("HopperRunning", 4)
    with pytest.raises(AssertionError):  # EMEI_ERR_STATE: no reset yet
        eng.plan_shooting(3, 2, 0)
    eng.sample_candidates(3, 2, 0)  # needs no state
    eng.reset(seed=0)
    good = torch.zeros((3, 4, 3), device=eng.device)
    eng.plan_shooting(3, 2, 0, nominal=good, sigma=0.1)
    for bad in (dict(nominal=good[:2].contiguous(), sigma=0.1), dict(nominal=good.double(), sigma=0.1), dict(nominal=good.cpu(), sigma=0.1),
                dict(nominal=good.transpose(0, 1), sigma=0.1), dict(nominal=good), dict(nominal=good, sigma=0.0),
                dict(nominal=good, sigma=float("nan")), dict(discount=0.0), dict(dtype=torch.int64),
                dict(start_state=torch.zeros(4, eng.state_dim, device=eng.device))):
        with pytest.raises(ValueError):
            eng.plan_shooting(3, 2, 0, **bad)
    with pytest.raises(ValueError):
        eng.plan_shooting(0, 2, 0)
    with pytest.raises(ValueError):
        eng.sample_candidates(3, 0, 0)


def test_env_surface_numpy_and_tensor():
    import emei_amd

    env = emei_amd.make("CartPoleSwingUp-v0", num_envs=8)
    with pytest.raises(AssertionError):
        env.plan_random_shooting(5, 4, 0)
    obs, _ = env.reset(seed=0)
    act, ret, idx = env.plan_random_shooting(10, 16, seed=3, discount=0.99)
    assert isinstance(act, torch.Tensor) and act.dtype == torch.int64 and tuple(act.shape) == (8,)  # what step() takes
    env.step(act)
    prob = np.full((10, 8), 0.5, np.float32)
    out = env.plan_random_shooting(10, 16, seed=3, discount=0.99, nominal=prob, sequence=True, length=True)
    assert all(isinstance(x, np.ndarray) for x in out) and out[3].shape == (10, 8) and out[4].dtype == np.int32
    hop = emei_amd.make("HopperRunning-v0", num_envs=4)
    hop.reset(seed=0)
    act, ret, idx = hop.plan_random_shooting(4, 8, seed=1)
    assert act.dtype == torch.float32 and tuple(act.shape) == (4, 3) and float(act.abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------ g. the README's MPC loop
def test_mpc_loop_equals_the_four_launch_composition():
    N, K, H = 64, 32, 20
    eng = _engine("CartPoleSwingUp", N)
    eng.reset(seed=0)
    rows = torch.arange(N, device=eng.device)
    total = torch.zeros(N, device=eng.device)
    for t in range(20):
        best, ret, idx = eng.plan_shooting(H, K, seed=1000 + t, discount=0.99)
        cand = eng.sample_candidates(H, K, seed=1000 + t)
        r, _ = eng.evaluate_sequences(cand, discount=0.99)
        pick = cand[0, rows, r.argmax(1)]
        assert torch.equal(best, pick), t
        assert torch.equal(ret, r.max(1).values), t
        obs, rew, done = eng.step(best)
        total += rew
    assert float(total.min()) > 0
