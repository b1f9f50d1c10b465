"""emei_plan_mppi on the GPU (Engine.plan_mppi / HipEnv.plan_mppi).

The yardstick is the definition: for the candidates emei_sample_candidates writes out and the returns emei_evaluate_sequences
gives them (both tied to the specification and to the CPU oracle by their own tests), the NumPy case analysis of
tests/mppi_reference.py in float64.  Tolerances: the kernel and the reference differ by float64 exp and summation order only,
about K * 2^-52 relative, which can move the one final rounding to float32 by at most one float32 step — one spacing at
max(|lo|, |hi|) of the env's range (np.spacing(np.float32(1)) for the discrete envs' probabilities); the effective sample size
stays in float64 and is held to 1e-12 relative.  best_index / best_return are emei_plan_shooting's, bit for bit."""
import numpy as np
import pytest

import mppi_reference as M
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MUJOCO = {"dt": 0.002, "fr": 4}  # half_cheetah.py:12, hopper.py:20
CH = dict(freq_rate=MUJOCO["fr"], real_time_scale=MUJOCO["dt"])
OFFSET = (1 << 32) + 7  # env_index_offset: the global env index reaches the second counter word


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


def _range(eng):
    """(lo, hi) of the values nominal_out can take: the ctrlrange, or [0, 1] for the discrete envs' probabilities"""
    if eng.act_dim == 0:
        return 0.0, 1.0
    return (-3.0, 3.0) if "InvertedPendulum" in eng.env_name and "Double" not in eng.env_name else (-1.0, 1.0)


def _step_tol(eng):
    lo, hi = _range(eng)
    return float(np.spacing(np.float32(max(abs(lo), abs(hi)))))


def _nominal(eng, H, seed):
    """a nominal in the layout plan_mppi returns: probabilities (discrete) or means with a sigma (continuous)"""
    rng = np.random.default_rng(seed)
    N = eng.n_envs
    if eng.act_dim == 0:
        return torch.as_tensor(rng.uniform(0.1, 0.9, (H, N)).astype(np.float32), device=eng.device), None
    lo, hi = _range(eng)
    shape = (H, N, eng.act_dim) if eng.act_dim > 1 else (H, N)
    return torch.as_tensor(rng.uniform(0.5 * lo, 0.5 * hi, shape).astype(np.float32), device=eng.device), 0.4 * hi


def _start(eng, seed=5):
    g = torch.Generator(device=eng.device).manual_seed(seed)
    return eng.get_state() + 0.02 * torch.randn((eng.n_envs, eng.state_dim), generator=g, device=eng.device, dtype=torch.float64)


def _temperature(ret):
    """the mean over envs of the standard deviation of each env's finite returns, or 1.0 if that is 0"""
    sds = [np.std(r[np.isfinite(r)]) for r in ret if np.isfinite(r).any()]
    t = float(np.mean(sds)) if sds else 0.0
    return t if t > 0.0 else 1.0


def _check_definition(eng, H, K, seed, gamma, temperature=None, nominal=None, sigma=None, start_state=None, cheetah=False, out=None,
                      label=""):
    """plan_mppi against mppi_reference on (sample_candidates, evaluate_sequences) -> (cand, ret, reference, outputs) as NumPy"""
    N = eng.n_envs
    cand = eng.sample_candidates(H, K, seed, nominal=nominal, sigma=sigma)
    ret, _ = eng.evaluate_sequences(cand, discount=gamma, start_state=start_state)
    _, sret, sidx = eng.plan_shooting(H, K, seed, discount=gamma, nominal=nominal, sigma=sigma, start_state=start_state)
    cand, ret = cand.cpu().numpy(), ret.cpu().numpy()
    T = _temperature(ret) if temperature is None else temperature
    with np.errstate(all="ignore"):
        want, wret, widx, wess = M.mppi(cand, ret, T)
    got, bret, idx, ess = eng.plan_mppi(H, K, seed, T, discount=gamma, nominal=nominal, sigma=sigma, start_state=start_state, out=out,
                                        ess=True)
    tail = (eng.act_dim,) if eng.act_dim > 1 else ()
    assert got.dtype == torch.float32 and bret.dtype == torch.float64 and idx.dtype == torch.int32 and ess.dtype == torch.float64
    assert tuple(got.shape) == (H, N) + tail and tuple(bret.shape) == (N,) and tuple(idx.shape) == (N,) and tuple(ess.shape) == (N,)
    # the winner is emei_plan_shooting's, bit for bit
    assert torch.equal(idx, sidx) and np.array_equal(bret.cpu().numpy(), sret.cpu().numpy(), equal_nan=True)
    got, bret, idx, ess = (x.cpu().numpy() for x in (got, bret, idx, ess))
    tol, ess_tol = _step_tol(eng), 1e-12
    if cheetah:
        # r_k may differ from the composition's by 1e-9 relative (the constraint-slot lending).  A soft-max mean moves by
        # at most (hi - lo) * max |d r_k| / temperature, ln ESS by at most 4 * max |d(r_k - r*)| / temperature
        lo, hi = _range(eng)
        slack = 1e-9 * np.abs(ret).max() / T
        tol, ess_tol = tol + (hi - lo) * slack, ess_tol + 8 * slack
        assert rel_err(bret, wret) <= 1e-9
        best = ret.max(1)
        assert (np.abs(ret[np.arange(N), idx] - best) <= 1e-9 * np.maximum(np.abs(best), 1e-3)).all()
    else:
        assert np.array_equal(idx, widx) and np.array_equal(bret, wret, equal_nan=True)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    ess_err = np.abs(ess - wess) / wess
    print(f"{label or eng.env_name} N={N} K={K} H={H} T={T:.4g}: max |nominal_out - reference| = {err:.3e} (bound {tol:.3e}), "
          f"ess rel err {ess_err.max():.3e} (bound {ess_tol:.1e}), reference ess {wess.min():.3f} .. {wess.max():.3f}")
    assert np.isfinite(got).all()
    assert err <= tol
    assert (ess_err <= ess_tol).all()
    lo, hi = _range(eng)
    assert got.min() >= lo and got.max() <= hi
    return cand, ret, (want, wret, widx, wess), (got, bret, idx, ess)


# ------------------------------------------------------------------------------------------------ a. the definition
# (env, engine kwargs, N, K, H, discount, start_state, nominal): (5, 13) straddles waves, (64, 64) is whole waves, (3, 300) spreads an
# env over blocks of the first launch and gives lanes several candidates, (257, 1) and (1, 257) are the degenerate reductions; the
# Hopper's 15 words leave the last Box-Muller pair half used and put components astride Philox blocks
CASES = [
    ("CartPoleSwingUp", dict(precision="ref", env_index_offset=OFFSET), 5, 13, 9, 0.99, False, False),
    ("CartPoleSwingUp", dict(precision="f32", freq_rate=2), 64, 64, 40, 0.99, True, True),
    ("CartPoleBalancing", dict(), 3, 300, 50, 1.0, False, False),  # integer returns: many ties
    ("CartPoleSwingUp", dict(), 257, 1, 5, 1.0, False, False),
    ("CartPoleSwingUp", dict(env_index_offset=OFFSET), 1, 257, 5, 0.99, False, True),
    ("ReboundInvertedPendulumBalancing", dict(precision="ref"), 5, 13, 5, 0.99, False, False),  # uniform draws
    ("ReboundInvertedPendulumBalancing", dict(precision="ref"), 5, 13, 5, 0.99, True, True),  # Gaussian draws
    ("ReboundInvertedDoublePendulumBalancing", dict(), 3, 300, 7, 0.99, False, True),
    ("HopperRunning", dict(**CH), 5, 13, 5, 0.99, True, True),
    ("HalfCheetahRunning", dict(**CH), 5, 13, 3, 0.99, False, True),
]


@pytest.mark.parametrize("name,kw,N,K,H,gamma,start,nominal", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_update_equals_its_definition(name, kw, N, K, H, gamma, start, nominal):
    kw = dict(kw)
    kw.setdefault("env_index_offset", 3)
    eng = _engine(name, N, **kw)
    eng.reset(seed=21 + N)
    st = _start(eng) if start else None
    nom, sigma = _nominal(eng, H, seed=K) if nominal else (None, None)
    cand, ret, (want, wret, widx, wess), (got, bret, idx, ess) = _check_definition(
        eng, H, K, 1000 * N + K, gamma, nominal=nom, sigma=sigma, start_state=st, cheetah=name == "HalfCheetahRunning")
    if K == 1:
        assert np.array_equal(got, cand[:, :, 0].astype(np.float32)) and (ess == 1.0).all() and (idx == 0).all()
    elif not (ret == ret[:, :1]).all():
        # the case is neither an arg-max nor a plain mean in disguise
        assert ((wess > 1.5) & (wess < 0.9 * K)).any(), wess
    if eng.act_dim == 0 and K > 1:
        assert ((got > 0) & (got < 1)).any()  # probabilities, not copies of one candidate
    assert eng.solver_cap_hits() == 0


# ------------------------------------------------------------------------------------------------ b. the temperature limits
@pytest.fixture(scope="module")
def balancing():
    """CartPoleBalancing, long enough for the candidates to fail at different steps: the return is the number of steps survived,
    so maxima are shared often.  (engine, cand, ret) with cand / ret as NumPy"""
    N, K, H = 70, 100, 200
    eng = _engine("CartPoleBalancing", N)
    eng.reset(seed=2)
    cand = eng.sample_candidates(H, K, 78)
    ret, _ = eng.evaluate_sequences(cand, discount=1.0)
    return eng, cand.cpu().numpy().astype(np.float64), ret.cpu().numpy()


def test_cold_limit_is_the_mean_over_the_maximisers(balancing):
    eng, cand, ret = balancing
    H, N, K = cand.shape
    maxi = ret == ret.max(1, keepdims=True)
    assert (maxi.sum(1) > 1).any() and len(np.unique(ret)) > 3
    got, bret, idx, ess = eng.plan_mppi(H, K, 78, 1e-300, ess=True)
    want = ((cand * maxi[None]).sum(2) / maxi.sum(1)[None]).astype(np.float32)
    assert np.abs(got.cpu().numpy().astype(np.float64) - want).max() <= _step_tol(eng)
    assert np.array_equal(ess.cpu().numpy(), maxi.sum(1).astype(np.float64))
    assert np.array_equal(idx.cpu().numpy(), ret.argmax(1)) and np.array_equal(bret.cpu().numpy(), ret.max(1))
    _check_definition(eng, H, K, 78, 1.0, temperature=1e-300, label="cold limit")


def test_hot_limit_is_the_plain_mean(balancing):
    eng, cand, ret = balancing
    H, N, K = cand.shape
    got, bret, idx, ess = eng.plan_mppi(H, K, 78, 1e300, ess=True)
    assert np.abs(got.cpu().numpy().astype(np.float64) - cand.mean(2).astype(np.float32)).max() <= _step_tol(eng)
    assert (np.abs(ess.cpu().numpy() - K) <= 1e-12 * K).all()
    assert np.array_equal(idx.cpu().numpy(), ret.argmax(1))
    _check_definition(eng, H, K, 78, 1.0, temperature=1e300, label="hot limit")


# ------------------------------------------------------------------------------------------------ c. NaN rows
def test_odd_start_rows():
    """NaN, +-inf, beyond-threshold and on-threshold start rows mixed with ordinary ones inside one wave (the rows
    tests/test_gpu_plan.py sends through the same kernels), plus two rows that are NaN throughout"""
    from test_gpu_plan import _odd_rows

    name, N, K, H, gamma, T = "CartPoleSwingUp", 70, 3, 12, 0.95, 0.5
    plain, rows, odd = _odd_rows(name, np.random.default_rng(5), N)
    rows[[3, 64]] = np.nan  # every coordinate: in the first wave and at the start of the second
    odd = np.union1d(odd, [3, 64])
    eng = _engine(name, N)
    eng.reset(seed=1)
    cand, ret, _, (got, bret, idx, ess) = _check_definition(eng, H, K, 9, gamma, temperature=T,
                                                            start_state=torch.as_tensor(rows, device=eng.device), label="odd rows")
    all_nan = np.isnan(ret).all(1)
    assert all_nan[[3, 64]].all()  # the reward is (cos theta + 1) / 2: a NaN row has NaN returns
    # all-NaN envs: the uniform mean, k* = 0, a NaN return
    uniform = cand.astype(np.float64).mean(2)
    assert np.abs(got[:, all_nan] - uniform[:, all_nan]).max() <= _step_tol(eng)
    assert (idx[all_nan] == 0).all() and np.isnan(bret[all_nan]).all() and (np.abs(ess[all_nan] - K) <= 1e-12 * K).all()
    assert not np.isnan(bret[~all_nan]).any()
    # the ordinary envs of the same waves: the bits of a run without the odd neighbours
    _, _, _, (got0, bret0, idx0, ess0) = _check_definition(eng, H, K, 9, gamma, temperature=T,
                                                           start_state=torch.as_tensor(plain, device=eng.device), label="plain rows")
    keep = np.setdiff1d(np.arange(N), odd)
    assert np.array_equal(got[:, keep], got0[:, keep]) and np.array_equal(ess[keep], ess0[keep])
    assert np.array_equal(idx[keep], idx0[keep]) and np.array_equal(bret[keep], bret0[keep]) and np.isfinite(bret0).all()


# ------------------------------------------------------------------------------------------------ d. shard invariance
@pytest.mark.parametrize("name,kw,nominal", [("CartPoleSwingUp", dict(), True), ("HopperRunning", dict(CH), False)])
def test_shards_give_the_whole(name, kw, nominal):
    N, K, H, T = 192, 24, 15, 0.7
    whole = _engine(name, N, env_index_offset=0, **kw)
    parts = [_engine(name, 64, env_index_offset=o, **kw) for o in (0, 64, 128)]
    whole.reset(seed=6)
    st = whole.get_state()
    nom, sigma = _nominal(whole, H, seed=1) if nominal else (None, None)
    want = whole.plan_mppi(H, K, 99, T, discount=0.97, nominal=nom, sigma=sigma, start_state=st, ess=True)
    got = []
    for p, o in zip(parts, (0, 64, 128)):
        sl = slice(o, o + 64)
        got.append(p.plan_mppi(H, K, 99, T, discount=0.97, nominal=None if nom is None else nom[:, sl].contiguous(), sigma=sigma,
                               start_state=st[sl].contiguous(), ess=True))
    for q, w in enumerate(want):
        cat = torch.cat([g[q] for g in got], dim=1 if q == 0 else 0)
        assert torch.equal(cat, w), q
    assert not torch.equal(want[0][:, :64], want[0][:, 64:128])  # the shards do not simply repeat each other
    assert float(want[3].min()) > 1.0 and float(want[3].max()) < K  # a soft-max, not an arg-max or a plain mean


# ------------------------------------------------------------------------------------------------ e. in place
@pytest.mark.parametrize("name,kw,N,K,H", [("CartPoleSwingUp", dict(), 70, 100, 21), ("HopperRunning", dict(CH), 5, 13, 5),
                                           ("ReboundInvertedPendulumSwingUp", dict(), 64, 64, 10)])
def test_in_place_equals_out_of_place(name, kw, N, K, H):
    eng = _engine(name, N, **kw)
    eng.reset(seed=3)
    nom, sigma = _nominal(eng, H, seed=2)
    keep = nom.clone()
    want = eng.plan_mppi(H, K, 5, 0.3, discount=0.99, nominal=nom, sigma=sigma, ess=True)
    assert torch.equal(nom, keep) and want[0].data_ptr() != nom.data_ptr()
    other = torch.full_like(nom, 7.0)
    got = eng.plan_mppi(H, K, 5, 0.3, discount=0.99, nominal=nom, sigma=sigma, out=other, ess=True)
    assert got[0] is other and torch.equal(other, want[0]) and torch.equal(nom, keep)
    got = eng.plan_mppi(H, K, 5, 0.3, discount=0.99, nominal=nom, sigma=sigma, out=nom, ess=True)
    assert got[0] is nom
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert not torch.equal(nom, keep)


# ------------------------------------------------------------------------------------------------ f. the contract
def test_repeat_calls_give_the_same_bits():
    eng = _engine("HopperRunning", 37, **CH)
    eng.reset(seed=4)
    nom, sigma = _nominal(eng, 6, seed=3)
    a = eng.plan_mppi(6, 70, 11, 0.4, discount=0.99, nominal=nom, sigma=sigma, ess=True)
    eng.plan_mppi(3, 200, 12, 0.1)  # another shape through the same workspace in between
    b = eng.plan_mppi(6, 70, 11, 0.4, discount=0.99, nominal=nom, sigma=sigma, ess=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert eng.solver_cap_hits() == 0


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
    a.plan_mppi(15, 5, 123, 0.5, discount=0.9, ess=True)
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
    nom, _ = _nominal(eng, H, seed=4)
    want = eng.plan_mppi(H, K, 31, 0.2, discount=0.99, nominal=nom, ess=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one linear chain: plan, finish
        got = eng.plan_mppi(H, K, 31, 0.2, discount=0.99, nominal=nom, ess=True)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for x in got:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)


def test_argument_checks_on_a_handle():
    eng = _engine("HopperRunning", 4)
    with pytest.raises(AssertionError):  # EMEI_ERR_STATE: no reset yet
        eng.plan_mppi(3, 2, 0, 1.0)
    eng.reset(seed=0)
    good = torch.zeros((3, 4, 3), device=eng.device)
    eng.plan_mppi(3, 2, 0, 1.0, nominal=good, sigma=0.1)
    out, ret, idx = eng.plan_mppi(3, 2, 0, 1.0)
    assert tuple(out.shape) == (3, 4, 3) and out.dtype == torch.float32
    for bad in (dict(nominal=good[:2].contiguous(), sigma=0.1), dict(nominal=good.double(), sigma=0.1), dict(nominal=good.cpu(), sigma=0.1),
                dict(nominal=good.transpose(0, 1), sigma=0.1), dict(nominal=good), dict(nominal=good, sigma=0.0),
                dict(nominal=good, sigma=float("nan")), dict(discount=0.0), dict(out=good[:2].contiguous()), dict(out=good.double()),
                dict(out=good.cpu()), dict(start_state=torch.zeros(4, eng.state_dim, device=eng.device))):
        with pytest.raises(ValueError):
            eng.plan_mppi(3, 2, 0, 1.0, **bad)
    for T in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            eng.plan_mppi(3, 2, 0, T)
    with pytest.raises(ValueError):
        eng.plan_mppi(0, 2, 0, 1.0)
    with pytest.raises(ValueError):
        eng.plan_mppi(3, 0, 0, 1.0)


def test_env_surface_numpy_and_tensor():
    import emei_amd

    env = emei_amd.make("CartPoleSwingUp-v0", num_envs=8)
    with pytest.raises(AssertionError):
        env.plan_mppi(5, 4, 0, 1.0)
    env.reset(seed=0)
    prob, ret, idx = env.plan_mppi(10, 16, seed=3, temperature=0.1, discount=0.99)
    assert isinstance(prob, torch.Tensor) and prob.dtype == torch.float32 and tuple(prob.shape) == (10, 8)
    assert float(prob.min()) >= 0.0 and float(prob.max()) <= 1.0 and ret.dtype == torch.float64 and idx.dtype == torch.int32
    env.step((prob[0] >= 0.5).to(torch.int64))
    out = env.plan_mppi(10, 16, seed=3, temperature=0.1, discount=0.99, nominal=np.full((10, 8), 0.5, np.float32), ess=True)
    assert all(isinstance(x, np.ndarray) for x in out) and out[0].shape == (10, 8) and out[3].dtype == np.float64
    hop = emei_amd.make("HopperRunning-v0", num_envs=4)
    hop.reset(seed=0)
    mean, ret, idx = hop.plan_mppi(4, 8, seed=1, temperature=0.5)
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (4, 4, 3) and float(mean.abs().max()) <= 1.0
    again = hop.plan_mppi(4, 8, seed=2, temperature=0.5, nominal=mean, sigma=0.3, out=mean)
    assert again[0] is mean
    hop.step(mean[0])


# ------------------------------------------------------------------------------------------------ g. the output is a valid input
@pytest.mark.parametrize("name,kw,N,K,H", [("CartPoleSwingUp", dict(), 33, 40, 12), ("HopperRunning", dict(CH), 5, 13, 5)])
def test_chained_updates_each_equal_their_definition(name, kw, N, K, H):
    """three calls, each taking the previous nominal_out as its nominal: pins that the output is a valid input (not that the
    planner improves anything)"""
    eng = _engine(name, N, **kw)
    eng.reset(seed=7)
    nom, sigma = None, (None if eng.act_dim == 0 else 0.3)
    for it in range(3):
        _, _, _, (got, _, _, _) = _check_definition(eng, H, K, 50 + it, 0.99, nominal=nom, sigma=sigma if nom is not None else None,
                                                   label=f"{name} chained call {it}")
        nom = torch.as_tensor(got, device=eng.device)
        if eng.act_dim == 0:
            nom = nom.clamp(0.05, 0.95)  # the caller keeps the coins exploring
        nom = nom.contiguous()
