"""emei_mpc_mppi / emei_mpc_cem on the InvertedDoublePendulum (body_mpc_mppi_kernel / body_mpc_cem_kernel), on the GPU.

The yardstick is the loop each call fuses, written against the API as it stood before (tests/mpc_reference.py, tests/mpc_cem_reference.py:
plan_mppi / plan_cem in place, step, clamp, shift, refill — body_plan_kernel, the finish kernels and body_rollout_kernel).  Two engines
of one configuration start from the same rows and the same mean; one runs the fused call, the other the loop.  The header specifies the
call as that loop bit for bit, so EVERY comparison is exact (torch.equal): actions, observations [T, N, 6], rewards, done codes, every
step's best return and effective sample size / admission threshold, the final mean, the final state and counters, and compact_done().
The loops are given clamp=(-1, 1), the InvertedDoublePendulum's ctrlrange (their default is the InvertedPendulum's); the fused calls
take it as their own default.

datasets.collect: a continuous env needs `sigma` with a nominal (Engine._candidate_args) and planner="cem" needs n_elites, so the mpc
dicts of the two collect tests carry sigma=0.5 (and n_elites=8) beside horizon, n_candidates and temperature."""
import numpy as np
import pytest

import mpc_cem_reference as RC
import mpc_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = (1 << 40) + 12345  # of the plan's candidates: a plain 64-bit key
CLAMP = (-1.0, 1.0)
SWINGUP = "ReboundInvertedDoublePendulumSwingUp"
IDS = ("ReboundInvertedDoublePendulumBalancing", "BoundaryInvertedDoublePendulumBalancing", SWINGUP,
       "BoundaryInvertedDoublePendulumSwingUp")
PLANNERS = ("mppi", "cem")
AUX = {"mppi": "ess", "cem": "elite_return"}
KERNEL = {"mppi": 13, "cem": 14}  # EMEI_KERNEL_BODY_MPC_MPPI / EMEI_KERNEL_BODY_MPC_CEM
CEM = dict(n_elites=8, iterations=2, sigma_min=0.05)  # of the tests that do not sweep them


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


def _pair(name, N, **kw):
    return _engine(name, N, seed=7, **kw), _engine(name, N, seed=7, **kw)


def _state0(n, seed=11):
    """start rows (x, theta1, theta2, v, omega1, omega2) near the reset distribution (the swing-up envs hang: the offset is the model's)"""
    return np.random.default_rng(seed).uniform(-0.05, 0.05, (n, 6))


def _nominal0(eng, H, seed=5):
    return torch.as_tensor(np.random.default_rng(seed).uniform(-0.8, 0.8, (H, eng.n_envs)).astype(np.float32), device=eng.device)


def _start(engs, state, reset_seed=3):
    for e in engs:
        e.reset(reset_seed)  # the key of the device reset generator, episode counters to 0
        e.set_state(state)


def _snapshot(eng):
    steps, epi = eng.get_counters()
    return {"state": eng.get_state(), "steps": steps, "episode": epi, "compact_done": eng.compact_done()}


def _names(planner):
    return ("actions", "obs", "reward", "done", "plan_return", AUX[planner])


def _fused(eng, planner, T, H, K, seed, nom, cem=CEM, **kw):
    """the fused call -> the six results as a tuple (diagnostics on)"""
    if planner == "mppi":
        return eng.mpc_mppi(T, H, K, seed, 0.7, nom, sigma=0.5, diagnostics=True, **kw)
    return eng.mpc_cem(T, H, K, cem["n_elites"], seed, nom, iterations=cem["iterations"], sigma=0.5, sigma_min=cem["sigma_min"],
                       diagnostics=True, **kw)


def _loop(eng, planner, T, H, K, seed, nom, cem=CEM, **kw):
    if planner == "mppi":
        return R.mpc_loop(eng, T, H, K, seed, 0.7, nom, sigma=0.5, clamp=CLAMP, **kw)
    return RC.mpc_cem_loop(eng, T, H, K, cem["n_elites"], seed, nom, iterations=cem["iterations"], sigma=0.5, sigma_min=cem["sigma_min"],
                           clamp=CLAMP, **kw)


def _first_difference(planner, got, want):
    """the first differing quantity in the order that locates a fault (tests/test_gpu_mpc.py): the first step's plan, then the rest"""
    aux = AUX[planner]
    for key in ("plan_return", aux):
        if not torch.equal(got[key][0], want[key][0]):
            return f"{key}[0]: {got[key][0].tolist()} != {want[key][0].tolist()}"
    for key in ("nominal", "actions", "plan_return", aux, "obs", "reward", "done", "state", "steps", "episode", "compact_done"):
        if got[key].shape != want[key].shape or not torch.equal(got[key], want[key]):
            return f"{key}: {got[key].tolist()} != {want[key].tolist()}"
    return None


def _run_both(fused, loop, planner, T, H, K, state, seed=SEED, **kw):
    """the fused call on `fused`, the loop on `loop`, from the same rows and mean -> (fused results, loop results) as dicts"""
    _start((fused, loop), state)
    nom = _nominal0(fused, H)
    na, nb = nom.clone(), nom.clone()
    a = dict(zip(_names(planner), _fused(fused, planner, T, H, K, seed, na, **kw)))
    b = dict(zip(_names(planner), _loop(loop, planner, T, H, K, seed, nb, **kw)))
    a["nominal"], b["nominal"] = na, nb
    a.update(_snapshot(fused)), b.update(_snapshot(loop))
    assert fused.last_kernel() == KERNEL[planner]
    return a, b


def _assert_equal(planner, a, b, what):
    diff = _first_difference(planner, a, b)
    assert diff is None, f"{planner} {what}: {diff}"


# (K, H, T, n_elites as "one" / "mid" / "all", iterations).  K: fewer candidates than lanes, exactly one pass, three passes with a ragged
# last one.  H: a degenerate shift, component counts that are no multiple of a Philox block.  Every value of every column occurs.
COVER = ((1, 1, 1, "all", 1), (1, 9, 4, "one", 3), (5, 3, 4, "mid", 1), (5, 1, 1, "all", 3), (64, 9, 1, "mid", 3), (64, 3, 4, "one", 1),
         (64, 1, 4, "all", 1), (130, 1, 4, "mid", 3), (130, 9, 4, "all", 1), (130, 3, 1, "one", 3), (5, 9, 1, "one", 1))


def test_the_cover_covers():
    assert len(COVER) <= 12
    for col, values in enumerate(((1, 5, 64, 130), (1, 3, 9), (1, 4), ("one", "mid", "all"), (1, 3))):
        assert {c[col] for c in COVER} == set(values), col


# N = 3: the block's last wave has no env; N = 5: two blocks
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("planner", PLANNERS)
def test_shape_cover_equals_the_loop(planner, N):
    fused, loop = _pair(SWINGUP, N)
    state = _state0(N)
    for K, H, T, elites, iterations in COVER:
        cem = dict(n_elites={"one": 1, "mid": (K + 1) // 2, "all": K}[elites], iterations=iterations, sigma_min=0.05)
        a, b = _run_both(fused, loop, planner, T, H, K, state, cem=cem, discount=0.97)
        _assert_equal(planner, a, b, f"N={N} K={K} H={H} T={T} {cem}")
        assert a["actions"].dtype == torch.float32 and tuple(a["obs"].shape) == (T, N, 6)
        # the planner does something: a finite best return, actions inside the ctrlrange
        assert bool(torch.isfinite(a["plan_return"]).all()) and bool((a["actions"].abs() <= 1.0).all())


@pytest.mark.parametrize("name", IDS)
@pytest.mark.parametrize("planner", PLANNERS)
def test_all_four_ids_equal_the_loop(planner, name):
    fused, loop = _pair(name, 3)
    a, b = _run_both(fused, loop, planner, 4, 9, 70, _state0(3))
    _assert_equal(planner, a, b, name)


@pytest.mark.parametrize("kw", [dict(precision="f32"), dict(integrator="semi_implicit_euler"), dict(integrator="rk4"), dict(freq_rate=2)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("planner", PLANNERS)
def test_kernel_variants_equal_the_loop(planner, kw):
    fused, loop = _pair("BoundaryInvertedDoublePendulumSwingUp", 3, **kw)
    a, b = _run_both(fused, loop, planner, 4, 9, 70, _state0(3))
    _assert_equal(planner, a, b, str(kw))


def _threshold_rows():
    """x leaves (-3, 3) with the first step under any action (row 0); at step 3 under actions >= 0 and not within 9 steps under -1, so the
    candidates of one env end at different lengths (row 1); the zero row does not end within 9 steps in BoundarySwingUp, and at step 8
    under constant +-1 in BoundaryBalancing (row 2) — dt 0.02, euler, on the CPU oracle.  Rows 3 and 4 mirror rows 0 and 1."""
    s = np.zeros((5, 6))
    s[0, (0, 3)] = (2.99, 2.0)
    s[1, (0, 3)] = (2.90, 2.0)
    s[3, (0, 3)] = (-2.99, -2.0)
    s[4, (0, 3)] = (-2.90, -2.0)
    return s


@pytest.mark.parametrize("auto_reset,layout", [(True, "iid"), (False, "iid"), (True, "shared")])
@pytest.mark.parametrize("name", ["BoundaryInvertedDoublePendulumSwingUp", "BoundaryInvertedDoublePendulumBalancing"])
@pytest.mark.parametrize("planner", PLANNERS)
def test_terminations_and_resets_equal_the_loop(planner, name, auto_reset, layout):
    fused, loop = _pair(name, 5, init_noise=5e-3, noise_layout=layout)
    a, b = _run_both(fused, loop, planner, 7, 9, 70, _threshold_rows(), auto_reset=auto_reset)
    # not vacuous, on the loop's own outputs: an env ended with its first step, an env lived through the call
    done = b["done"].cpu().numpy()
    assert done[0, 0] == 1 and done.any(0).sum() < 5, done.tolist()
    epi = b["episode"].cpu().numpy()
    if auto_reset:
        assert np.array_equal(epi, (done != 0).sum(0)) and epi[0] >= 1
        # the reset state is the Body's base state (zero) plus the init noise: the noise was drawn
        idx = torch.as_tensor([0], device=loop.device)
        first = loop.episode_init_obs(idx, torch.as_tensor([1], device=loop.device))
        assert bool((first[:, 3:] != 0).all()), first.tolist()
    else:
        assert not epi.any() and b["steps"].tolist() == [7] * 5
    _assert_equal(planner, a, b, f"{name} auto_reset={auto_reset} {layout}")
    assert np.array_equal(a["compact_done"].cpu().numpy(), np.nonzero(done[-1])[0])


@pytest.mark.parametrize("planner", PLANNERS)
def test_time_limit_equals_the_loop(planner):
    fused, loop = _pair(SWINGUP, 3, max_episode_steps=3)
    a, b = _run_both(fused, loop, planner, 7, 5, 64, _state0(3), auto_reset=True, refill=0.25)
    _assert_equal(planner, a, b, "TimeLimit T=7")
    zero, trunc = [0] * 3, [2] * 3
    assert a["done"].tolist() == [zero, zero, trunc, zero, zero, trunc, zero]  # the truncated bit, nothing else
    assert a["steps"].tolist() == [1] * 3 and a["episode"].tolist() == [2] * 3
    # six steps end with the second truncation: a reset env's mean is `refill` everywhere
    a, b = _run_both(fused, loop, planner, 6, 5, 64, _state0(3), auto_reset=True, refill=0.25)
    _assert_equal(planner, a, b, "TimeLimit T=6")
    assert bool((a["nominal"] == 0.25).all()) and a["steps"].tolist() == [0] * 3 and a["episode"].tolist() == [2] * 3


@pytest.mark.parametrize("planner", PLANNERS)
def test_chunking(planner):
    """n_steps = 2 + 3 in one call equals a call with (2, seed) followed by one with (3, seed + 2) (CEM: seed + 2 * iterations)"""
    one, two = _pair("BoundaryInvertedDoublePendulumSwingUp", 5, init_noise=5e-3)
    H, K = 9, 70
    _start((one, two), _threshold_rows())
    na, nb = _nominal0(one, H), _nominal0(two, H)
    whole = _fused(one, planner, 5, H, K, SEED, na, auto_reset=True)
    first = _fused(two, planner, 2, H, K, SEED, nb, auto_reset=True)
    second = _fused(two, planner, 3, H, K, SEED + 2 * (CEM["iterations"] if planner == "cem" else 1), nb, auto_reset=True)
    for key, w, f, s in zip(_names(planner), whole, first, second):
        assert torch.equal(w, torch.cat([f, s])), key
    assert bool((whole[3] != 0).any()) and torch.equal(na, nb)
    sa, sb = _snapshot(one), _snapshot(two)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key


@pytest.mark.parametrize("planner", PLANNERS)
def test_shards(planner):
    """N = 6 in one engine equals engines of 2 and 4 envs with env_index_offset 0 and 2 (candidates and resets are keyed by the global index)"""
    name, H, K, T = "BoundaryInvertedDoublePendulumSwingUp", 9, 70, 4
    state = np.concatenate([_threshold_rows(), _state0(1)])
    big = _engine(name, 6, seed=7, init_noise=5e-3)
    _start((big,), state)
    nom = _nominal0(big, H)
    na = nom.clone()
    a = _fused(big, planner, T, H, K, SEED, na, auto_reset=True)
    assert bool((a[3] != 0).any(0).cpu().numpy()[[0, 3]].all())  # a reset on either side of the cut
    for lo, hi in ((0, 2), (2, 6)):
        part = _engine(name, hi - lo, seed=7, init_noise=5e-3, env_index_offset=lo)
        _start((part,), state[lo:hi])
        nb = nom[:, lo:hi].contiguous()
        b = _fused(part, planner, T, H, K, SEED, nb, auto_reset=True)
        for key, x, y in zip(_names(planner), a, b):
            assert torch.equal(x[:, lo:hi], y), (lo, key)
        assert torch.equal(na[:, lo:hi], nb) and torch.equal(big.get_state()[lo:hi], part.get_state())
        assert all(torch.equal(x[lo:hi], y) for x, y in zip(big.get_counters(), part.get_counters()))


@pytest.mark.parametrize("planner", PLANNERS)
def test_graph_capture(planner):
    """one call captured on a single stream; two replays equal two direct calls with the same arguments"""
    graphed, direct = _pair("BoundaryInvertedDoublePendulumSwingUp", 5, init_noise=5e-3)
    state, H, K, T = _threshold_rows(), 9, 70, 3
    _start((graphed, direct), state)
    nom = _nominal0(graphed, H)
    na, nb = nom.clone(), nom.clone()
    _fused(graphed, planner, T, H, K, SEED, na.clone(), auto_reset=True)  # allocates the workspace outside the capture
    _start((graphed,), state)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=graphed.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _fused(graphed, planner, T, H, K, SEED, na, auto_reset=True)
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        want = _fused(direct, planner, T, H, K, SEED, nb, auto_reset=True)
        for key, x, y in zip(_names(planner), out, want):
            assert torch.equal(x, y), (rep, key)
        assert torch.equal(na, nb), rep
    sa, sb = _snapshot(graphed), _snapshot(direct)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key


@pytest.mark.parametrize("planner", PLANNERS)
def test_refusals_and_neighbours(planner):
    noisy = _engine(SWINGUP, 2, obs_noise=1e-3)
    noisy.reset(0)
    nom = torch.zeros((4, 2), dtype=torch.float32, device=noisy.device)
    with pytest.raises(NotImplementedError, match=f"emei_mpc_{planner}: .*observation noise"):
        _fused(noisy, planner, 2, 4, 8, 1, nom)
    torch.cuda.synchronize()
    assert torch.equal(nom, torch.zeros_like(nom))  # a refused call writes nothing
    hop = _engine("HopperRunning", 2, freq_rate=4, real_time_scale=0.002)
    hop.reset(0)
    nom3 = torch.zeros((4, 2, 3), dtype=torch.float32, device=hop.device)
    with pytest.raises(NotImplementedError, match=f"emei_mpc_{planner}: .*body kernels"):
        _fused(hop, planner, 2, 4, 8, 1, nom3)


def test_env_method_numpy_in_numpy_out():
    import emei_amd

    env = emei_amd.make("ReboundInvertedDoublePendulumSwingUp-v0", num_envs=3)
    twin = emei_amd.make("ReboundInvertedDoublePendulumSwingUp-v0", num_envs=3)
    for e in (env, twin):
        e.reset(seed=4, options={"device_rng": True})
    nom = np.zeros((5, 3), np.float32)
    res = env.mpc_mppi(4, 5, 64, 9, 0.5, nom, sigma=0.5, diagnostics=True)
    assert len(res) == 8 and all(isinstance(x, np.ndarray) for x in res) and not nom.any()  # the caller's array is left alone
    act, obs, rew, term, trunc, pret, ess, nom_out = res
    assert act.shape == (4, 3) and obs.shape == (4, 3, 6) and term.dtype == np.bool_ and trunc.dtype == np.bool_ and nom_out.shape == (5, 3)
    assert np.abs(act).max() <= 1.0 and act.any()  # the default clamp is the ctrlrange
    t = torch.zeros((5, 3), dtype=torch.float32, device=twin.engine.device)
    tres = twin.mpc_mppi(4, 5, 64, 9, 0.5, t, sigma=0.5)
    assert len(tres) == 5 and np.array_equal(tres[0].cpu().numpy(), act) and np.array_equal(t.cpu().numpy(), nom_out)
    assert env.engine.last_kernel() == 13


@pytest.mark.parametrize("planner", PLANNERS)
def test_datasets_collect_with_an_mpc_controller(planner):
    """the zoo schema, the actions those of a direct call on a twin env"""
    import emei_amd
    from emei_amd import datasets

    N, T = 3, 6
    mpc = dict(horizon=5, n_candidates=64, sigma=0.5)
    mpc.update(dict(temperature=0.5) if planner == "mppi" else dict(planner="cem", n_elites=8))
    env = emei_amd.make("ReboundInvertedDoublePendulumSwingUp-v0", num_envs=N)
    data, info = datasets.collect(env, T, seed=3, mpc=mpc)
    assert set(data) == set(datasets.DATASET_KEYS) and all(len(v) == N * T for v in data.values())
    assert info["total_sample_num"] == N * T and tuple(data["observations"].shape) == (N * T, 6)
    obs, nxt, act = (data[k].reshape(N, T, -1) for k in ("observations", "next_observations", "actions"))
    assert torch.equal(obs[:, 1:], nxt[:, :-1])  # no episode ends in six steps of a swing-up: one continuous chain
    twin = emei_amd.make("ReboundInvertedDoublePendulumSwingUp-v0", num_envs=N)
    obs0, _ = twin.reset(seed=3, options={"device_rng": True})
    assert torch.equal(obs[:, 0], torch.as_tensor(obs0, device=obs.device).float())
    nominal = torch.zeros((5, N), dtype=torch.float32, device=twin.engine.device)
    if planner == "mppi":
        direct = twin.mpc_mppi(T, 5, 64, 3, 0.5, nominal, sigma=0.5, auto_reset=True)
    else:
        direct = twin.mpc_cem(T, 5, 64, 8, 3, nominal, sigma=0.5, auto_reset=True)
    assert torch.equal(act[..., 0], direct[0].T) and torch.equal(nxt, direct[1].transpose(0, 1))
    assert env.engine.last_kernel() == KERNEL[planner]
