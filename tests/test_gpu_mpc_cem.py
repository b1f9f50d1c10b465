"""emei_mpc_cem on the GPU (Engine.mpc_cem / HipEnv.mpc_cem / datasets.collect(mpc=dict(planner="cem", ...))).

The yardstick is the loop the call fuses, written against the API as it stood before (tests/mpc_cem_reference.py: plan_cem in place
with a per-entry std tensor, step, clamp, shift, refill).  Two engines of the same configuration start from the same state and the
same nominal; one runs the fused call, the other the loop.  The header specifies the call as that loop bit for bit, so EVERY
comparison here is exact (torch.equal / np.array_equal): actions, observations, rewards, done codes, every step's best return and
admission threshold, the final nominal, the final state and counters, and compact_done()."""
import numpy as np
import pytest

import mpc_cem_reference as R
from test_gpu_mpc import _nominal0, _snapshot, _start, _state0, _threshold_rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = (1 << 40) + 54321  # of the plan's candidates: a plain 64-bit key
NAMES = ("actions", "obs", "reward", "done", "plan_return", "elite_return")
IP = dict(sigma=0.5, sigma_min=0.05)  # the continuous envs' planner settings


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


def _pair(name, N, **kw):
    return _engine(name, N, seed=7, **kw), _engine(name, N, seed=7, **kw)


def _first_difference(got, want):
    """the first differing quantity in the order that locates a fault: the first step's plan, then the rest"""
    for key in ("plan_return", "elite_return"):
        if not torch.equal(got[key][0], want[key][0]):
            return f"{key}[0]: {got[key][0].tolist()} != {want[key][0].tolist()}"
    for key in ("nominal", "actions", "plan_return", "elite_return", "obs", "reward", "done", "state", "steps", "episode", "compact_done"):
        if got[key].shape != want[key].shape or not torch.equal(got[key], want[key]):
            return f"{key}: {got[key].tolist()} != {want[key].tolist()}"
    return None


def _run_both(fused, loop, T, H, K, n_elites, state, seed=SEED, nominal=None, **kw):
    """the fused call on `fused`, the loop on `loop`, from the same state and nominal -> (fused results, loop results) as dicts"""
    _start((fused, loop), state)
    nom = _nominal0(fused, H) if nominal is None else nominal
    na, nb = nom.clone(), nom.clone()
    a = dict(zip(NAMES, fused.mpc_cem(T, H, K, n_elites, seed, na, diagnostics=True, **kw)))
    b = dict(zip(NAMES, R.mpc_cem_loop(loop, T, H, K, n_elites, seed, nb, **kw)))
    a["nominal"], b["nominal"] = na, nb
    a.update(_snapshot(fused)), b.update(_snapshot(loop))
    return a, b


def _assert_equal(a, b, what):
    diff = _first_difference(a, b)
    assert diff is None, f"{what}: {diff}"


def _assert_sane(a):
    """not parity: the planner does something — every step's best return is finite and no threshold lies above it"""
    assert bool(torch.isfinite(a["plan_return"]).all()) and bool((a["elite_return"] <= a["plan_return"]).all())


# (K, n_elites, H, T, iterations): a covering set, not the product.  K: fewer candidates than lanes, exactly one pass, three passes
# with a ragged last one — each with one elite, a middle count and every candidate; H: a degenerate shift, component counts that
# are no multiple of a Philox block (4); T and iterations: one and several, in all four combinations.
COVER = ((1, 1, 1, 1, 1), (1, 1, 3, 4, 3), (1, 1, 9, 4, 1),
         (5, 1, 1, 4, 3), (5, 3, 3, 1, 1), (5, 5, 9, 1, 3),
         (64, 64, 1, 1, 3), (64, 1, 3, 4, 1), (64, 20, 9, 4, 3),
         (130, 7, 1, 4, 1), (130, 130, 3, 1, 3), (130, 1, 9, 4, 3))


# N = 3: the block's last wave has no env; N = 5: two blocks.
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("name,kw", [("CartPoleSwingUp", {}), ("ReboundInvertedPendulumSwingUp", IP)])
def test_shape_cover_equals_the_loop(name, kw, N):
    fused, loop = _pair(name, N)
    state = _state0(fused)
    for K, n_elites, H, T, iterations in COVER:
        a, b = _run_both(fused, loop, T, H, K, n_elites, state, iterations=iterations, discount=0.97, **kw)
        _assert_equal(a, b, f"{name} N={N} K={K} n_elites={n_elites} H={H} T={T} iterations={iterations}")
        _assert_sane(a)
        assert a["actions"].dtype == (torch.int64 if fused.act_dim == 0 else torch.float32)
        assert fused.last_kernel() == 12  # EMEI_KERNEL_PEND_MPC_CEM


def test_ties_at_the_threshold_go_to_the_lower_index():
    """CartPoleBalancing at discount 1: the returns are small integers (the steps survived), so the admission threshold falls inside
    a large tie and the lower-k rule decides who is a member"""
    fused, loop = _pair("CartPoleBalancing", 5)
    H, K, n_elites, state = 6, 130, 7, _threshold_rows()
    # the premise, from the first iteration's candidates on the host: some env's threshold return is shared by more candidates
    # than were admitted with it
    _start((fused,), state)
    nom = _nominal0(fused, H)
    cand = fused.sample_candidates(H, K, SEED, nominal=nom.clamp(0.05, 0.95))
    ret = fused.evaluate_sequences(cand, discount=1.0)[0].cpu().numpy()
    thr = np.sort(ret, axis=1)[:, ::-1][:, n_elites - 1]
    shared = (ret == thr[:, None]).sum(1)
    admitted = n_elites - (ret > thr[:, None]).sum(1)
    assert (shared > admitted).any(), (shared, admitted)
    a, b = _run_both(fused, loop, 4, H, K, n_elites, state, nominal=nom, iterations=3, discount=1.0)
    _assert_equal(a, b, "ties")
    _assert_sane(a)
    one = dict(zip(NAMES, _rerun(fused, state, 1, H, K, n_elites, nom, iterations=1, discount=1.0)))
    assert np.array_equal(one["elite_return"][0].cpu().numpy(), thr)  # the threshold the host found


def _rerun(eng, state, T, H, K, n_elites, nom, **kw):
    _start((eng,), state)
    return eng.mpc_cem(T, H, K, n_elites, SEED, nom.clone(), diagnostics=True, **kw)


@pytest.mark.parametrize("sigma_min", [0.0, 0.05])
def test_collapse_and_floor(sigma_min):
    """one elite: the std is exactly 0 after the first refit, so with no floor every later draw is the clipped mean; with a floor
    the std is exactly the floor"""
    fused, loop = _pair("ReboundInvertedPendulumSwingUp", 3)
    H, K, state = 5, 70, _state0(fused)
    # the premise: plan_cem with one elite returns std == 0 exactly
    _start((loop,), state)
    nom = _nominal0(loop, H)
    std = loop.plan_cem(H, K, 1, SEED, nominal=nom.clone(), sigma=torch.full_like(nom, 0.5))[1]
    assert bool((std == 0).all())
    a, b = _run_both(fused, loop, 4, H, K, 1, state, nominal=nom, iterations=3, sigma=0.5, sigma_min=sigma_min)
    _assert_equal(a, b, f"sigma_min={sigma_min}")
    _assert_sane(a)


@pytest.mark.parametrize("name,pk,kw", [
    ("CartPoleSwingUp", {}, dict(precision="f32")),
    ("ReboundInvertedPendulumSwingUp", IP, dict(precision="f32")),
    ("CartPoleSwingUp", {}, dict(ode_method="rk4")),
    ("CartPoleSwingUp", {}, dict(freq_rate=2)),
    ("BoundaryInvertedPendulumBalancing", IP, dict(freq_rate=2)),
])
def test_other_kernel_variants_equal_the_loop(name, pk, kw):
    fused, loop = _pair(name, 3, **kw)
    a, b = _run_both(fused, loop, 4, 9, 70, 9, _state0(fused), iterations=2, **pk)
    _assert_equal(a, b, f"{name} {kw}")
    _assert_sane(a)


@pytest.mark.parametrize("auto_reset", [True, False])
def test_termination_and_reset_equal_the_loop(auto_reset):
    fused, loop = _pair("CartPoleBalancing", 5)
    a, b = _run_both(fused, loop, 7, 6, 70, 9, _threshold_rows(), iterations=2, auto_reset=auto_reset)
    _assert_equal(a, b, f"auto_reset={auto_reset}")
    done = a["done"].cpu().numpy()
    assert np.array_equal(done[0, :2], [1, 1]) and done[:3, 2].any() and done[:3, 3].any()  # terminal within three steps
    assert np.array_equal(a["compact_done"].cpu().numpy(), np.nonzero(done[-1])[0])
    epi = a["episode"].cpu().numpy()
    if auto_reset:
        assert np.array_equal(epi, (done != 0).sum(0)) and epi[0] >= 1
    else:
        assert not epi.any() and np.array_equal(a["steps"].cpu().numpy(), [7] * 5)
        assert done[-1, 0] == 1 and done[-1, 1] == 1  # past the rail at x_dot = 2 they stay terminal


def test_a_reset_env_gets_no_warm_start():
    """one step that ends env 0's and env 1's episodes: their mean columns are `refill` everywhere and their episode counters
    advanced; the surviving envs' columns are the shifted plan with `refill` behind it"""
    fused, loop = _pair("CartPoleBalancing", 5)
    a, b = _run_both(fused, loop, 1, 6, 70, 9, _threshold_rows(), iterations=2, auto_reset=True, refill=0.25)
    _assert_equal(a, b, "one step")
    nom = a["nominal"].cpu().numpy()
    assert a["done"][0].tolist() == [1, 1, 0, 0, 0] and a["episode"].tolist() == [1, 1, 0, 0, 0]
    assert np.all(nom[:, :2] == np.float32(0.25)) and np.all(nom[-1] == np.float32(0.25))
    assert not np.all(nom[:-1, 2:] == np.float32(0.25))  # the others keep their plans


def test_time_limit_equals_the_loop():
    fused, loop = _pair("CartPoleSwingUp", 3, max_episode_steps=4)
    a, b = _run_both(fused, loop, 7, 5, 64, 8, _state0(fused), iterations=2, auto_reset=True)
    _assert_equal(a, b, "TimeLimit")
    assert a["done"].tolist() == [[0] * 3] * 3 + [[2] * 3] + [[0] * 3] * 3  # truncated at step 4, nothing else
    assert a["steps"].tolist() == [3] * 3 and a["episode"].tolist() == [1] * 3


CEM = dict(iterations=3, auto_reset=True, diagnostics=True)  # of the three tests below; seeds advance by iterations per step


def test_chunking():
    """n_steps = 3 + 4 in one call equals a call with (3, seed) followed by one with (4, seed + 3 * iterations)"""
    one, two = _pair("CartPoleBalancing", 5)
    state, H, K, E = _threshold_rows(), 6, 70, 9
    _start((one, two), state)
    na, nb = _nominal0(one, H), _nominal0(two, H)
    whole = one.mpc_cem(7, H, K, E, SEED, na, **CEM)
    first = two.mpc_cem(3, H, K, E, SEED, nb, **CEM)
    second = two.mpc_cem(4, H, K, E, SEED + 3 * CEM["iterations"], nb, **CEM)
    for key, w, f, s in zip(NAMES, whole, first, second):
        assert torch.equal(w, torch.cat([f, s])), key
    assert torch.equal(na, nb)
    sa, sb = _snapshot(one), _snapshot(two)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key


def test_sharding():
    """envs 1..2 of a 3-env engine equal a 2-env engine with env_index_offset = 1 (candidates and resets are keyed by the global index)"""
    big = _engine("CartPoleBalancing", 3, seed=7)
    part = _engine("CartPoleBalancing", 2, seed=7, env_index_offset=1)
    state, H, K, E = _threshold_rows()[[4, 0, 3]], 6, 70, 9
    _start((big,), state)
    _start((part,), state[1:])
    nom = _nominal0(big, H)
    na, nb = nom.clone(), nom[:, 1:].contiguous()
    a = big.mpc_cem(7, H, K, E, SEED, na, **CEM)
    b = part.mpc_cem(7, H, K, E, SEED, nb, **CEM)
    for key, x, y in zip(NAMES, a, b):
        assert torch.equal(x[:, 1:], y), key
    assert bool((a[3][:, 1:] != 0).any())  # a reset happened in the compared envs
    assert torch.equal(na[:, 1:], nb) and torch.equal(big.get_state()[1:], part.get_state())
    assert all(torch.equal(x[1:], y) for x, y in zip(big.get_counters(), part.get_counters()))


def test_graph_capture():
    """one call captured on a side stream; two replays equal two direct calls with the same arguments"""
    graphed, direct = _pair("ReboundInvertedPendulumSwingUp", 3)
    state, H, K, E, T = _state0(graphed), 6, 70, 9, 3
    _start((graphed, direct), state)
    nom = _nominal0(graphed, H)
    na, nb = nom.clone(), nom.clone()
    graphed.mpc_cem(T, H, K, E, SEED, na.clone(), **IP, **CEM)  # allocates the workspace outside the capture
    _start((graphed,), state)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=graphed.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = graphed.mpc_cem(T, H, K, E, SEED, na, **IP, **CEM)
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        want = direct.mpc_cem(T, H, K, E, SEED, nb, **IP, **CEM)
        for key, x, y in zip(NAMES, out, want):
            assert torch.equal(x, y), (rep, key)
        assert torch.equal(na, nb), rep
    sa, sb = _snapshot(graphed), _snapshot(direct)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key


def test_handle_dependent_refusals():
    hop = _engine("HopperRunning", 2, freq_rate=4, real_time_scale=0.002)
    hop.reset(0)
    nom3 = torch.zeros((4, 2, 3), dtype=torch.float32, device=hop.device)
    with pytest.raises(NotImplementedError, match="emei_mpc_cem: .*body kernels"):
        hop.mpc_cem(2, 4, 8, 2, 1, nom3, sigma=0.3)
    ip = _engine("ReboundInvertedPendulumSwingUp", 2, integrator="rk4")
    ip.reset(0)
    nom = torch.zeros((4, 2), dtype=torch.float32, device=ip.device)
    with pytest.raises(NotImplementedError, match="emei_mpc_cem: .*body kernels"):
        ip.mpc_cem(2, 4, 8, 2, 1, nom, sigma=0.3)
    fresh = _engine("CartPoleSwingUp", 2)
    half = torch.full((4, 2), 0.5, dtype=torch.float32, device=fresh.device)
    with pytest.raises(AssertionError, match="emei_mpc_cem"):
        fresh.mpc_cem(2, 4, 8, 2, 1, half)
    with pytest.raises(ValueError, match="EMEI_MPC_MAX_HORIZON"):
        fresh.mpc_cem(2, 257, 8, 2, 1, torch.full((257, 2), 0.5, dtype=torch.float32, device=fresh.device))
    with pytest.raises(ValueError, match="n_elites"):
        fresh.mpc_cem(2, 4, 8, 9, 1, half)
    plain = _engine("ReboundInvertedPendulumSwingUp", 2)
    plain.reset(0)
    state = plain.get_state().clone()
    pnom = torch.zeros((4, 2), dtype=torch.float32, device=plain.device)
    with pytest.raises(ValueError, match="sigma"):
        plain.mpc_cem(2, 4, 8, 2, 1, pnom)  # sigma=None on a continuous env
    with pytest.raises(ValueError, match="sigma_min"):
        plain.mpc_cem(2, 4, 8, 2, 1, pnom, sigma=0.3, sigma_min=-1.0)
    # a refused call writes nothing
    assert torch.equal(nom, torch.zeros_like(nom)) and torch.equal(pnom, torch.zeros_like(pnom))
    assert torch.equal(half, torch.full_like(half, 0.5)) and torch.equal(plain.get_state(), state)


def test_env_method_numpy_in_numpy_out():
    import emei_amd

    env = emei_amd.make("ReboundInvertedPendulumSwingUp-v0", num_envs=3)
    twin = emei_amd.make("ReboundInvertedPendulumSwingUp-v0", num_envs=3)
    for e in (env, twin):
        e.reset(seed=4, options={"device_rng": True})
    nom = np.zeros((5, 3), np.float32)
    res = env.mpc_cem(4, 5, 64, 8, 9, nom, iterations=2, diagnostics=True, **IP)
    assert len(res) == 8 and all(isinstance(x, np.ndarray) for x in res) and not nom.any()  # the caller's array is left alone
    act, obs, rew, term, trunc, pret, eret, nom_out = res
    assert act.shape == (4, 3) and obs.shape == (4, 3, 4) and term.dtype == np.bool_ and trunc.dtype == np.bool_ and nom_out.shape == (5, 3)
    assert pret.shape == (4, 3) and np.all(eret <= pret)
    t = torch.zeros((5, 3), dtype=torch.float32, device=twin.engine.device)
    tres = twin.mpc_cem(4, 5, 64, 8, 9, t, iterations=2, **IP)
    assert len(tres) == 5 and np.array_equal(tres[0].cpu().numpy(), act) and np.array_equal(t.cpu().numpy(), nom_out)


def test_datasets_collect_with_a_cem_controller():
    """every row a true transition, the rows after a done the device reset's observation, the actions those of a direct call.
    freq_rate = 2 and a mean pinned near "always push right" end an episode every few steps."""
    import emei_amd
    from emei_amd import datasets

    N, T = 3, 12
    mpc = dict(planner="cem", horizon=4, n_candidates=70, n_elites=9, iterations=2, clamp=(0.9, 0.95), refill=0.9)
    env = emei_amd.make("CartPoleBalancing-v0", num_envs=N, freq_rate=2)
    data, info = datasets.collect(env, T, seed=3, mpc=mpc)
    assert env.engine.last_kernel() == 12
    assert set(data) == set(datasets.DATASET_KEYS) and all(len(v) == N * T for v in data.values())
    obs, nxt, act, done = (data[k].reshape(N, T, -1) for k in ("observations", "next_observations", "actions", "dones"))
    done = done[..., 0] != 0
    assert info["total_episode_num"] == int(done.sum()) >= 1 and not bool(done.all())
    cont = ~done[:, :-1]
    assert torch.equal(obs[:, 1:][cont], nxt[:, :-1][cont])  # inside an episode the chain is continuous
    e, t = torch.nonzero(done[:, :-1], as_tuple=True)
    assert len(e) >= 1  # some row follows a done
    epi = torch.cumsum(done.to(torch.int64), dim=1)
    assert torch.equal(obs[e, t + 1], env.engine.episode_init_obs(e, epi[e, t]))  # after a done: the next episode's first observation
    twin = emei_amd.make("CartPoleBalancing-v0", num_envs=N, freq_rate=2)
    obs0, _ = twin.reset(seed=3, options={"device_rng": True})
    assert torch.equal(obs[:, 0], torch.as_tensor(obs0, device=obs.device).float())
    nominal = torch.full((4, N), 0.9, dtype=torch.float32, device=twin.engine.device)
    direct = twin.mpc_cem(T, 4, 70, 9, 3, nominal, iterations=2, clamp=(0.9, 0.95), refill=0.9, auto_reset=True)
    assert torch.equal(act[..., 0], direct[0].T)
    assert torch.equal(nxt, direct[1].transpose(0, 1)) and torch.equal(done, (direct[3] | direct[4]).T)
