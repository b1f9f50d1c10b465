"""HalfCheetah-style kernels against the oracle: two independent formulations of the same planar
9-DoF model (oracle: recursive Newton-Euler in joint coordinates + dense LDL; kernel: absolute-angle
closed forms + fill-free sparse LDL).  Parity with libmujoco is unpinned."""
import numpy as np
import pytest

from conftest import rel_err
from start_states import cheetah_states as _states

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


@pytest.mark.parametrize("fr,dt", [(1, 0.002), (4, 0.002), (2, 0.01)])
@pytest.mark.parametrize("precision", ["ref", "f32"])
@pytest.mark.parametrize("solver", ["newton", "sweep1"])
def test_onestep_vs_oracle(fr, dt, precision, solver):
    """both constraint solvers: MuJoCo's formulation solved to convergence (kernel: unit-step Newton on the active set;
    oracle: Newton with exact line search — the same unique minimiser) and round 1's single Gauss-Seidel sweep"""
    from oracle import oracle as O

    rng = np.random.default_rng(3)
    n = 1000  # ragged last wave
    s0 = _states(rng, n)
    act = rng.uniform(-1.3, 1.3, (n, 6)).astype(np.float32)
    eng = _engine("HalfCheetahRunning", n, freq_rate=fr, real_time_scale=dt, precision=precision, solver=solver)
    eng.set_state(s0)
    obs, rew, done = eng.step(torch.as_tensor(act, device=eng.device))
    o_st, o_rew, o_term = O.cheetah_step(s0, act.astype(np.float64), fr, dt, O.opts(solver=solver))
    if precision == "ref":
        assert rel_err(eng.get_state().cpu().numpy(), o_st, floor=1.0) <= 1e-9
        assert rel_err(obs.cpu().numpy(), o_st) <= 1e-5
        assert rel_err(rew.cpu().numpy(), o_rew) <= 1e-5
    else:
        assert rel_err(obs.cpu().numpy(), o_st) <= 5e-3  # float32: stiff contact terms amplify rounding
    assert np.array_equal((done.cpu().numpy() & 1).astype(bool), o_term) and not o_term.any()


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_lanes_with_three_row_blocks_vs_oracle(integrator):
    """Round 4: a lane with exactly three row blocks (contact points / violated limits) iterates in constraint space too, its
    third block in the unused second slot of a wave-mate (cheetah_model.h: `donor`); four and more keep the primal loop.  States
    are drawn until the oracle's row mask says a few hundred lanes have exactly 3 blocks, 4+ blocks, 2 and fewer — mixed inside
    the same waves, so that donors are taken and some three-block lanes find none; all against the oracle to 1e-9."""
    from oracle import oracle as O

    rng = np.random.default_rng(31)
    pool = _states(rng, 60000)
    pool[:, 1] = rng.uniform(-0.45, 0.1, len(pool))  # lower: more points on the floor
    nb = np.array([bin(int(m)).count("1") for m in O.planar_row_mask("cheetah", pool)])
    pick = np.concatenate([np.nonzero(nb == 3)[0][:700], np.nonzero(nb >= 4)[0][:200], np.nonzero(nb <= 2)[0][:636]])
    assert (nb[pick] == 3).sum() >= 300 and (nb[pick] >= 4).sum() >= 50
    pick = rng.permutation(pick)
    s0 = pool[pick]
    # one wave made of three-block lanes only: no donor there (the primal fallback), another with a single donor
    s0[:64] = pool[np.nonzero(nb == 3)[0][:64]]
    s0[64:127] = pool[np.nonzero(nb == 3)[0][64:127]]
    act = rng.uniform(-1.2, 1.2, (len(s0), 6)).astype(np.float32)
    eng = _engine("HalfCheetahRunning", len(s0), freq_rate=2, real_time_scale=0.002, integrator=integrator)
    eng.set_state(s0)
    eng.step(torch.as_tensor(act, device=eng.device))
    want, _, _ = O.cheetah_step(s0, act.astype(np.float64), 2, 0.002, O.opts(integrator))
    assert rel_err(eng.get_state().cpu().numpy(), want, floor=1.0) <= 1e-9
    assert eng.solver_cap_hits() == 0


def test_three_block_lane_alone_and_among_three_block_wave_mates():
    """ADVICE r04 / DESIGN "Determinism": a three-block cheetah lane borrows a constraint slot from a wave-mate with at most one
    row block and otherwise runs the primal loop — the ONE place where a lane's bits depend on who shares its wave.  Pinned here:
    the same env stepped as an n = 1 engine (63 parked padding lanes = 63 lenders: the constraint-space solver) and inside a wave
    made of three-block lanes only (no lender: the primal loop) agrees to 1e-11 per step (the two solvers converge to the same
    minimiser; measured 2e-13), and bit for bit wherever the lane finds a lender (the same env in a wave of free-flight lanes).
    Sharded-versus-unsharded bit equality therefore needs shard sizes that are multiples of 64 (same wave composition), which is
    what sharding.py's contiguous blocks of BASELINE's sizes are."""
    from oracle import oracle as O

    rng = np.random.default_rng(77)
    pool = _states(rng, 40000)
    pool[:, 1] = rng.uniform(-0.45, 0.1, len(pool))
    nb = np.array([bin(int(m)).count("1") for m in O.planar_row_mask("cheetah", pool)])
    tri = pool[np.nonzero(nb == 3)[0][:64]]
    assert len(tri) == 64
    air = _states(rng, 63)
    air[:, 1], air[:, 3:9] = 1.0, rng.uniform(-0.2, 0.2, (63, 6))  # high above the floor, joints inside their ranges: no row
    assert not O.planar_row_mask("cheetah", air).any()
    act = rng.uniform(-1.0, 1.0, (64, 6)).astype(np.float32)
    kw = dict(freq_rate=1, real_time_scale=0.002)
    dense = _engine("HalfCheetahRunning", 64, **kw)  # a wave of three-block lanes: nobody lends
    dense.set_state(tri)
    dense.step(torch.as_tensor(act, device=dense.device))
    got_dense = dense.get_state().cpu().numpy()
    worst = 0.0
    for k in (0, 17, 63):
        alone = _engine("HalfCheetahRunning", 1, **kw)  # the padding lanes of its wave are parked in the air: lenders
        alone.set_state(tri[k : k + 1])
        alone.step(torch.as_tensor(act[k : k + 1], device=alone.device))
        got_alone = alone.get_state().cpu().numpy()[0]
        worst = max(worst, rel_err(got_dense[k], got_alone, floor=1.0))
        mixed = _engine("HalfCheetahRunning", 64, **kw)  # the same env at the same lane among free-flight lanes: lenders again
        st = np.concatenate([air[:k], tri[k : k + 1], air[k:]])
        a2 = np.concatenate([act[:k], act[k : k + 1], act[k + 1 :]])
        mixed.set_state(st)
        mixed.step(torch.as_tensor(a2, device=mixed.device))
        assert np.array_equal(mixed.get_state().cpu().numpy()[k], got_alone)  # same solver: the same bits
    assert worst <= 1e-11, worst
    assert dense.solver_cap_hits() == 0


def test_rollout_segments_vs_oracle_and_step_equivalence():
    from oracle import oracle as O

    rng = np.random.default_rng(4)
    n, T = 128, 60
    acts = rng.uniform(-1, 1, (T, n, 6)).astype(np.float32)
    a = _engine("HalfCheetahRunning", n, freq_rate=4, real_time_scale=0.002, init_noise=0.1, seed=5)
    b = _engine("HalfCheetahRunning", n, freq_rate=4, real_time_scale=0.002, init_noise=0.1, seed=5)
    a.reset(5)
    b.reset(5)
    dev = torch.as_tensor(acts, device=a.device)
    for t0 in range(0, T, 20):  # re-synchronise the oracle every 20 steps (80 substeps): chaotic contacts
        st = a.get_state().cpu().numpy()
        obs, rew, done = a.rollout(dev[t0 : t0 + 20].contiguous())
        for t in range(20):
            o, r, d = b.step(dev[t0 + t])
            assert torch.equal(o, obs[t]) and torch.equal(r, rew[t]) and torch.equal(d, done[t])
            st, o_rew, _ = O.cheetah_step(st, acts[t0 + t].astype(np.float64))
            assert rel_err(obs[t].cpu().numpy(), st) <= 1e-5, (t0, t)
            assert rel_err(rew[t].cpu().numpy(), o_rew) <= 1e-4, (t0, t)
    assert torch.equal(a.get_state(), b.get_state())


def test_reference_behaviour_and_env_api(mujoco_golden):
    """test_half_cheetah.py:6-13 of the reference: obs.shape == (18,) after reset and after one step."""
    import emei_amd
    from emei_amd import engine as E

    env = emei_amd.HalfCheetahRunningEnv()
    np.random.seed(0)
    obs, _ = env.reset()
    assert obs.shape == (18,)
    obs, reward, terminal, truncated, info = env.step(env.action_space.sample())
    assert obs.shape == (18,) and not terminal and np.isfinite(reward)
    g = mujoco_golden
    o, po, ac = g["cheetah_obs"], g["cheetah_pre_obs"], g["cheetah_action"]
    r = env.get_batch_reward(o, po, ac)  # float64 rows in, float64 arithmetic on them (half_cheetah.py:59-63)
    assert r.dtype == np.float64 and rel_err(r[:, 0], g["cheetah_reward_B1"]) <= 1e-5  # every row (NaN rows: NaN on both sides)
    t = env.get_batch_terminal(o)
    assert np.array_equal(t, g["cheetah_terminal"])
    # what the reference EXECUTES for B > 1: np.sum(np.square(action)) has no axis, the control cost of the whole batch is
    # charged to every row (half_cheetah.py:61) — opt-in, per call or per env
    rq = env.get_batch_reward(o, po, ac, reference_batch_semantics=True)
    assert rel_err(rq, g["cheetah_reward_batchquirk"]) <= 1e-5
    env.reference_batch_semantics = True
    assert np.array_equal(env.get_batch_reward(o, po, ac), rq)
    assert rel_err(env.get_batch_reward(o[:1], po[:1], ac[:1])[:, 0], g["cheetah_reward_B1"][:1]) <= 1e-5  # B = 1: the same thing
    env.reference_batch_semantics = False
    t32 = E.batch_terminal("HalfCheetahRunning", torch.as_tensor(o, dtype=torch.float32, device="cuda")).cpu().numpy()
    assert np.array_equal(t32, g["cheetah_terminal"][:, 0])


def test_full_size_config4_properties():
    """BASELINE configs[3]: 131 072 envs, freq 4: rollout == chunked rollouts; device reset spec; finite."""
    from oracle import oracle as O

    N, T = 131072, 8
    acts = (torch.rand((T, N, 6), device="cuda") * 2 - 1).float()
    a = _engine("HalfCheetahRunning", N, freq_rate=4, real_time_scale=0.002, init_noise=0.1, max_episode_steps=1000, seed=2)
    a.reset(2)
    s0 = a.get_state()[:4].cpu().numpy()
    assert float(a.get_state().std()) == pytest.approx(0.1, rel=0.02)
    obs, rew, done = a.rollout(acts, auto_reset=True)
    b = _engine("HalfCheetahRunning", N, freq_rate=4, real_time_scale=0.002, init_noise=0.1, max_episode_steps=1000, seed=2)
    b.reset(2)
    p = [b.rollout(acts[k : k + 4].contiguous(), auto_reset=True) for k in (0, 4)]
    assert torch.equal(torch.cat([p[0][0], p[1][0]]), obs) and torch.equal(torch.cat([p[0][1], p[1][1]]), rew)
    assert bool(torch.isfinite(obs).all()) and not bool(done.any())
    st = s0
    for t in range(T):
        st, _, _ = O.cheetah_step(st, acts[t, :4].cpu().numpy().astype(np.float64))
    assert rel_err(obs[-1, :4].cpu().numpy(), st) <= 1e-5
