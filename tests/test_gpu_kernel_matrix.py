"""Every compiled configuration (tests/kernel_matrix.py) through one step against the CPU oracle, then through every fused entry point
against its composition on a second engine of the SAME configuration.
Size: 64 rows (16 four-state units, 24 body units x {RK4 false, true}) x 16 entry points = 1024 pairs. 916 are supported. 108 are
kernel_matrix.UNSUPPORTED and are tests too: 80 refuse (mpc_mppi / mpc_cem on the 32 body rows other than the
InvertedDoublePendulum, batch_next_obs on its 16 rows), 20 accept and ignore the option (the chunked rollout on the 16 four-state
units and on the 4 single-sweep Hopper rows, whose rollout blocks are not one wave), and 8 cannot be reached (batch_next_obs has no
solver argument, so the single-sweep units' next-obs kernels are compiled and never launched: the call runs the Newton sibling's
step, which is what the test pins). Layer 1 adds 16 semi-implicit rows (a runtime flag of the non-RK4 body kernels): 80 one-step
cases.
Layer 1 (N = 130: two waves and a ragged one of 2 lanes; freq_rate 2; one step). precision="ref": state and get_obs 1e-9 with an
absolute floor of 1, float32 observation 1e-5, reward 1e-5 (2e-5 on the body kernels, tests/test_gpu_integrators.py), terminal bits
equal on the decidable rows (at most 1 % are not: tests/test_kernel_matrix.py), no Newton solve at its cap. precision="f32": the
tolerance and floor of the family's own float32 one-step test (Row.f32_bound), and the terminal bits wherever the oracle's flag does
not change within that tolerance of its observation (at most 2 % of the rows do). The Hopper's rows are those of its float32 test
(its draw without the stiff rows, index % 5 >= 2) and EVERY capsule-pair row that kernel_matrix appends, the ragged wave included; a
row is left out only where the float64 oracle itself moves by more than the bound under a 1e-5 relative change of the start state
(Row.ill_conditioned: a constraint row switching inside the step), and the seed is chosen so that at most 1 % of the rows do, which
tests/test_kernel_matrix.py asserts. The bounds are the project's, not derived; the measured maxima of this file (MEASURED lines,
MI355X) against them, on the asserted rows and on all 130:

    row            asserted   rows  bound (floor)   what          all 130 rows
    ip0_f32-euler  6.981e-06   130  2e-04 (1    )  obs+reward    6.981e-06
    ip1_f32-euler  6.981e-06   130  2e-04 (1    )  obs+reward    6.981e-06
    ip2_f32-euler  1.513e-06   130  2e-04 (1    )  obs+reward    1.513e-06
    ip3_f32-euler  1.513e-06   130  2e-04 (1    )  obs+reward    1.513e-06
    cp0_f32-euler  1.716e-07   130  1e-04 (1    )  obs+reward    1.716e-07
    cr0_f32-rk4    1.756e-07   130  1e-04 (1    )  obs           1.756e-07
    cp1_f32-euler  1.176e-07   130  1e-04 (1    )  obs+reward    1.176e-07
    cr1_f32-rk4    1.212e-07   130  1e-04 (1    )  obs           1.212e-07
    ip0_f32-semi   6.645e-06   130  2e-04 (1    )  obs+reward    6.645e-06
    ip1_f32-semi   6.645e-06   130  2e-04 (1    )  obs+reward    6.645e-06
    ip2_f32-semi   2.283e-06   130  2e-04 (1    )  obs+reward    2.283e-06
    ip3_f32-semi   2.283e-06   130  2e-04 (1    )  obs+reward    2.283e-06
    dp0_f32-euler  1.325e-05   130  2e-03 (0.001)  obs           1.325e-05
    dp1_f32-euler  1.325e-05   130  2e-03 (0.001)  obs           1.325e-05
    dp2_f32-euler  8.592e-05   130  2e-03 (0.001)  obs           8.592e-05
    dp3_f32-euler  8.592e-05   130  2e-03 (0.001)  obs           8.592e-05
    ch_f32-euler   4.482e-05   130  5e-03 (0.001)  obs           4.482e-05
    chs_f32-euler  3.825e-05   130  5e-03 (0.001)  obs           3.825e-05
    hp_f32-euler   3.650e-05    90  5e-03 (0.001)  obs           3.650e-05
    hps_f32-euler  1.479e-04    90  5e-03 (0.001)  obs           1.479e-04
    ip0_f32-rk4    2.888e-06   130  2e-04 (1    )  obs+reward    2.888e-06
    ip1_f32-rk4    2.888e-06   130  2e-04 (1    )  obs+reward    2.888e-06
    ip2_f32-rk4    4.830e-06   130  2e-04 (1    )  obs+reward    4.830e-06
    ip3_f32-rk4    4.830e-06   130  2e-04 (1    )  obs+reward    4.830e-06
    dp0_f32-rk4    9.443e-04   130  2e-03 (0.001)  obs           9.443e-04
    dp1_f32-rk4    9.443e-04   130  2e-03 (0.001)  obs           9.443e-04
    dp2_f32-rk4    2.150e-04   130  2e-03 (0.001)  obs           2.150e-04
    dp3_f32-rk4    2.150e-04   130  2e-03 (0.001)  obs           2.150e-04
    ch_f32-rk4     8.933e-05   130  5e-03 (0.001)  obs           8.933e-05
    chs_f32-rk4    6.925e-05   130  5e-03 (0.001)  obs           6.925e-05
    hp_f32-rk4     1.437e-04    90  5e-03 (0.001)  obs           1.437e-04
    hps_f32-rk4    2.304e-04    90  5e-03 (0.001)  obs           2.304e-04
    dp0_f32-semi   4.511e-05   130  2e-03 (0.001)  obs           4.511e-05
    dp1_f32-semi   4.511e-05   130  2e-03 (0.001)  obs           4.511e-05
    dp2_f32-semi   9.433e-05   130  2e-03 (0.001)  obs           9.433e-05
    dp3_f32-semi   9.433e-05   130  2e-03 (0.001)  obs           9.433e-05
    ch_f32-semi    1.527e-04   130  5e-03 (0.001)  obs           1.527e-04
    chs_f32-semi   9.757e-05   130  5e-03 (0.001)  obs           9.757e-05
    hp_f32-semi    4.880e-05    90  5e-03 (0.001)  obs           4.880e-05
    hps_f32-semi   1.942e-04    90  5e-03 (0.001)  obs           1.942e-04

Every float32 row stays inside its family's bound; the semi-implicit and RK4 rows, which nobody had measured, are no worse than an
order of magnitude above their Euler siblings (the InvertedDoublePendulum's RK4 rows come closest: 9.4e-4 against 2e-3). With the
Hopper's first draw (seed 0) the single-sweep float32 RK4 row reached 7.9e-2 on one capsule-pair row (row 128, coordinate 11); the
oracle moves that coordinate by as much under a 1e-5 relative change of the state, which is what Row.ill_conditioned now detects and
the seed avoids.
Layer 2 (N = 70: a full wave and 6 lanes; K = 5 candidates, so N * K = 350 straddles waves and ends ragged; H = T = 6; rollout-type
calls with max_episode_steps = 4 and auto_reset, so every env crosses a device reset inside the call; env_index_offset 2^32 + 7 and
seeds above 2^32, so the reset and noise streams see high key words). The reference runs in the row's own precision, so the
comparison is bit for bit; the HalfCheetah takes the project's lane-lending exception (1e-9 relative on returns
and observations, between lanes with the same wave-mates: the population's replay runs member by member there). plan_mppi and
plan_cem are held to their definition by the helpers of tests/test_gpu_mppi.py and tests/test_gpu_cem.py, with the bounds derived
there; plan_policy's weighted mean and effective sample size to the header's weights and summation tree
(tests/test_gpu_policy_plan.py), bit for bit. The rollout at these shapes takes the generic four-state kernel (a ragged N); the
staged kernel is the subject of tests/test_gpu_shapes.py and the bench tests.
Mutation check (a local edit, never committed): in DPendBody::accel (dpend_model.h) the cart force was scaled by 1.001 under `if
constexpr (VARIANT == 2)` for the evaluations that the RK4 stages make (they pass hd = 0; the model has no branch of its own there,
so the edit stands in for one wrong instantiation), and the library rebuilt. Of this file's 280 InvertedDoublePendulum cases exactly
two failed, test_layer1_one_step_vs_oracle[dp2_f64-rk4] and [dp2_f32-rk4]; the 278 others passed (layer 2 compares a configuration
with itself, so it cannot see a consistent error: that is layer 1's job, which is why it runs first), and tests/test_gpu_dpend.py
plus tests/test_gpu_integrators.py passed on the same library (76 passed): the RK4 ReboundSwingUp instantiation was held to the
oracle by nothing before.
Wall time on an MI355X: about 9 s for this file's 1104 cases, and 292 s for the whole GPU suite with it (2686 passed). The suite was
not timed on the parent commit; 292 s less this file's share, about 283 s, is an inference.
"""
import types

import numpy as np
import pytest

import kernel_matrix as KM
import plan_reference as PLAN
import policy_noise_reference as NR
import policy_reference as POL
import shooting_reference as SR
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N1, FREQ_RATE1 = 130, 2
N, K, H, T = 70, 5, 6, 6
OFFSET = 2 ** 32 + 7
SEED = 2 ** 32 + 11  # the engine's reset key
PLAN_SEED = 2 ** 33 + 5
NOISE_SEED = 2 ** 64 - 3  # seed + t wraps inside the call
GAMMA = 0.97
INIT_NOISE = {"cartpole": 0.0, "ip_staged": 0.05, "ip": 0.05, "dp": 0.05, "cheetah": 0.1, "hopper": 5e-3}


def _engine(row, n, **over):
    from emei_amd.engine import Engine

    kw = dict(row.kw, seed=SEED, env_index_offset=OFFSET, init_noise=INIT_NOISE[row.family])
    kw.update(over)
    eng = Engine(row.env, n, **kw)
    eng.reset(SEED)
    return eng


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _end(eng):
    steps, epi = eng.get_counters()
    return dict(state=eng.get_state().cpu().numpy(), steps=steps.cpu().numpy(), episode=epi.cpu().numpy(),
                compact=eng.compact_done().cpu().numpy())


def _assert_same_end(a, b):
    for k in ("state", "steps", "episode", "compact"):
        assert _same(a[k], b[k]), k


def _rewind(eng):
    eng.unfreeze()
    eng.freeze()


def _dev(a, eng):
    return torch.as_tensor(np.ascontiguousarray(a), device=eng.device)


# ================================================================================================ layer 1: one step against the oracle
@pytest.mark.parametrize("row", KM.LAYER1_ROWS, ids=lambda r: r.id)
def test_layer1_one_step_vs_oracle(row):
    from emei_amd.engine import Engine

    s0, act = row.states(N1), row.actions(N1)
    eng = Engine(row.env, N1, **dict(row.kw, freq_rate=FREQ_RATE1))
    eng.set_state(s0)
    obs, rew, done = eng.step(_dev(act, eng))
    obs, rew, term = obs.cpu().numpy(), rew.cpu().numpy(), (done.cpu().numpy() & 1).astype(bool)
    o_st, o_obs, o_rew, o_term = row.oracle_step(s0, act, FREQ_RATE1)
    ones = np.ones(N1, np.int32)
    got_obs = PLAN.circle(row.env, obs, o_obs)  # the wrapped angles on the oracle's branch
    if row.kw["precision"] == "ref":
        skip = PLAN.undecidable(row.env, o_obs[None], ones, row.kw)
        assert skip.mean() <= 0.01
        assert rel_err(eng.get_state().cpu().numpy(), o_st, floor=1.0) <= 1e-9
        assert rel_err(PLAN.circle(row.env, eng.get_obs().cpu().numpy(), o_obs), o_obs, floor=1.0) <= 1e-9
        assert rel_err(got_obs, o_obs) <= 1e-5
        assert rel_err(rew, o_rew) <= (2e-5 if row.body else 1e-5)
        assert np.array_equal(term[~skip], o_term[~skip])
        if row.family in ("cheetah", "hopper") and row.kw["solver"] == "newton":
            assert eng.solver_cap_hits() == 0
    else:
        tol, floor, what = row.f32_bound()
        rows = row.f32_rows(N1)
        if row.family == "hopper":  # rows on which the oracle itself cannot be held to the bound (at most 1 %: test_kernel_matrix.py)
            bad = row.ill_conditioned(s0, act, FREQ_RATE1, tol, floor)
            assert (bad & rows).mean() <= 0.01
            rows = rows & ~bad
        errs = {"obs": rel_err(got_obs[rows], o_obs[rows], floor=floor), "reward": rel_err(rew[rows], o_rew[rows], floor=floor)}
        worst = max(errs[k] for k in what)
        e = np.abs(got_obs - o_obs) / np.maximum(np.abs(o_obs), floor)
        i, j = np.unravel_index(np.argmax(e), e.shape)
        print(f"MEASURED {row.id} {worst:.3e} (bound {tol:.0e}, floor {floor:g}, {'+'.join(what)} on {int(rows.sum())} rows; obs on all "
              f"{N1} rows {rel_err(got_obs, o_obs, floor=floor):.3e} at row {i} coordinate {j}: {got_obs[i, j]:.6e} against "
              f"{o_obs[i, j]:.6e}; reward {rel_err(rew, o_rew, floor=floor):.3e})")
        assert worst <= tol
        # the terminal flag is a function of the observation: where the oracle's flag does not change within the float32 tolerance
        # of its observation, the device's must be the oracle's (at most 2 % of the rows are left out: test_kernel_matrix.py)
        skip = PLAN.undecidable(row.env, o_obs[None], ones, row.kw, tol=tol, floor=floor)
        assert skip.mean() <= 0.02
        keep = ~skip & rows
        assert np.array_equal(term[keep], o_term[keep])
    assert not (done.cpu().numpy() & 2).any()  # no TimeLimit configured
    eng.close()


# ================================================================================================ layer 2: the fused entry points
def _check_returns(row, got, want, what):
    """returns / observations of a fused call against its composition: bit for bit, the cheetah to 1e-9"""
    if row.family == "cheetah":
        assert rel_err(got, want) <= 1e-9, (what, rel_err(got, want))
    else:
        assert _same(got, want), what


def run_rollout(row):
    a, b = _engine(row, N, max_episode_steps=4), _engine(row, N, max_episode_steps=4)
    acts = _dev(row.actions(N, lead=(T,)), a)
    obs, rew, done = a.rollout(acts, auto_reset=True)
    assert a.last_kernel() == row.kernel
    for t in range(T):  # tests/test_gpu_shapes.py:26-41
        o, r, d = b.step(acts[t], auto_reset=True)
        assert torch.equal(o, obs[t]) and torch.equal(r, rew[t]) and torch.equal(d, done[t]), t
    _assert_same_end(_end(a), _end(b))
    assert torch.equal(a.compact_done(), torch.nonzero(done[-1]).flatten().to(torch.int32))
    assert bool((done != 0).any(dim=0).all()) and int(a.get_counters()[1].min()) >= 1  # every env crossed a device reset
    assert bool(torch.isfinite(obs).all())


def run_rollout_chunked(row):
    from emei_amd import _lib as L

    a, b = _engine(row, N, max_episode_steps=4, rollout_chunk_steps=-1), _engine(row, N, max_episode_steps=4, rollout_chunk_steps=2)
    acts = _dev(row.actions(N, lead=(T,)), a)
    oa, ra, da = a.rollout(acts, auto_reset=True)
    ob, rb, db = b.rollout(acts, auto_reset=True)
    assert a.last_kernel() == row.kernel
    assert b.last_kernel() == (L.KERNEL_BODY_RK4_CHUNKED if row.rk4 else L.KERNEL_BODY_CHUNKED)
    assert a.rollout_faults() == 0 and b.rollout_faults() == 0
    assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
    _assert_same_end(_end(a), _end(b))
    assert bool((da != 0).any(dim=0).all())


def _sequences(row, eng):
    acts = row.actions(N * K, lead=(H,))
    return _dev(acts.reshape((H, N, K) + acts.shape[2:]), eng)


def run_evaluate_sequences(row):
    from test_gpu_plan import _compose

    eng = _engine(row, N)
    s0 = row.states(N)
    eng.set_state(s0)
    s0 = eng.get_state().cpu().numpy()  # as the row's precision holds it
    acts = _sequences(row, eng)
    ret, L, fo = (x.cpu().numpy() for x in eng.evaluate_sequences(acts, discount=GAMMA, final_obs=True))
    kw = {k: v for k, v in row.kw.items()}
    e_ret, e_L, e_fo = _compose(row.env, s0, acts, GAMMA, **kw)
    assert ret.shape == (N, K) and L.dtype == np.int32 and fo.shape == (N, K, eng.obs_dim)
    assert np.array_equal(L, e_L)
    _check_returns(row, ret, e_ret, "returns")
    _check_returns(row, fo, e_fo.astype(np.float32), "final_obs")
    if row.env in KM.TERMINATING:
        assert (L < H).any()  # the start rows reach the early exit


def run_plan_shooting(row):
    from test_gpu_shooting import _check_definition, _nominal

    eng = _engine(row, N)
    nom, sigma = _nominal(eng, H, N, seed=K)
    cand, _, _, _ = _check_definition(eng, H, K, PLAN_SEED, GAMMA, nominal=nom, sigma=sigma, cheetah=row.family == "cheetah")
    assert (cand[:, :, 0] != cand[:, :, 1]).any()


def run_plan_mppi(row):
    from test_gpu_mppi import _check_definition, _nominal

    eng = _engine(row, N)
    nom, sigma = _nominal(eng, H, seed=K)
    _check_definition(eng, H, K, PLAN_SEED + 1, GAMMA, nominal=nom, sigma=sigma, cheetah=row.family == "cheetah", label=row.id)


def run_plan_cem(row):
    from test_gpu_cem import _check_definition
    from test_gpu_mppi import _nominal

    eng = _engine(row, N)
    nom, sigma = _nominal(eng, H, seed=K)
    _check_definition(eng, H, K, 2, PLAN_SEED + 2, GAMMA, nominal=nom, sigma=sigma, cheetah=row.family == "cheetah", label=row.id)


def _mpc(row, planner):
    """the fused controller against the loop of plan_* and step on a second engine (tests/test_gpu_mpc.py:_run_both)"""
    import mpc_cem_reference as RC
    import mpc_reference as RM
    from emei_amd import _lib as L
    from test_gpu_mppi import _nominal

    fused, loop = _engine(row, N, max_episode_steps=4), _engine(row, N, max_episode_steps=4)
    nom, sigma = _nominal(fused, H, seed=K)
    na, nb = nom.clone(), nom.clone()
    clamp = (0.05, 0.95) if fused.act_dim == 0 else ((-1.0, 1.0) if row.family == "dp" else (-3.0, 3.0))
    if planner == "mppi":
        kw = dict(discount=GAMMA, sigma=sigma, clamp=clamp, auto_reset=True)
        a = fused.mpc_mppi(T, H, K, PLAN_SEED, 0.7, na, diagnostics=True, **kw)
        b = RM.mpc_loop(loop, T, H, K, PLAN_SEED, 0.7, nb, **kw)
        want = L.KERNEL_BODY_MPC_MPPI if row.body else L.KERNEL_PEND_MPC_MPPI
    else:
        kw = dict(iterations=2, sigma=sigma, sigma_min=0.05, discount=GAMMA, clamp=clamp, auto_reset=True)
        a = fused.mpc_cem(T, H, K, 2, PLAN_SEED, na, diagnostics=True, **kw)
        b = RC.mpc_cem_loop(loop, T, H, K, 2, PLAN_SEED, nb, **kw)
        want = L.KERNEL_BODY_MPC_CEM if row.body else L.KERNEL_PEND_MPC_CEM
    assert fused.last_kernel() == want
    names = ("actions", "obs", "reward", "done", "plan_return", "plan_diagnostic")
    for name, x, y in zip(names, a, b):
        assert x.shape == y.shape and _same(x.cpu().numpy(), y.cpu().numpy()), name
    assert _same(na.cpu().numpy(), nb.cpu().numpy())
    _assert_same_end(_end(fused), _end(loop))
    assert bool((a[3] != 0).any(dim=0).all())


def run_mpc_mppi(row):
    _mpc(row, "mppi")


def run_mpc_cem(row):
    _mpc(row, "cem")


def _rand(rng, *s):
    return (rng.standard_normal(s) * 1.5 / np.sqrt(s[-1])).astype(np.float32)


def _one_layer(eng, seed, hidden=5):
    """(MLPPolicy, its weights for tests/policy_reference.py): hidden 5"""
    from emei_amd.policy import MLPPolicy

    rng = np.random.default_rng(seed)
    n_out = max(eng.act_dim, 1)
    w = dict(w2=_rand(rng, n_out, hidden), b2=_rand(rng, n_out), w1=_rand(rng, hidden, eng.obs_dim), b1=_rand(rng, hidden))
    return MLPPolicy(**w), types.SimpleNamespace(out="clip", **w)


def _deep(eng, seed, n_out=None, h1=6, h2=5):
    """DeepMLPPolicy / DeepValueFunction weights 6-5: neither width a multiple of the deep kernel's block of four"""
    rng = np.random.default_rng(seed)
    n_out = max(eng.act_dim, 1) if n_out is None else n_out
    return types.SimpleNamespace(w1=_rand(rng, h1, eng.obs_dim), b1=_rand(rng, h1), w2=_rand(rng, h2, h1), b2=_rand(rng, h2),
                                 w3=_rand(rng, n_out, h2), b3=_rand(rng, n_out))


def _deep_policy(eng, seed):
    from emei_amd.policy import DeepMLPPolicy

    w = _deep(eng, seed)
    return DeepMLPPolicy(w.w3, w.b3, w.w2, w.b2, w.w1, w.b1)


def _noise(eng, seed=NOISE_SEED):
    """(PolicyNoise, its description for tests/policy_noise_reference.py): a std per component, epsilon-greedy on the discrete envs"""
    from emei_amd.policy import PolicyNoise

    if eng.act_dim == 0:
        return PolicyNoise(seed, epsilon=0.25), types.SimpleNamespace(mode="eps", seed=seed, epsilon=0.25)
    std = (0.1 + 0.3 * np.arange(1, eng.act_dim + 1, dtype=np.float32) / eng.act_dim).astype(np.float32)
    return PolicyNoise(seed, std=std), types.SimpleNamespace(mode="gauss", seed=seed, std=std)


def _policy_kernel(row, pend_id):
    """the ids of a policy launch come in threes: four-state, body, body RK4"""
    return pend_id + (0 if not row.body else (2 if row.rk4 else 1))


def _fused_policy_run(eng, pol, noise):
    act, obs, rew, done = eng.rollout_policy(T, pol, auto_reset=True, noise=noise)
    r = dict(actions=act.cpu().numpy(), obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), done=done.cpu().numpy())
    r["kernel"], r["end"] = eng.last_kernel(), _end(eng)
    return r


def _assert_policy_parity(row, fused, loop, loop_end, kernel):
    want = loop["actions"] if loop["actions"].dtype.kind == "i" else loop["actions"].astype(np.float32)
    assert _same(fused["actions"], want), "actions"
    for k in ("obs", "reward", "done"):
        assert _same(fused[k], loop[k]), k
    _assert_same_end(fused["end"], loop_end)
    assert fused["kernel"] == kernel
    assert (fused["done"] != 0).any(axis=0).all()  # every env crossed a device reset inside the call
    assert np.isfinite(fused["obs"]).all()


def run_rollout_policy(row):
    from emei_amd import _lib as L

    eng = _engine(row, N, max_episode_steps=4)
    pol, ref = _one_layer(eng, 1000)
    eng.freeze()
    loop = POL.policy_loop(eng, T, ref, True)
    loop_end = _end(eng)
    _rewind(eng)
    _assert_policy_parity(row, _fused_policy_run(eng, pol, None), loop, loop_end, _policy_kernel(row, L.KERNEL_PEND_POLICY))


def run_rollout_policy_noisy(row):
    from emei_amd import _lib as L

    eng = _engine(row, N, max_episode_steps=4)
    pol, ref = _one_layer(eng, 1001)
    noise, nref = _noise(eng)
    noise.bind(eng)
    eng.freeze()
    g = np.arange(N, dtype=np.uint64) + np.uint64(OFFSET)
    loop = NR.noisy_policy_loop(eng, T, ref, nref, lambda t: noise.draws(eng, t), True, g)
    loop_end = _end(eng)
    _rewind(eng)
    fused = _fused_policy_run(eng, pol, noise)
    _assert_policy_parity(row, fused, loop, loop_end, _policy_kernel(row, L.KERNEL_PEND_POLICY_NOISY))
    _rewind(eng)
    plain = _fused_policy_run(eng, pol, None)
    assert not _same(plain["actions"], fused["actions"])  # the noise did something


def run_rollout_policy_deep(row):
    from emei_amd import _lib as L
    from test_gpu_policy_deep import _loop

    eng = _engine(row, N, max_episode_steps=4)
    pol = _deep_policy(eng, 1002).bind(eng)
    eng.freeze()
    for noise in (None, _noise(eng)[0].bind(eng)):  # one kernel, with and without noise
        _rewind(eng)
        loop = _loop(eng, pol, T, noise)
        _rewind(eng)
        _assert_policy_parity(row, _fused_policy_run(eng, pol, noise), loop, loop["end"], _policy_kernel(row, L.KERNEL_PEND_POLICY_DEEP))


def _population(row, deep):
    from emei_amd.policy import DeepPolicyPopulation, PolicyPopulation
    from test_gpu_policy_population import _replay

    eng = _engine(row, N)
    if deep:
        pop = DeepPolicyPopulation.from_policies([_deep_policy(eng, 1100 + p) for p in range(2)])
    else:
        pop = PolicyPopulation.from_policies([_one_layer(eng, 1200 + p)[0] for p in range(2)])
    eng.set_state(row.states(N))
    start = eng.get_state().clone()
    if row.family == "cheetah":
        # the project's lane-lending exception is a statement about lanes with the same wave-mates: member by member (K = 1) the
        # replay's lane i is env i among the same envs, as in the policy-major launch
        per = [_replay(eng, [pop[p]], start, H, GAMMA) for p in range(2)]
        e_ret, e_L, e_fo, acts = (np.concatenate([m[q] for m in per]) for q in range(4))
    else:
        e_ret, e_L, e_fo, acts = _replay(eng, pop, start, H, GAMMA)
    eng.set_state(start)
    ret, L, fo = (t.cpu().numpy() for t in eng.evaluate_policies(pop, H, discount=GAMMA, final_obs=True))
    assert ret.shape == (2, N) and L.dtype == np.int32 and fo.shape == (2, N, eng.obs_dim)
    assert np.array_equal(L, e_L)
    _check_returns(row, ret, e_ret, "returns")
    _check_returns(row, fo, e_fo, "final_obs")
    assert not _same(acts[0], acts[1])  # the members are told apart


def run_evaluate_policies(row):
    _population(row, False)


def run_evaluate_policies_deep(row):
    _population(row, True)


def run_plan_policy(row):
    from test_gpu_policy_plan import _temperature, _twin_actions

    eng = _engine(row, N)
    pol, noise = _one_layer(eng, 1300)[0].bind(eng), _noise(eng, 2 ** 64 - 5)[0].bind(eng)
    start = eng.get_state().clone()
    acts = _twin_actions(eng, pol, noise, start, H, K)
    ret, length = (t.cpu().numpy() for t in eng.evaluate_sequences(acts, discount=GAMMA, start_state=start))
    temp = _temperature(ret)
    out = eng.plan_policy(H, K, pol, noise, discount=GAMMA, temperature=temp, start_state=start, returns=True, length=True, ess=True)
    _check_plan_policy(row, eng, acts.cpu().numpy(), ret, length, [t.cpu().numpy() for t in out], temp)


def _check_plan_policy(row, eng, acts, twin_ret, twin_len, out, temperature):
    from test_gpu_policy_plan import _mean_and_ess

    best_action, best_return, best_index, mean_action, returns, best_length, ess = out
    rows = np.arange(N)
    _check_returns(row, returns, twin_ret, "returns")
    assert np.array_equal(best_index, SR.best_of(returns).astype(np.int32))
    assert _same(best_return, returns[rows, best_index])
    assert np.array_equal(best_length, twin_len[rows, best_index])
    assert _same(best_action, acts[0][rows, best_index])
    a0 = acts[0].reshape(N, K, -1)
    assert (a0[:, 1:] != a0[:, :1]).any()  # the noise reached the candidates
    # the weighted mean and the effective sample size: the header's weights and summation tree from the call's own returns, the one
    # transcendental taken from the device's float64 exp (tests/test_gpu_policy_plan.py), bit for bit
    with np.errstate(all="ignore"):
        arg = (returns - best_return[:, None]) / temperature
    exp = torch.exp(torch.as_tensor(arg, device=eng.device)).cpu().numpy()
    first = a0.astype(np.float32).astype(np.float64)
    want_mean, want_ess = _mean_and_ess(returns, best_return, exp, first)
    assert mean_action.dtype == np.float32 and _same(mean_action.reshape(N, -1), want_mean)
    assert _same(ess, want_ess) and (ess >= 1.0).all() and (ess <= K).all()


def run_plan_policy_deep(row):
    from emei_amd.policy import DeepValueFunction
    from test_gpu_policy_plan_deep import _bootstrap, _temperature, _twin_actions

    eng = _engine(row, N)
    pol, noise = _deep_policy(eng, 1400).bind(eng), _noise(eng, 2 ** 64 - 5)[0].bind(eng)
    v = _deep(eng, 1401, n_out=1)
    value = DeepValueFunction(v.w3, v.b3, v.w2, v.b2, v.w1, v.b1).bind(eng)
    start = eng.get_state().clone()
    acts, ended = _twin_actions(eng, pol, noise, start, H, K)
    ret, length, fobs = eng.evaluate_sequences(acts, discount=GAMMA, start_state=start, final_obs=True)
    ret, length = ret.cpu().numpy(), length.cpu().numpy()
    boot = _bootstrap(ret, ended, fobs, value, GAMMA, H)
    temp = _temperature(boot)
    out = eng.plan_policy(H, K, pol, noise, discount=GAMMA, temperature=temp, start_state=start, returns=True, length=True, ess=True,
                          value=value)
    _check_plan_policy(row, eng, acts.cpu().numpy(), boot, length, [t.cpu().numpy() for t in out], temp)
    if not ended.all():  # (six steps end every candidate of the Balancing double pendulums: the value then reaches nobody)
        assert not _same(boot, ret)  # the value reached the candidates that never terminated


def _next_obs_inputs(row, eng):
    """observation rows of the row's start states (the wrapped angle, as the row's precision holds them) and one action each"""
    eng.set_state(row.states(N))
    return eng.get_obs().clone(), _dev(row.actions(N), eng)


def _step_from(eng, obs, act):
    eng.set_state(obs)
    eng.step(act)
    return eng.get_obs().cpu().numpy()


def _batch_next_obs(row, obs, act):
    from emei_amd import engine as E

    return E.batch_next_obs(row.env, obs, act, row.kw["real_time_scale"], row.kw["freq_rate"], row.kw["precision"],
                            row.kw.get("integrator", "euler"), row.kw.get("ode_method", "euler"))


def run_batch_next_obs(row):
    eng = _engine(row, N)
    obs, act = _next_obs_inputs(row, eng)
    got = _batch_next_obs(row, obs, act)
    assert got.dtype == torch.float64 and tuple(got.shape) == (N, eng.obs_dim)
    _check_returns(row, got.cpu().numpy(), _step_from(eng, obs, act), "next_obs")


RUNNERS = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("run_")}
assert set(RUNNERS) == set(KM.ENTRY_POINTS)


@pytest.mark.parametrize("entry,row", KM.SUPPORTED, ids=[f"{e}-{r.id}" for e, r in KM.SUPPORTED])
def test_layer2_entry_point_equals_its_composition(entry, row):
    RUNNERS[entry](row)


@pytest.mark.parametrize("entry,row", KM.REFUSED, ids=[f"{e}-{r.id}" for e, r in KM.REFUSED])
def test_layer2_unsupported_pair_is_refused(entry, row):
    ref = KM.refusal(entry, row)
    if ref.kind == "raises":
        with pytest.raises(ref.exc, match=ref.match):
            RUNNERS[entry](row)
    elif ref.kind == "ignored":  # the four-state units have no work queue: the option changes nothing
        a, b = _engine(row, N, max_episode_steps=4), _engine(row, N, max_episode_steps=4, rollout_chunk_steps=2)
        acts = _dev(row.actions(N, lead=(T,)), a)
        outs = [e.rollout(acts, auto_reset=True) for e in (a, b)]
        assert a.last_kernel() == row.kernel and b.last_kernel() == row.kernel and b.rollout_faults() == 0
        assert all(torch.equal(x, y) for x, y in zip(*outs))
    else:  # unreachable: emei_next_obs_io cannot name the single-sweep unit; what it runs is the Newton sibling's step
        sibling = next(r for r in KM.ROWS if r.tu == row.tu.replace("s_f", "_f") and r.rk4 == row.rk4)
        eng, sib = _engine(row, N), _engine(sibling, N)
        obs, act = _next_obs_inputs(row, eng)
        got = _batch_next_obs(row, obs, act).cpu().numpy()
        _check_returns(sibling, got, _step_from(sib, obs, act), "next_obs of the Newton sibling")
        assert not _same(got, _step_from(eng, obs, act))  # ... and not the single-sweep unit's
