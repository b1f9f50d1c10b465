"""body_rollout_kernel's auto-reset against the oracle twin (tests/body_twin.py) ACROSS episodes: the spare initial state of the
kSpareReset bodies (drawn for episode + 1 when a wave-mate resets, used steps later, not reused), the per-lane reset of the
other bodies, the observation-noise counter (env, episode, steps) behind a reset, and episode_init_obs — for the
InvertedDoublePendulum, the Hopper, the HalfCheetah-style body and the InvertedPendulum on the body path.

A case is 130 envs (two full waves and a ragged one of 2 lanes) at env_index_offset 4000, rolled out in segments.  After every
segment the device's done codes are compared bit for bit, its float32 observations and rewards to the suite's float32
tolerances, its counters exactly and its float64 state to the case's measured tolerance; then the twin takes the device's state
(as test_trajectory_vs_oracle does), so chaos never accumulates beyond one segment.  An env whose terminal predicate the twin
sees within 1e-5 of a threshold is left out from that step on; at most one env per case may be.

Tolerances.  Observations 1e-5, rewards 1e-5 (pendulums) / 1e-4 (cheetah, Hopper), as absolute-or-relative errors
(rel_err(..., floor=1.0): positions and angles pass through zero and their error is set by O(1) dynamics, as in
test_autoreset_rollout_vs_oracle).  The state at a boundary carries the device's hardware Box-Muller (within 1.5e-6 of the
oracle's exact z: 1.5e-6 * sigma per reset coordinate and per noise draw) through up to one segment of dynamics; 4 x the
figure tests/test_body_twin.py:test_tolerance_measured measures on the CPU by moving every draw by +-1.5e-6 * sigma:

    case                          segment  measured   state_tol
    dp-rebound_balancing-euler       4     1.50e-06   6.0e-06      (segments of 8: 4.05e-06, of 5: 2.20e-06)
    dp-rebound_balancing-rk4         4     6.85e-07   2.8e-06
    dp-boundary_balancing-euler      4     1.73e-06   7.0e-06      (segments of 8: 5.79e-06, of 5: 2.71e-06 -> 4 x is above 1e-5)
    dp-boundary_balancing-rk4        4     7.04e-07   2.9e-06
    dp-*_swingup-euler               4     9.83e-07   4.0e-06
    dp-*_swingup-rk4                 4     6.18e-07   2.5e-06
    hopper-rk4                       6     7.08e-07   2.9e-06
    cheetah-euler-iid                1     1.77e-06   7.1e-06      (init_noise 0.1; segments of 2: 3.2e-05, of 6: 4.9e-05)
    cheetah-rk4-shared               1     9.05e-07   3.7e-06      (segments of 2: 6.0e-05)
    cheetah-euler-gentle             6     5.44e-07   2.2e-06      (init_noise 0.01)
    ip-rebound_balancing-rk4         8     2.00e-06   8.1e-06      (init_noise 0.2: episodes short enough for two resets per launch)

Envs with neither a reset nor a noise draw inside a segment keep the suite's 1e-9."""
import numpy as np
import pytest

import body_twin as B
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = {c["id"]: c for c in B.CASES}
BARE = {c["id"]: c for c in B.BARE_CASES}
ENVS = [0, 1, 63, 64, 128, 129]  # first / last lanes of the full waves and both lanes of the ragged one


def _engine(c, precision="ref", chunk=0):
    from emei_amd.engine import Engine

    return Engine(c["env"], c["n"], freq_rate=c["freq_rate"], real_time_scale=c["dt"], precision=precision,
                  max_episode_steps=c["max_episode_steps"], seed=c["seed"], env_index_offset=c["env_offset"], init_noise=c["init_noise"],
                  integrator=c["integrator"], obs_noise=c["obs_noise"], noise_layout="shared" if c["shared"] else "iid",
                  env_params=c["params"], rollout_chunk_steps=chunk)


def _expected_kernel(c, chunked):
    from emei_amd import _lib as L

    if c["integrator"] == "rk4":
        return L.KERNEL_BODY_RK4_CHUNKED if chunked else L.KERNEL_BODY_RK4
    return L.KERNEL_BODY_CHUNKED if chunked else L.KERNEL_BODY


def _draw_bound(c, want, f32=False):
    """|device reset state - oracle's|: the project's Box-Muller bound, sigma * 1.5e-6 per coordinate (test_init_layouts_on_device,
    tools/bm_accuracy.hip); a float32 state adds one float32 ulp of the value"""
    b = B.sigma_vector(c["kind"], c["init_noise"]) * B.BM_EPS
    return b + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) if f32 else b + 0.0 * want


def _run_case(c, chunk=0):
    """the segmented comparison of the module docstring -> dict(kernels, excluded, episodes)"""
    n, acts = c["n"], B.case_actions(c)
    eng = _engine(c, chunk=chunk)
    eng.reset(c["seed"])
    st = eng.get_state().cpu().numpy()
    want0 = B.case_init(c)
    assert (np.abs(st - want0) <= _draw_bound(c, want0)).all()  # episode 0
    sc, ep = np.zeros(n, np.int64), np.zeros(n, np.int64)
    excluded = np.zeros(n, bool)
    noisy = any(s != 0.0 for s in B.pair(c["obs_noise"]))
    kernels = set()
    for a, b in B.segments(c):
        obs, rew, done = eng.rollout(torch.as_tensor(acts[a:b], device=eng.device), auto_reset=True)
        kernels.add(eng.last_kernel())
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        d_st = eng.get_state().cpu().numpy()
        d_sc, d_ep = (x.cpu().numpy().astype(np.int64) for x in eng.get_counters())
        tw = B.case_rollout(c, st, sc, ep, acts[a:b])
        # an env near a threshold at step t is left out from t to the end of the case
        out_t = excluded[None, :] | (np.cumsum(tw["near"], axis=0) > 0)
        keep = ~out_t
        excluded = out_t[-1]
        ok = ~excluded
        touched = (tw["done"] != 0).any(axis=0) | noisy
        e_obs = rel_err(obs[keep], tw["obs"][keep], floor=1.0)
        e_rew = rel_err(rew[keep], tw["reward"][keep], floor=1.0)
        e_st = rel_err(d_st[ok & touched], tw["state"][ok & touched], floor=1.0)
        e_clean = rel_err(d_st[ok & ~touched], tw["state"][ok & ~touched], floor=1.0)
        print(f"{c['id']} steps [{a}, {b}): obs {e_obs:.2e} reward {e_rew:.2e} state {e_st:.2e} (tol {c['state_tol']:.1e}) untouched {e_clean:.2e} "
              f"done mismatches {int((done[keep] != tw['done'][keep]).sum())} endings {int((tw['done'] != 0).sum())} excluded {int(excluded.sum())}")
        assert np.array_equal(done[keep], tw["done"][keep]), (c["id"], a)
        assert np.array_equal(d_sc[ok], tw["steps"][ok]) and np.array_equal(d_ep[ok], tw["episode"][ok]), (c["id"], a)
        assert e_obs <= B.OBS_TOL and e_rew <= B.REWARD_TOL[c["kind"]], (c["id"], a, e_obs, e_rew)
        assert e_st <= c["state_tol"] and e_clean <= 1e-9, (c["id"], a, e_st, e_clean)
        st, sc, ep = d_st, d_sc, d_ep  # re-synchronise (an excluded env goes on from the device's own counters)
    assert int(excluded.sum()) <= 1, (c["id"], np.nonzero(excluded)[0])
    assert ep[~excluded].min() >= 2  # every env compared over at least three episodes
    assert eng.rollout_faults() == 0 and eng.solver_cap_hits() == 0
    return dict(kernels=kernels, excluded=excluded, episodes=ep)


@pytest.mark.parametrize("case_id", B.CASE_IDS)
def test_autoreset_vs_twin(case_id):
    c = CASES[case_id]
    r = _run_case(c)
    assert r["kernels"] == {_expected_kernel(c, False)}  # 3 waves: the automatic policy launches in one piece


@pytest.mark.parametrize("chunk", [-1, 3])
@pytest.mark.parametrize("case_id", ["dp-rebound_balancing-euler", "dp-boundary_balancing-rk4", "cheetah-euler-gentle"])
def test_autoreset_vs_twin_chunked_and_one_piece(case_id, chunk):
    """In a chunked launch every work item starts without a spare while `episode` and `steps` come from memory: the same twin."""
    c = CASES[case_id]
    assert c["seg"] > 3  # a segment is cut into more than one item
    r = _run_case(c, chunk=chunk)
    assert r["kernels"] == {_expected_kernel(c, chunk == 3)}


@pytest.mark.parametrize("layout", ["iid", "shared"])
@pytest.mark.parametrize("precision", ["ref", "f32"])
@pytest.mark.parametrize("kind", sorted(BARE))
def test_bare_reset_draws_and_init_obs(kind, precision, layout):
    """Segment length = max_episode_steps on a TimeLimit-only configuration without observation noise: at every boundary each env
    has just been reset, so get_state() is the bare draw of (env, episode = 1, 2, 3) — no dynamics involved — and equals
    O.body_init + init_qpos within sigma * 1.5e-6 (float32 states: plus one float32 ulp of the value).  episode_init_obs(env,
    episode) for episodes 0..3 is the observation of that draw: compared with the oracle's (through the pendulums' angle wraps,
    with the Hopper's 1.25) and, bit for bit, with the observation of the state the rollout left at the matching boundary."""
    c = dict(BARE[kind], shared=layout == "shared")
    n, nv, acts = c["n"], B.DIM[c["kind"]] // 2, B.case_actions(c)
    f32 = precision == "f32"
    eng = _engine(c, precision=precision)
    eng.reset(c["seed"])
    base = B.base_state(c["kind"])
    sig = B.sigma_vector(c["kind"], c["init_noise"])
    envs = torch.as_tensor(ENVS)
    for k in range(4):
        if k > 0:
            a, b = B.segments(c)[k - 1]
            _, _, done = eng.rollout(torch.as_tensor(acts[a:b], device=eng.device), auto_reset=True)
            assert eng.last_kernel() == _expected_kernel(c, False)
            done = done.cpu().numpy()
            assert not done[:-1].any() and (done[-1] == 2).all()
        steps, epi = (x.cpu().numpy() for x in eng.get_counters())
        assert not steps.any() and (epi == k).all()
        st = eng.get_state().cpu().numpy()
        want = B.case_init(c, k)
        err = np.abs(st - want)
        print(f"{kind} {precision} {layout} episode {k}: worst |state - oracle| / bound {float((err / _draw_bound(c, want, f32)).max()):.3f}")
        assert (err <= _draw_bound(c, want, f32)).all(), (kind, k)
        off = st - base
        if layout == "iid":  # a draw per coordinate, of the configured sigmas
            assert off[:, :nv].std() == pytest.approx(sig[0], rel=0.25) and off[:, nv:].std() == pytest.approx(sig[nv], rel=0.25)
            assert np.abs(off[:, :nv] - off[:, :1]).max() > sig[0]
        else:  # one draw for all of qpos, one for all of qvel
            rest = [j for j in range(nv) if base[j] == 0.0]
            assert np.array_equal(off[:, rest], np.repeat(off[:, rest[:1]], len(rest), axis=1))
            assert np.array_equal(off[:, nv:], np.repeat(off[:, nv : nv + 1], nv, axis=1))
            z_slack = np.spacing(np.float32(1.25)) if f32 else 1e-12  # 1.25 + d - 1.25 rounds in the state's precision
            assert np.abs(off[:, :nv] - off[:, rest[:1]]).max() <= z_slack
            assert off[:, rest[0]].std() == pytest.approx(sig[0], rel=0.25) and off[:, nv].std() == pytest.approx(sig[nv], rel=0.25)
        # episode_init_obs of this episode
        io = eng.episode_init_obs(envs, torch.full((len(ENVS),), k)).cpu().numpy()
        assert io.dtype == np.float32 and io.shape == (len(ENVS), 2 * nv)
        assert np.array_equal(io, eng.get_obs().cpu().numpy()[ENVS].astype(np.float32)), (kind, k)
        if not f32:
            o_want = B.observe(c["kind"], want[ENVS])
            slope = np.ones(2 * nv)
            if c["kind"] == "dp":
                slope[1:3] = np.pi  # (theta + pi) % 2 * pi - pi (sic) multiplies an angle's error by pi
            bound = sig * B.BM_EPS * slope + np.spacing(np.abs(o_want).astype(np.float32))
            assert (np.abs(io - o_want) <= bound).all(), (kind, k)
    # a different episode or env is a different draw
    other = eng.episode_init_obs(envs, torch.full((len(ENVS),), 2)).cpu().numpy()
    assert np.abs(other - io).max() > 1e-3 * sig.max()


@pytest.mark.parametrize("case_id", ["dp-boundary_balancing-euler", "hopper-rk4"])
def test_init_obs_is_the_state_after_a_done_mid_rollout(case_id):
    """Asynchronous endings: after a rollout the envs whose LAST step ended an episode hold the reset state of their new
    episode, and episode_init_obs(env, that episode) is its observation bit for bit — and the oracle's draw within the bound."""
    c = CASES[case_id]
    acts = B.case_actions(c)
    eng = _engine(c)
    eng.reset(c["seed"])
    seen = 0
    for a, b in B.segments(c):
        _, _, done = eng.rollout(torch.as_tensor(acts[a:b], device=eng.device), auto_reset=True)
        idx = np.nonzero(done[-1].cpu().numpy())[0]
        if not len(idx):
            continue
        steps, epi = (x.cpu().numpy() for x in eng.get_counters())
        assert not steps[idx].any() and (epi[idx] >= 1).all()
        io = eng.episode_init_obs(torch.as_tensor(idx), torch.as_tensor(epi[idx])).cpu().numpy()
        assert np.array_equal(io, eng.get_obs().cpu().numpy()[idx].astype(np.float32))
        want = np.stack([B.init_state(c["kind"], c["seed"], c["env_offset"] + int(i), int(epi[i]), c["init_noise"]) for i in idx])
        st = eng.get_state().cpu().numpy()[idx]
        assert (np.abs(st - want) <= _draw_bound(c, want)).all()
        seen += len(idx)
    assert seen >= 20
