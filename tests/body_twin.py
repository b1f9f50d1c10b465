"""Oracle twin of `emei_rollout(..., EMEI_FLAG_AUTO_RESET)` for the bodies that run on body_rollout_kernel (host code: NumPy
plus oracle.oracle), and the cases tests/test_body_twin.py (CPU) and tests/test_gpu_body_autoreset.py (GPU) share.

The twin steps N envs with the oracle's float64 step functions and restates the auto-reset of include/emei_hip.h: after a
step, steps += 1, done = terminal | truncated << 1 with truncated = max_episode_steps > 0 and steps >= max_episode_steps; on
done != 0 the env goes to episode + 1, steps = 0, state = init noise of (seed, env_offset + row, episode) + init_qpos.  The
observation noise of an env-step is indexed by (env, episode, steps before the step): `oracle_opts_t` carries one
(episode, step_index) per call, so with noise on the step function is called once per run of consecutive rows that share them.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import oracle as O

DIM = {"ip": 4, "dp": 6, "cheetah": 18, "hopper": 12}
BM_EPS = 1.5e-6  # |device Box-Muller z - exact z| (tools/bm_accuracy.hip, tests/test_gpu_integrators.py:test_init_layouts_on_device)
NEAR = 1e-5      # a terminal predicate's quantity this close to its threshold may fall on either side on the device

ENV_NAMES = {
    ("dp", "rebound_balancing"): "ReboundInvertedDoublePendulumBalancing",
    ("dp", "boundary_balancing"): "BoundaryInvertedDoublePendulumBalancing",
    ("dp", "rebound_swingup"): "ReboundInvertedDoublePendulumSwingUp",
    ("dp", "boundary_swingup"): "BoundaryInvertedDoublePendulumSwingUp",
    ("ip", "rebound_balancing"): "ReboundInvertedPendulumBalancing",
    ("ip", "boundary_balancing"): "BoundaryInvertedPendulumBalancing",
    ("ip", "rebound_swingup"): "ReboundInvertedPendulumSwingUp",
    ("ip", "boundary_swingup"): "BoundaryInvertedPendulumSwingUp",
    ("cheetah", None): "HalfCheetahRunning",
    ("hopper", None): "HopperRunning",
}


def pair(x):
    """one sigma or (pos, vel) -> (pos, vel)"""
    return (float(x[0]), float(x[1])) if isinstance(x, (tuple, list)) else (float(x), float(x))


def sigma_vector(kind, sig):
    nv = DIM[kind] // 2
    p, v = pair(sig)
    return np.array([p] * nv + [v] * nv)


def base_state(kind):
    """init_qpos ++ init_qvel: zero except the Hopper's rootz reference"""
    b = np.zeros(DIM[kind])
    if kind == "hopper":
        b[1] = 1.25
    return b


def init_state(kind, seed, env, episode, init_noise, shared=False):
    """the device reset of global env `env` for `episode` (body_kernels.h:body_init), float64 [dim]"""
    p, v = pair(init_noise)
    return O.body_init(seed, env, episode, DIM[kind] // 2, p, v, shared) + base_state(kind)


def observe(kind, state):
    """float64 observation rows of state rows (the pendulums wrap their angles)"""
    o = np.array(state, np.float64).reshape(-1, DIM[kind]).copy()
    if kind == "ip":
        o[:, 1] = O.ip_wrap(o[:, 1])
    elif kind == "dp":
        o[:, 1], o[:, 2] = O.dpend_wrap(o[:, 1]), O.dpend_wrap(o[:, 2])
    return o


def near_threshold(kind, variant, obs, params=None):
    """rows whose terminal predicate tests a quantity within NEAR of its threshold, or that hold a non-finite value"""
    o = np.asarray(obs, np.float64)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(o).all(axis=1)
        close = lambda q, thr: np.abs(q - thr) < NEAR
        if kind == "dp":
            y = np.cos(o[:, 1]) + np.cos(o[:, 1] + o[:, 2])
            if variant == "rebound_balancing":
                bad |= close(y, 1.5)
            elif variant == "boundary_balancing":
                bad |= close(y, 0.0) | close(np.abs(o[:, 0]), 3.0)
            elif variant == "boundary_swingup":
                bad |= close(np.abs(o[:, 0]), 3.0)
        elif kind == "ip":
            m = O.ip_model()
            y = np.cos(o[:, 1])
            rail = close(o[:, 0], m.x_lo) | close(o[:, 0], m.x_hi)
            if variant == "rebound_balancing":
                bad |= close(y, 0.9)
            elif variant == "boundary_balancing":
                bad |= close(y, 0.0) | rail
            elif variant == "boundary_swingup":
                bad |= rail
        elif kind == "hopper":
            P = O._params(O.HOPPER_DEFAULTS, params)
            if P[3] == 0.0:  # terminate_when_unhealthy = False is the setting under which the Hopper terminates (planar_oracle.c)
                bad |= close(o[:, 1], P[6]) | close(o[:, 1], P[7])
                bad |= (close(o[:, 2:], P[4]) | close(o[:, 2:], P[5])).any(axis=1)
    return bad


def _step(kind, variant, st, act, fr, dt, opt, params):
    """-> (next_state, obs, reward, terminal) of one oracle call"""
    if kind == "ip":
        return O.ip_step(variant, st, act, fr, dt, opt)
    if kind == "dp":
        return O.dpend_step(variant, st, act, fr, dt, opt)
    if kind == "cheetah":
        s, r, d = O.cheetah_step(st, act, fr, dt, opt, params)
    else:
        s, r, d = O.hopper_step(st, act, fr, dt, opt, params)
    return s, s.copy(), r, d


def _runs(episode, steps):
    """[lo, hi) runs of consecutive rows that share (episode, steps)"""
    cut = np.nonzero((np.diff(episode) != 0) | (np.diff(steps) != 0))[0] + 1
    edges = np.concatenate([[0], cut, [len(episode)]])
    return list(zip(edges[:-1].tolist(), edges[1:].tolist()))


def rollout(kind, variant, state, steps, episode, actions, seed, env_offset=0, max_episode_steps=0, freq_rate=1, dt=0.02,
            integrator="euler", init_noise=0.0, obs_noise=0.0, shared=False, params=None, perturb=None, follow_done=None, eps=BM_EPS):
    """T auto-reset env-steps of N envs.  state [N, dim] float64, steps [N], episode [N] (copied), actions float32 [T, N(, nu)].
    -> dict(obs [T,N,dim] f64, reward [T,N] f64, done [T,N] u8 (terminal | truncated << 1), near [T,N] bool, state, steps,
    episode, calls = oracle step calls made).

    perturb = a np.random.Generator: the tolerance measurement of tests/test_body_twin.py — every reset draw and every
    observation-noise draw is moved by +-eps * sigma (random signs, per coordinate).  The env-step is then made of freq_rate
    one-substep calls (step_index = steps * freq_rate + k addresses the same noise blocks: integrators.h:oracle_env_step), the
    reward of the cheetah / Hopper is evaluated on the whole step afterwards, and `follow_done` [T, N] (the unperturbed run's
    codes) decides the resets so that both runs stay in the same episodes."""
    dim = DIM[kind]
    st = np.array(state, np.float64).reshape(-1, dim).copy()
    n = st.shape[0]
    act = np.asarray(actions, np.float32)
    T = act.shape[0]
    act = act.reshape((T, n) if kind in ("ip", "dp") else (T, n, -1)).astype(np.float64)
    sc, ep = np.array(steps, np.int64).copy(), np.array(episode, np.int64).copy()
    op, ov = pair(obs_noise)
    noisy = op != 0.0 or ov != 0.0
    sig_init, sig_obs = sigma_vector(kind, init_noise), sigma_vector(kind, obs_noise)
    obs, rew = np.empty((T, n, dim)), np.empty((T, n))
    done, near = np.zeros((T, n), np.uint8), np.zeros((T, n), bool)
    calls = 0
    sign = (lambda shape: perturb.choice([-1.0, 1.0], size=shape)) if perturb is not None else None

    def opt(lo, k=None):
        if not noisy:
            return O.opts(integrator)
        idx = int(sc[lo]) if k is None else int(sc[lo]) * freq_rate + k
        return O.opts(integrator, obs_noise=(op, ov), shared=shared, seed=seed, env_offset=env_offset + lo, episode=int(ep[lo]), step_index=idx)

    for t in range(T):
        runs = _runs(ep, sc) if noisy else [(0, n)]
        term = np.empty(n, bool)
        if perturb is None:
            for lo, hi in runs:
                st[lo:hi], obs[t, lo:hi], rew[t, lo:hi], term[lo:hi] = _step(kind, variant, st[lo:hi], act[t, lo:hi], freq_rate, dt, opt(lo), params)
                calls += 1
        else:
            pre = st.copy()
            for k in range(freq_rate):
                for lo, hi in runs:
                    st[lo:hi], obs[t, lo:hi], rew[t, lo:hi], term[lo:hi] = _step(kind, variant, st[lo:hi], act[t, lo:hi], 1, dt, opt(lo, k), params)
                    calls += 1
                if noisy:
                    st += sign(st.shape) * eps * sig_obs
            obs[t] = observe(kind, st)
            if kind == "cheetah":
                rew[t] = O.cheetah_reward(st, pre, act[t], dt * freq_rate, params)
            elif kind == "hopper":
                rew[t] = O.hopper_reward(st, pre, act[t], dt * freq_rate, params)
        sc += 1
        trunc = (sc >= max_episode_steps) if max_episode_steps > 0 else np.zeros(n, bool)
        done[t] = term.astype(np.uint8) | (trunc.astype(np.uint8) << 1)
        near[t] = near_threshold(kind, variant, obs[t], params)
        for i in np.nonzero(done[t] if follow_done is None else follow_done[t])[0]:
            ep[i] += 1
            sc[i] = 0
            st[i] = init_state(kind, seed, env_offset + i, int(ep[i]), init_noise, shared)
            if perturb is not None:
                st[i] += sign(dim) * eps * sig_init
    return dict(obs=obs, reward=rew, done=done, near=near, state=st, steps=sc, episode=ep, calls=calls)


# ----------------------------------------------------------------------------------------------- the shared cases
N_ENVS = 130          # two full waves and a ragged one of 2 lanes
ENV_OFFSET = 4000
HOPPER_PARAMS = dict(terminate_when_unhealthy=0.0, healthy_z_lo=1.22, healthy_z_hi=1.5)


def _case(id, kind, variant, **kw):
    c = dict(id=id, kind=kind, variant=variant, env=ENV_NAMES[(kind, variant)], n=N_ENVS, env_offset=ENV_OFFSET, seed=17, act_seed=29,
             T=48, seg=8, max_episode_steps=12, freq_rate=1, dt=0.02, integrator="euler", init_noise=5e-2, obs_noise=0.01,
             shared=False, params=None, act_scale=1.0, mixed=False, asynchronous=False, double_reset=False, state_tol=None)
    c.update(kw)
    return c


REWARD_TOL = {"ip": 1e-5, "dp": 1e-5, "cheetah": 1e-4, "hopper": 1e-4}  # the suite's float32 reward tolerances
OBS_TOL = 1e-5


# state_tol: the float64 state against the twin at a segment boundary, scaled as rel_err(..., floor=1.0).  Four times the value
# tests/test_body_twin.py:test_tolerance_measured measures (and holds these figures to); profiles/EXPERIMENTS.md has the table.
CASES = []
# Double pendulum: segments of 4 steps (8 and 5 measure looser than 1e-5, see the table) against a TimeLimit of 11, so that
# TimeLimit resets fall inside segments (11, 22, 33) and on a boundary (44)
_DP_TOL = {"rebound_balancing": (6.0e-6, 2.8e-6), "boundary_balancing": (7.0e-6, 2.9e-6), "rebound_swingup": (4.0e-6, 2.5e-6),
           "boundary_swingup": (4.0e-6, 2.5e-6)}
for _v in ("rebound_balancing", "boundary_balancing", "rebound_swingup", "boundary_swingup"):
    _bal = _v.endswith("balancing")
    CASES.append(_case(f"dp-{_v}-euler", "dp", _v, integrator="euler", freq_rate=2, seg=4, max_episode_steps=11, asynchronous=_bal,
                       double_reset=_v == "rebound_balancing", mixed=_v == "boundary_balancing", state_tol=_DP_TOL[_v][0]))
    CASES.append(_case(f"dp-{_v}-rk4", "dp", _v, integrator="rk4", freq_rate=1, seg=4, max_episode_steps=11, asynchronous=_bal,
                       double_reset=_v == "rebound_balancing", state_tol=_DP_TOL[_v][1]))
CASES.append(_case("hopper-rk4", "hopper", None, integrator="rk4", freq_rate=4, dt=0.002, max_episode_steps=16, seg=6, init_noise=0.01,
                   obs_noise=1e-3, params=HOPPER_PARAMS, mixed=True, asynchronous=True, act_seed=4, state_tol=2.9e-6))
# Cheetah, init_noise = 0.1: rootz 0.1 below the floor is a stiff contact that amplifies a draw's 1.5e-7 by 300 within two
# env-steps, so these two cases re-synchronise after EVERY step (the only segment length that measures below 1e-5) ...
CASES.append(_case("cheetah-euler-iid", "cheetah", None, integrator="euler", freq_rate=4, dt=0.002, max_episode_steps=7, T=30, seg=1,
                   init_noise=0.1, obs_noise=1e-3, state_tol=7.1e-6))
CASES.append(_case("cheetah-rk4-shared", "cheetah", None, integrator="rk4", freq_rate=4, dt=0.002, max_episode_steps=7, T=30, seg=1,
                   init_noise=0.1, obs_noise=1e-3, shared=True, state_tol=3.7e-6))
# ... and a gentler one keeps resets INSIDE a launch for the non-spare branch (7, 14, 21, 28 against segments of 6)
CASES.append(_case("cheetah-euler-gentle", "cheetah", None, integrator="euler", freq_rate=4, dt=0.002, max_episode_steps=7, T=30, seg=6,
                   init_noise=0.01, obs_noise=1e-3, state_tol=2.2e-6))
CASES.append(_case("ip-rebound_balancing-rk4", "ip", "rebound_balancing", integrator="rk4", act_scale=3.0, init_noise=0.2, mixed=True,
                   asynchronous=True, double_reset=True, state_tol=8.1e-6))
CASE_IDS = [c["id"] for c in CASES]

# TimeLimit-only configurations whose segment length is max_episode_steps, observation noise off: at every boundary each env
# has just been reset, so the state is the bare draw of (env, episode = 1, 2, 3)
BARE_CASES = [
    _case("dp", "dp", "rebound_swingup", T=9, seg=3, max_episode_steps=3, obs_noise=0.0, init_noise=(0.1, 0.2)),
    _case("ip", "ip", "rebound_swingup", T=9, seg=3, max_episode_steps=3, obs_noise=0.0, init_noise=(0.1, 0.2), integrator="rk4"),
    _case("cheetah", "cheetah", None, T=9, seg=3, max_episode_steps=3, obs_noise=0.0, init_noise=(0.1, 0.2), freq_rate=4, dt=0.002),
    _case("hopper", "hopper", None, T=9, seg=3, max_episode_steps=3, obs_noise=0.0, init_noise=(0.01, 0.02), freq_rate=4, dt=0.002,
          integrator="rk4"),
]


def case_actions(c):
    """float32 actions [T, N(, nu)] of a case"""
    rng = np.random.default_rng(c["act_seed"])
    nu = {"ip": None, "dp": None, "cheetah": 6, "hopper": 3}[c["kind"]]
    shape = (c["T"], c["n"]) if nu is None else (c["T"], c["n"], nu)
    return rng.uniform(-c["act_scale"], c["act_scale"], shape).astype(np.float32)


def case_init(c, episode=0):
    """the oracle's reset states [N, dim] of a case for `episode`"""
    return np.stack([init_state(c["kind"], c["seed"], c["env_offset"] + i, episode, c["init_noise"], c["shared"]) for i in range(c["n"])])


def segments(c):
    """[a, b) step ranges of a case's launches"""
    return [(a, min(a + c["seg"], c["T"])) for a in range(0, c["T"], c["seg"])]


def measure_perturbation(c, seed=5):
    """The tolerance measurement: per segment the twin runs twice from the same state, the second time with every reset and
    noise draw moved by +-BM_EPS * sigma -> the largest scaled (floor 1.0) difference of the boundary states, of the
    observations and of the rewards, over the envs that are not near a threshold."""
    from conftest import rel_err

    acts, rng, n = case_actions(c), np.random.default_rng(seed), c["n"]
    st, sc, ep = case_init(c), np.zeros(n, np.int64), np.zeros(n, np.int64)
    worst = np.zeros(3)
    for a, b in segments(c):
        ref = case_rollout(c, st, sc, ep, acts[a:b])
        per = case_rollout(c, st, sc, ep, acts[a:b], perturb=rng, follow_done=ref["done"])
        ok = ~ref["near"].any(axis=0)
        worst = np.maximum(worst, [rel_err(per["state"][ok], ref["state"][ok], floor=1.0), rel_err(per["obs"][:, ok], ref["obs"][:, ok], floor=1.0),
                                   rel_err(per["reward"][:, ok], ref["reward"][:, ok], floor=1.0)])
        st, sc, ep = ref["state"], ref["steps"], ref["episode"]
    return dict(state=float(worst[0]), obs=float(worst[1]), reward=float(worst[2]))


def case_rollout(c, state, steps, episode, actions, **kw):
    return rollout(c["kind"], c["variant"], state, steps, episode, actions, c["seed"], c["env_offset"], c["max_episode_steps"],
                   c["freq_rate"], c["dt"], c["integrator"], c["init_noise"], c["obs_noise"], c["shared"], c["params"], **kw)
