"""A plain reference of emei_evaluate_sequences (include/emei_hip.h), independent of the HIP library: the CPU oracle steps the
N * K tiled candidates and `contract` restates the header text in NumPy.  Shared by tests/test_plan_reference.py (CPU: the
inputs are shown to be good from the oracle alone) and tests/test_gpu_plan_oracle.py (the fused call against it).  A helper
module: no fixtures, no test."""
import math

import numpy as np

from conftest import rel_err

MUJOCO = dict(freq_rate=4, real_time_scale=0.002)  # half_cheetah.py:12, hopper.py:20

# env id -> (oracle family, oracle variant)
FAMILY = {
    "CartPoleSwingUp": ("cartpole", "swingup"),
    "CartPoleBalancing": ("cartpole", "balancing"),
    "ReboundInvertedPendulumBalancing": ("ip", "rebound_balancing"),
    "BoundaryInvertedPendulumBalancing": ("ip", "boundary_balancing"),
    "ReboundInvertedPendulumSwingUp": ("ip", "rebound_swingup"),
    "BoundaryInvertedPendulumSwingUp": ("ip", "boundary_swingup"),
    "ReboundInvertedDoublePendulumBalancing": ("dp", "rebound_balancing"),
    "BoundaryInvertedDoublePendulumBalancing": ("dp", "boundary_balancing"),
    "ReboundInvertedDoublePendulumSwingUp": ("dp", "rebound_swingup"),
    "BoundaryInvertedDoublePendulumSwingUp": ("dp", "boundary_swingup"),
    "HalfCheetahRunning": ("cheetah", None),
    "HopperRunning": ("hopper", None),
}
# observation coordinates that are angles the env wraps: compared on the circle (test_gpu_invpend.py:86)
WRAPPED = {"cartpole": (), "ip": (1,), "dp": (1, 2), "cheetah": (), "hopper": ()}

# per-step reward tolerance the project holds each kernel to against the same oracle (test_gpu_cartpole.py, test_gpu_invpend.py:12,
# test_gpu_dpend.py:45, test_gpu_cheetah.py:48 one step; test_gpu_cheetah.py:143 and test_gpu_hopper.py:117 over 20 steps)
TOL_R = {"cartpole": 1e-5, "ip": 1e-5, "dp": 1e-5, "cheetah": 1e-4, "hopper": 1e-4}
TOL_OBS = 1e-5  # the project's per-step observation tolerance (rel_err with its 1e-3 floor)


# ------------------------------------------------------------------------------------------------ the contract
def contract(obs, reward_f32, terminal, discount):
    """The header text of emei_evaluate_sequences from per-step outputs obs [H, M, obs_dim], reward_f32 [H, M], terminal [H, M]:
    L = index of the first set terminal bit + 1 (else H); ret = sum_{t < L} discount^t * float64(float32 r_t); final_obs =
    obs[L - 1].  The sum is math.fsum of products with discount ** t: neither the kernel's running product nor its running sum.
    -> (ret float64 [M], L int32 [M], final_obs [M, obs_dim])"""
    reward_f32 = np.asarray(reward_f32)
    assert reward_f32.dtype == np.float32
    term = np.asarray(terminal).astype(bool)
    H, M = term.shape
    L = np.where(term.any(axis=0), term.argmax(axis=0) + 1, H).astype(np.int32)
    r64 = reward_f32.astype(np.float64)
    ret = np.array([math.fsum(float(discount) ** t * float(r64[t, m]) for t in range(L[m])) for m in range(M)])
    return ret, L, np.asarray(obs)[L - 1, np.arange(M)]


def ret_bound(reward_f32, L, discount, tol_r):
    """tol_r * sum_{t < L} discount^t * max(|r_t|, 1e-3): every counted step's reward off by the per-step tolerance"""
    r = np.maximum(np.abs(np.asarray(reward_f32, np.float64)), 1e-3)
    H, M = r.shape
    w = (float(discount) ** np.arange(H))[:, None] * (np.arange(H)[:, None] < np.asarray(L)[None, :])
    return tol_r * (w * r).sum(axis=0)


# ------------------------------------------------------------------------------------------------ the oracle, step by step
def _opts(kw):
    from oracle import oracle as O

    return O.opts(kw.get("integrator", "euler"), solver=kw.get("solver", "newton"))


def oracle_steps(env_name, kw, s0, acts):
    """s0 [M, state_dim] float64 (the start rows tiled K times), acts [H, M(, act_dim)], kw the Engine's keyword arguments
    -> (obs float64 [H, M, obs_dim], reward float32 [H, M], terminal bool [H, M]) of the CPU oracle, no reset, no noise."""
    from oracle import oracle as O

    fam, variant = FAMILY[env_name]
    fr, dt = int(kw.get("freq_rate", 1)), float(kw.get("real_time_scale", 0.02))
    st = np.array(s0, np.float64)
    H, M = acts.shape[:2]
    if fam == "cartpole":
        states, rew, term = O.cartpole_rollout(variant, st, np.asarray(acts), fr, dt, kw.get("ode_method", "euler"))
        return states[1:], rew.astype(np.float32), term
    opt, prm = _opts(kw), kw.get("env_params")
    obs = np.empty((H, M, st.shape[1]))
    rew, term = np.empty((H, M)), np.empty((H, M), bool)
    for t in range(H):
        a = np.asarray(acts[t], np.float32).astype(np.float64)  # the float32 action the device reads
        if fam == "ip":
            st, obs[t], rew[t], term[t] = O.ip_step(variant, st, a, fr, dt, opt)
        elif fam == "dp":
            st, obs[t], rew[t], term[t] = O.dpend_step(variant, st, a, fr, dt, opt)
        elif fam == "cheetah":
            st, rew[t], term[t] = O.cheetah_step(st, a, fr, dt, opt, prm)
            obs[t] = st
        else:
            st, rew[t], term[t] = O.hopper_step(st, a, fr, dt, opt, prm)
            obs[t] = st
    return obs, rew.astype(np.float32), term


def _terminal(env_name, kw, rows):
    from oracle import oracle as O

    fam, variant = FAMILY[env_name]
    if fam == "cartpole":
        return O.cartpole_terminal(variant, rows)
    if fam == "ip":
        return O.ip_terminal(variant, rows)
    if fam == "dp":
        return O.dpend_reward_terminal(variant, rows)[1]
    if fam == "hopper":
        return O.hopper_healthy_terminal(rows, kw.get("env_params"))[1]
    return np.zeros(len(rows), bool)  # half_cheetah.py: never terminal


def undecidable(env_name, obs, L, kw=None, tol=TOL_OBS, floor=1e-3):
    """Candidates [M] for which the oracle's own terminal function changes its answer at some counted step t < L when the
    observation moves by the project's per-step observation tolerance, 1e-5 * max(|v|, 1e-3) per component (rel_err's floor):
    all components outward, all inward, and each component alone outward and inward (the double pendulum's tip height depends on
    th1 + th2, which the joint move can leave unchanged).  The only candidates a test may leave out.  tol, floor: another observation
    tolerance than the project's 1e-5 with its 1e-3 floor (a float32 mode's: tests/test_gpu_kernel_matrix.py)."""
    kw = kw or {}
    obs = np.asarray(obs, np.float64)
    H, M, D = obs.shape
    rows = obs.reshape(H * M, D)
    step = tol * np.maximum(np.abs(rows), floor) * np.where(rows >= 0, 1.0, -1.0)
    base = _terminal(env_name, kw, rows)
    flip = np.zeros(H * M, bool)
    masks = [np.ones(D)] + [np.eye(D)[d] for d in range(D)]
    for mk in masks:
        for sgn in (1.0, -1.0):
            flip |= _terminal(env_name, kw, rows + sgn * step * mk) != base
    counted = np.arange(H)[:, None] < np.asarray(L)[None, :]
    return (flip.reshape(H, M) & counted).any(axis=0)


def circle(env_name, got, ref):
    """`got` with its wrapped angles moved onto the branch of `ref` (theta wraps at +-pi: compared on the circle)"""
    got = np.array(got, np.float64)
    for d in WRAPPED[FAMILY[env_name][0]]:
        got[..., d] = ref[..., d] + np.angle(np.exp(1j * (got[..., d] - ref[..., d])))
    return got


def compare(case, ref, ret, L, final_obs):
    """a result [M] / [M, obs_dim] against reference(case) on the decidable candidates -> (indices whose length differs, worst
    |ret - ref| / bound, worst final_obs rel_err / TOL_OBS): the test passes when the first is empty and the others <= 1"""
    ok = ~ref["skip"]
    wrong = np.nonzero(ok & (np.asarray(L) != ref["L"]))[0]
    r_ratio = float((np.abs(np.asarray(ret) - ref["ret"]) / ref["bound"])[ok].max())
    o_err = rel_err(circle(case.name, final_obs, ref["final_obs"])[ok], ref["final_obs"][ok])
    return wrong, r_ratio, o_err / TOL_OBS


# ------------------------------------------------------------------------------------------------ inputs
def cartpole_inputs(name, N, K, H, seed, spread=0.05):
    """uniform(-spread, spread) start rows (the reference's reset, cartpole.py:131-132; SwingUp hangs: theta + pi), fair-coin pushes"""
    rng = np.random.default_rng(seed)
    s0 = rng.uniform(-spread, spread, (N, 4))
    if FAMILY[name][1] == "swingup":
        s0[:, 2] += np.pi
    return s0, rng.integers(0, 2, (H, N, K)).astype(np.uint8)


def pendulum_inputs(name, N, K, H, seed, spread=0.05, amp=None):
    """InvertedPendulum (4 states) / InvertedDoublePendulum (6): uniform(-spread, spread) start rows around upright, actions
    uniform in the ctrlrange (+-3 / +-1)"""
    rng = np.random.default_rng(seed)
    fam = FAMILY[name][0]
    dim, a = (4, 3.0) if fam == "ip" else (6, 1.0)
    s0 = rng.uniform(-spread, spread, (N, dim))
    return s0, rng.uniform(-(amp or a), amp or a, (H, N, K)).astype(np.float32)


def cheetah_inputs(name, N, K, H, seed, spread=0.1):
    """the reset distribution of half_cheetah.py (zeros + 0.1 noise), actions uniform in [-1, 1]^6"""
    rng = np.random.default_rng(seed)
    return rng.normal(0, spread, (N, 18)), rng.uniform(-1, 1, (H, N, K, 6)).astype(np.float32)


def hopper_inputs(name, N, K, H, seed, spread=5e-3, z_spread=0.0):
    """init_qpos (rootz = 1.25) + 5e-3 noise (hopper.py), optionally z spread further; actions uniform in [-1, 1]^3"""
    rng = np.random.default_rng(seed)
    s0 = rng.normal(0, spread, (N, 12))
    s0[:, 1] += 1.25 + rng.uniform(-z_spread, z_spread, N)
    return s0, rng.uniform(-1, 1, (H, N, K, 3)).astype(np.float32)


BUILDERS = {"cartpole": cartpole_inputs, "ip": pendulum_inputs, "dp": pendulum_inputs, "cheetah": cheetah_inputs,
            "hopper": hopper_inputs}


class Case:
    """One launch: env id, Engine keyword arguments, N x K candidates over H steps, the discount, the input builder's arguments.
    ends: the candidates must end early / run the whole horizon / spread over lengths as §(b) of test_plan_reference.py asks."""

    def __init__(self, tag, name, kw, N, K, H, discount, seed, ends=False, **inputs):
        self.tag, self.name, self.kw, self.N, self.K, self.H, self.discount, self.seed = tag, name, kw, N, K, H, discount, seed
        self.ends, self.inputs = ends, inputs
        self.family = FAMILY[name][0]

    def build(self):
        """-> (s0 [N, state_dim] float64, acts [H, N, K(, act_dim)])"""
        return BUILDERS[self.family](self.name, self.N, self.K, self.H, self.seed, **self.inputs)

    def engine_kw(self):
        return dict(self.kw, precision="ref")


_reference_cache = {}


def reference(case):
    """dict(s0, acts, obs, reward, terminal, ret, L, final_obs, bound, skip) of a case, computed once per process and shared
    (read-only arrays)"""
    if case.tag not in _reference_cache:
        s0, acts = case.build()
        H, M = case.H, case.N * case.K
        obs, rew, term = oracle_steps(case.name, case.kw, np.repeat(s0, case.K, axis=0), acts.reshape((H, M) + acts.shape[3:]))
        ret, L, fo = contract(obs, rew, term, case.discount)
        out = dict(s0=s0, acts=acts, obs=obs, reward=rew, terminal=term, ret=ret, L=L, final_obs=fo,
                   bound=ret_bound(rew, L, case.discount, TOL_R[case.family]), skip=undecidable(case.name, obs, L, case.kw))
        for v in out.values():
            v.setflags(write=False)
        _reference_cache[case.tag] = out
    return _reference_cache[case.tag]


# Shapes: N * K a few hundred with N no multiple of 64 and K no divisor of 64 (an env's candidates straddle wave boundaries, the
# last block is ragged); the planar bodies N = 9, K = 15.  H no longer than the stretch over which the env's trajectory test lets
# the oracle run without re-synchronising: 20 env-steps for the cheetah and the Hopper (test_gpu_cheetah.py:135,
# test_gpu_hopper.py:109), 100 substeps for the pendulums (test_gpu_invpend.py:68), CartPole 48.  Discount below 1 except one
# case per family.  Spreads / horizons of the balancing ids are chosen so that >= 5 % of the candidates run the whole horizon.
_HOP_TERM = dict(terminate_when_unhealthy=0.0, healthy_z_lo=1.2, healthy_z_hi=1.4)
CASES = [
    Case("cartpole-swingup", "CartPoleSwingUp", dict(), 37, 7, 48, 0.97, 101),
    Case("cartpole-balancing", "CartPoleBalancing", dict(), 37, 7, 38, 0.95, 102, ends=True),
    Case("cartpole-balancing-g1", "CartPoleBalancing", dict(), 37, 7, 39, 1.0, 103, ends=True),
    Case("cartpole-swingup-rk4", "CartPoleSwingUp", dict(ode_method="rk4"), 37, 7, 48, 0.97, 104),
    Case("cartpole-balancing-fr2", "CartPoleBalancing", dict(freq_rate=2), 37, 7, 19, 0.95, 105, ends=True),
    Case("ip-rebound-balancing", "ReboundInvertedPendulumBalancing", dict(), 37, 7, 33, 0.95, 111, ends=True),
    Case("ip-boundary-balancing", "BoundaryInvertedPendulumBalancing", dict(), 37, 7, 40, 1.0, 112, ends=True),
    Case("ip-rebound-swingup", "ReboundInvertedPendulumSwingUp", dict(), 37, 7, 40, 0.97, 113),
    Case("ip-boundary-swingup", "BoundaryInvertedPendulumSwingUp", dict(), 37, 7, 40, 0.97, 114),
    Case("ip-rebound-balancing-rk4", "ReboundInvertedPendulumBalancing", dict(integrator="rk4"), 37, 7, 33, 0.95, 115, ends=True),
    Case("ip-boundary-balancing-semi", "BoundaryInvertedPendulumBalancing", dict(integrator="semi_implicit_euler"), 37, 7, 40, 0.95,
         116, ends=True),
    Case("dp-rebound-balancing", "ReboundInvertedDoublePendulumBalancing", dict(), 37, 7, 13, 0.95, 121, ends=True),
    Case("dp-boundary-balancing", "BoundaryInvertedDoublePendulumBalancing", dict(), 37, 7, 26, 1.0, 122, ends=True),
    Case("dp-rebound-swingup", "ReboundInvertedDoublePendulumSwingUp", dict(), 37, 7, 40, 0.97, 123),
    Case("dp-boundary-swingup", "BoundaryInvertedDoublePendulumSwingUp", dict(), 37, 7, 40, 0.97, 124),
    Case("cheetah-euler", "HalfCheetahRunning", dict(MUJOCO), 9, 15, 20, 0.97, 131),
    Case("cheetah-semi", "HalfCheetahRunning", dict(MUJOCO, integrator="semi_implicit_euler"), 9, 15, 12, 1.0, 132),
    Case("cheetah-rk4", "HalfCheetahRunning", dict(MUJOCO, integrator="rk4"), 9, 15, 10, 0.97, 133),
    Case("cheetah-sweep1", "HalfCheetahRunning", dict(MUJOCO, solver="sweep1"), 9, 15, 12, 0.97, 134),
    Case("hopper-rk4", "HopperRunning", dict(MUJOCO, integrator="rk4"), 9, 15, 20, 0.97, 141),
    Case("hopper-euler", "HopperRunning", dict(MUJOCO, integrator="euler"), 9, 15, 20, 1.0, 142),
    Case("hopper-sweep1", "HopperRunning", dict(MUJOCO, integrator="rk4", solver="sweep1"), 9, 15, 12, 0.97, 143),
    Case("hopper-terminating", "HopperRunning", dict(MUJOCO, integrator="rk4", env_params=_HOP_TERM), 9, 15, 20, 0.97, 144,
         ends=True, z_spread=0.04),
]
CASE_IDS = [c.tag for c in CASES]
