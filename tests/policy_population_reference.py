"""A numpy twin of emei_evaluate_policies, written from the normative text of include/emei_hip.h and independent of the HIP
library: policy_reference.mlp_actions is the "Policy" clause, the CPU oracle steps the envs one step at a time as
plan_reference.oracle_steps steps them, and the scoring restates "Step and score" as the text has it (a running float64 product
for the discount, a running float64 sum in step order, the reward rounded to float32 first).  Policy after policy: pair (p, i)
never sees another pair.  A helper module: no fixtures, no test."""
import numpy as np

import plan_reference as R
import policy_reference as PR


def first_observation(env_name, s0):
    """x_0 of the text: the observation of the start state as emei_get_obs gives it (float64; the caller rounds).  The 4- and
    6-state pendulums show their angles wrapped, every other env shows its state."""
    from oracle import oracle as O

    fam = R.FAMILY[env_name][0]
    x = np.array(s0, np.float64)
    if fam == "ip":
        x[:, 1] = O.ip_wrap(x[:, 1])
    elif fam == "dp":
        x[:, 1], x[:, 2] = O.dpend_wrap(x[:, 1]), O.dpend_wrap(x[:, 2])
    return x


def evaluate_policies(env_name, kw, s0, policies, H, discount):
    """s0 [N, state_dim] float64, policies: objects with w1 / b1 / w2 / b2 (/ out), kw the Engine's keyword arguments
    -> dict(ret float64 [P, N], L int32 [P, N], final_obs float64 [P, N, obs_dim] (the oracle's row of step L - 1),
            actions [P, H, N(, act_dim)], obs float64 [P, H, N, obs_dim], reward float32 [P, H, N], terminal bool [P, H, N])."""
    fam = R.FAMILY[env_name][0]
    discrete = fam == "cartpole"
    lo, hi = PR.ctrl_range(env_name)
    s0 = np.array(s0, np.float64)
    N = s0.shape[0]
    out = dict(ret=[], L=[], final_obs=[], actions=[], obs=[], reward=[], terminal=[])
    for pol in policies:
        st = s0.copy()
        x = first_observation(env_name, st).astype(np.float32)
        ret, g = np.zeros(N), 1.0
        live = np.ones(N, bool)
        L = np.full(N, H, np.int32)
        fo = np.zeros((N, x.shape[1]))
        acts, obs, rew, term = [], [], [], []
        for t in range(H):
            a = PR.mlp_actions(pol, x, lo, hi, discrete)
            if not discrete and a.shape[1] == 1:
                a = a[:, 0]
            o, r, d = R.oracle_steps(env_name, kw, st, a[None])
            o, r, d = o[0], r[0], d[0]
            st = _next_state(env_name, kw, st, a, o)
            ret = np.where(live, ret + g * r.astype(np.float64), ret)
            g = g * float(discount)
            fo[live] = o[live]
            L[live & d] = t + 1
            live = live & ~d
            x = o.astype(np.float32)
            acts.append(a), obs.append(o), rew.append(r), term.append(d)
        for k, v in (("ret", ret), ("L", L), ("final_obs", fo), ("actions", np.stack(acts)), ("obs", np.stack(obs)),
                     ("reward", np.stack(rew)), ("terminal", np.stack(term))):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def _next_state(env_name, kw, st, a, obs):
    """the state after the step oracle_steps just took: it returns observations, which are the state except for the pendulums'
    wrapped angles — those envs are stepped once more for their (unwrapped) state"""
    from oracle import oracle as O

    fam, variant = R.FAMILY[env_name]
    if fam not in ("ip", "dp"):
        return np.array(obs, np.float64)
    fr, dt = int(kw.get("freq_rate", 1)), float(kw.get("real_time_scale", 0.02))
    step = O.ip_step if fam == "ip" else O.dpend_step
    return step(variant, st, np.asarray(a, np.float32).astype(np.float64), fr, dt, R._opts(kw))[0]


# ------------------------------------------------------------------------------------------------ inputs
class Weights:
    """one member of a population for the twin: float32 arrays (w1 / b1 None: an affine policy)"""

    def __init__(self, w2, b2, w1=None, b1=None, out="clip"):
        self.w1, self.b1, self.w2, self.b2, self.out = w1, b1, w2, b2, out


def random_weights(rng, obs_dim, hidden, n_out, scale=1.5, bias=0.0, out="clip"):
    f = lambda *s: (rng.standard_normal(s) * scale / np.sqrt(s[-1])).astype(np.float32)
    b2 = f(n_out).reshape(n_out) + np.float32(bias)
    if hidden == 0:
        return Weights(f(n_out, obs_dim), b2, out=out)
    return Weights(f(n_out, hidden), b2, f(hidden, obs_dim), f(hidden).reshape(hidden), out=out)


def linear_as(hidden, gain, obs_dim):
    """the linear controller y = gain . x as a member of the given architecture: affine, or with ReLU units 0 and 1 carrying
    +-(gain . x) (relu(v) - relu(-v) = v) and the other units switched off by a negative bias"""
    gain = np.asarray(gain, np.float32)
    if hidden == 0:
        return Weights(gain[None, :].copy(), np.zeros(1, np.float32))
    assert hidden >= 2
    w1, b1 = np.zeros((hidden, obs_dim), np.float32), np.full(hidden, -1.0, np.float32)
    w1[0], w1[1], b1[:2] = gain, -gain, 0.0
    w2 = np.zeros((1, hidden), np.float32)
    w2[0, 0], w2[0, 1] = 1.0, -1.0
    return Weights(w2, np.zeros(1, np.float32), w1, b1)


def cartpole_balancing_population(hidden, seed=2):
    """P = 3 members that behave differently from uniform(-0.05, 0.05) starts: a pole-angle feedback that keeps every env up for
    40 steps, a random member (with the default seed its envs fall at many different steps, some not at all), and a member
    whose bias pushes one way until the pole falls (a dozen steps)"""
    rng = np.random.default_rng(seed + hidden)
    return [linear_as(hidden, [0.0, 0.0, 1.0, 0.3], 4), random_weights(rng, 4, hidden, 1), random_weights(rng, 4, hidden, 1, bias=3.0)]


def random_population(obs_dim, n_out, hidden, P, seed, out="clip", scale=1.5):
    rng = np.random.default_rng(seed + 31 * hidden)
    return [random_weights(rng, obs_dim, hidden, n_out, scale=scale, out=out) for _ in range(P)]


# the Hopper that terminates (plan_reference's "hopper-terminating" parameters: terminate_when_unhealthy=False is what makes the env
# terminate, hopper.py:104-106; with the default, True, no step is ever terminal)
HOPPER_TERMINATING = dict(R.MUJOCO, integrator="rk4", env_params=R._HOP_TERM)


def hopper_population(hidden, out="clip"):
    """P = 2 random members; from gpu_start's rows the first keeps every env healthy for 12 steps and the second drives some of them
    out of HOPPER_TERMINATING's healthy height range at different steps (tests/test_policy_population_reference.py shows it)"""
    return random_population(12, 3, hidden, 2, 506, out=out)


def gpu_start(env_name, N):
    """the start rows tests/test_gpu_policy_population.py gives an env: the input builders of plan_reference, one seed per family"""
    fam = R.FAMILY[env_name][0]
    kw = dict(z_spread=0.04) if fam == "hopper" else {}
    seed = {"cartpole": 501, "hopper": 502, "ip": 503, "dp": 504, "cheetah": 505}[fam]
    return R.BUILDERS[fam](env_name, N, 1, 1, seed, **kw)[0]
