"""emei_plan_policy_deep on the GPU (Engine.plan_policy with a DeepMLPPolicy and, optionally, value=DeepValueFunction:
pend_policy_plan_deep_kernel / body_policy_plan_deep_kernel, then plan_policy_finish_kernel).

The yardstick is the per-step twin of tests/test_gpu_policy_plan.py.  For each candidate k the envs are put back to the start rows
and stepped with step() under policy(obs) (k = 0: candidate 0 takes no noise) or policy(obs, noise, t, candidate=k); the stacked
[H, N, K] actions go to evaluate_sequences(..., final_obs=True).  Without a value the call's returns and lengths equal that
composition bit for bit (out="clip" with a given std, and epsilon-greedy); on the HalfCheetah the returns are held to 1e-9 relative,
the project's documented lane-lending bound, and the lengths are equal.  With a value the twin return is
ret + g_H * float64(V(final_obs)) where no step of the candidate reported the terminal bit — g_H the float64 running product of the
discount over H steps, V DeepValueFunction.__call__, the arithmetic numpy float64 and unfused — and the same bounds hold against it.
Selection, the weighted mean and the effective sample size are recomputed from the call's own return_out with the header's case
analysis and summation tree, the one transcendental taken from the device's float64 exp.

Shapes: (N = 3, K = 70) one env spanning two waves, (67, 5) segments straddling wave edges with a ragged last wave, (1, 1); H in
{1, 12}; policy widths (5, 3) — a ragged last group of h1, h2 below the second-layer block of 4 — with a value of (9, 2), whose
first layer sizes the tile; (8, 5) — full groups, one full block and a ragged one — with a value of (3, 4), so that the policy
sizes the tile; and (1, 1).  A case runs once, with and without the value, and is shared by the tests that read it."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import policy_noise_reference as NR
import policy_population_reference as PP
import policy_reference as PR
import shooting_reference as SR
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BODY = dict(freq_rate=4, real_time_scale=0.002)
OFFSET = (1 << 32) + 7  # env_index_offset: the global env index reaches the second counter word
EPSILON = 0.3
# tests/test_gpu_policy_plan.py's CASES: env, engine kwargs, where the start rows come from, discount, does an episode end inside H = 12
CASES = {
    "cartpole-balancing": dict(env="CartPoleBalancing", kw={}, start="rows", discount=1.0, ends=True),
    "ip-boundary-balancing-rk4": dict(env="BoundaryInvertedPendulumBalancing", kw=dict(integrator="rk4", init_noise=0.2), start="reset",
                                      discount=0.97, ends=True),
    "idp-ref": dict(env="ReboundInvertedDoublePendulumSwingUp", kw=dict(init_noise=0.05), start="reset", discount=0.99, ends=False),
    "idp-f32": dict(env="ReboundInvertedDoublePendulumSwingUp", kw=dict(init_noise=0.05, precision="f32"), start="reset", discount=1.0,
                    ends=False),
    # pol_seed: with the default seed the random 8x5 network keeps every one of the 67 x 5 candidates healthy for 12 steps (seed 2 ends
    # them all); under seed 5, 92 of the 335 leave the healthy height range, in 43 envs next to candidates that do not
    "hopper-terminating": dict(env="HopperRunning", kw=dict(PP.HOPPER_TERMINATING), start="rows", discount=0.97, ends=True, pol_seed=5),
    "cheetah": dict(env="HalfCheetahRunning", kw=dict(init_noise=0.1, **BODY), start="reset", discount=0.99, ends=False),
}
VALUE_WIDTHS = {(5, 3): (9, 2), (8, 5): (3, 4), (1, 1): (9, 2), (256, 256): (256, 256)}
# (case, N, K, H, h1, h2)
SHAPES = [
    ("cartpole-balancing", 3, 70, 12, 5, 3), ("cartpole-balancing", 67, 5, 12, 8, 5), ("cartpole-balancing", 67, 5, 1, 1, 1),
    ("cartpole-balancing", 1, 1, 1, 5, 3),
    ("ip-boundary-balancing-rk4", 3, 70, 12, 8, 5), ("ip-boundary-balancing-rk4", 67, 5, 12, 5, 3),
    ("idp-ref", 3, 70, 12, 5, 3), ("idp-ref", 1, 1, 12, 8, 5), ("idp-f32", 67, 5, 12, 8, 5), ("idp-f32", 3, 70, 1, 1, 1),
    ("hopper-terminating", 3, 70, 12, 5, 3), ("hopper-terminating", 67, 5, 12, 8, 5), ("hopper-terminating", 3, 70, 1, 1, 1),
    ("cheetah", 3, 70, 1, 5, 3), ("cheetah", 67, 5, 12, 8, 5),
]
IDS = ["%s-N%d-K%d-H%d-h%dx%d" % s for s in SHAPES]
BOTH = pytest.mark.parametrize("valued", [False, True], ids=["plain", "value"])


def _engine(case, n, **over):
    from emei_amd.engine import Engine

    kw = dict(seed=11, env_index_offset=OFFSET)
    kw.update(CASES[case]["kw"])
    kw.update(over)
    eng = Engine(CASES[case]["env"], n, **kw)
    eng.reset(11)
    return eng


def _weights(eng, h1, h2, n_out, seed, gain):
    rng = np.random.default_rng(3000 + 17 * h1 + 5 * h2 + eng.obs_dim + seed)
    f = lambda *s: (rng.standard_normal(s) * gain / np.sqrt(s[-1])).astype(np.float32)
    return types.SimpleNamespace(w1=f(h1, eng.obs_dim), b1=f(h1).reshape(h1), w2=f(h2, h1), b2=f(h2).reshape(h2), w3=f(n_out, h2),
                                 b3=f(n_out).reshape(n_out))


def _policy(eng, h1, h2, out="clip", seed=0, gain=1.0):
    from emei_amd.policy import DeepMLPPolicy

    w = _weights(eng, h1, h2, max(eng.act_dim, 1), seed, gain)
    pol = DeepMLPPolicy(w.w3, w.b3, w.w2, w.b2, w.w1, w.b1, out=out)
    pol.numpy_weights = w
    return pol


def _value(eng, h1, h2, seed=0, gain=1.5):
    from emei_amd.policy import DeepValueFunction

    w = _weights(eng, h1, h2, 1, 500 + seed, gain)
    return DeepValueFunction(w.w3, w.b3, w.w2, w.b2, w.w1, w.b1)


def _noise(eng, seed=2 ** 64 - 5, zero=False):
    """a std per component (the Hopper's three: the odd Box-Muller pairing) or epsilon-greedy; the seed wraps inside H = 12"""
    from emei_amd.policy import PolicyNoise

    if eng.act_dim == 0:
        return PolicyNoise(seed, epsilon=0.0 if zero else EPSILON)
    n_out = eng.act_dim
    scale = 0.0 if zero else 1.0
    return PolicyNoise(seed, std=(scale * (0.2 + 0.3 * np.arange(1, n_out + 1, dtype=np.float32) / n_out)).astype(np.float32))


def _start(eng, case):
    """the start rows of tests/test_gpu_policy_plan.py: leaning poles, so that some candidates end inside H and some do not"""
    if CASES[case]["start"] == "reset":
        st = eng.get_state().clone()
        if CASES[case]["env"] == "BoundaryInvertedPendulumBalancing":
            g = torch.Generator(device=eng.device).manual_seed(17)
            u = torch.rand((2, eng.n_envs), generator=g, device=eng.device, dtype=torch.float64)
            st[:, 1] = torch.where(u[0] < 0.5, -1.0, 1.0) * (0.3 + 1.25 * u[1])
        return st.contiguous()
    rows = PP.gpu_start(CASES[case]["env"], eng.n_envs).copy()
    if CASES[case]["env"] == "CartPoleBalancing":
        rows[:, 2] *= 3.0  # the pole up to 0.15 rad from upright: some candidates cross the 12 degrees inside H
    return torch.as_tensor(rows, device=eng.device, dtype=torch.float64).contiguous()


def _twin_actions(eng, pol, noise, start, H, K):
    """([H, N, K(, act_dim)] candidate k's actions by the per-step loop from the start rows, [N, K] bool: did any of its steps report
    the terminal bit)"""
    per_k, ended = [], []
    for k in range(K):
        eng.set_state(start)
        x = eng.get_obs().to(torch.float32)
        seq, end = [], torch.zeros(eng.n_envs, dtype=torch.bool, device=eng.device)
        for t in range(H):
            a = pol(x) if k == 0 else pol(x, noise, t, candidate=k)
            seq.append(a)
            obs, _, done = eng.step(a)
            x = obs.clone()
            end = end | ((done & 1) != 0)
        per_k.append(torch.stack(seq))
        ended.append(end)
    eng.set_state(start)
    return torch.stack(per_k, dim=2).contiguous(), torch.stack(ended, dim=1).cpu().numpy()


def _g_H(gamma, H):
    g = np.float64(1.0)
    for _ in range(H):
        g = g * np.float64(gamma)
    return g


def _bootstrap(ret, ended, final_obs, value, gamma, H):
    """the value clause on the twin: ret + g_H * float64(V(x_H)) where no terminal bit was set, numpy float64, unfused"""
    N, K = ret.shape
    v = value(final_obs.reshape(N * K, -1)).cpu().numpy().reshape(N, K).astype(np.float64)
    with np.errstate(all="ignore"):
        tail = _g_H(gamma, H) * v
        return np.where(ended, ret, ret + tail)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _temperature(ret):
    sds = [np.std(r[np.isfinite(r)]) for r in ret if np.isfinite(r).any()]
    t = float(np.mean(sds)) if sds else 0.0
    return t if t > 0.0 else 1.0


NAMES = ("best_action", "best_return", "best_index", "mean_action", "returns", "best_length", "ess")


def _call(eng, H, K, pol, noise, value, gamma, T, start):
    out = eng.plan_policy(H, K, pol, noise, discount=gamma, temperature=T, start_state=start, returns=True, length=True, ess=True, value=value)
    res = dict(zip(NAMES, (t.cpu().numpy() for t in out)))
    r = res["returns"]
    rs = r[np.arange(r.shape[0]), res["best_index"]]
    with np.errstate(all="ignore"):
        arg = (r - rs[:, None]) / T
    res["exp"] = torch.exp(torch.as_tensor(arg, device=eng.device)).cpu().numpy()  # the device's float64 exp, for the weights
    res["T"] = T
    return res


@functools.lru_cache(maxsize=None)
def _run(case, N, K, H, h1, h2, env_kw=()):
    """one start: the twin's actions, their evaluate_sequences scores and the bootstrapped twin, the call without and with the value
    (every output), evaluate_policies of the policy"""
    eng = _engine(case, N, **dict(env_kw))
    pol, noise = _policy(eng, h1, h2, seed=CASES[case].get("pol_seed", 0)).bind(eng), _noise(eng).bind(eng)
    value = _value(eng, *VALUE_WIDTHS[(h1, h2)]).bind(eng)
    gamma = CASES[case]["discount"]
    start = _start(eng, case)
    eng.set_state(start)
    acts, ended = _twin_actions(eng, pol, noise, start, H, K)
    ret, length, fobs = eng.evaluate_sequences(acts, discount=gamma, start_state=start, final_obs=True)
    ret, length = ret.cpu().numpy(), length.cpu().numpy()
    assert ((length < H) <= ended).all()  # the twin's terminal bits cover the short lengths (one at the last step leaves length == H)
    boot = _bootstrap(ret, ended, fobs, value, gamma, H)
    pret, plen, pobs = eng.evaluate_policies(pol, H, discount=gamma, start_state=start, final_obs=True)
    pret, plen = pret.cpu().numpy()[0], plen.cpu().numpy()[0]
    pboot = _bootstrap(pret[:, None], ended[:, :1], pobs[0][:, None], value, gamma, H)[:, 0]
    plain = _call(eng, H, K, pol, noise, None, gamma, _temperature(ret), start)
    valued = _call(eng, H, K, pol, noise, value, gamma, _temperature(boot), start)
    plain.update(twin_ret=ret, pol_ret=pret)
    valued.update(twin_ret=boot, pol_ret=pboot)
    shared = dict(acts=acts.cpu().numpy(), twin_len=length, ended=ended, pol_len=plen, cap_hits=eng.solver_cap_hits(), act_dim=eng.act_dim,
                  cheetah=CASES[case]["env"] == "HalfCheetahRunning", plain=plain, valued=valued)
    eng.close()
    return shared


def _pick(r, valued):
    return r["valued" if valued else "plain"]


# ------------------------------------------------------------------------------------------------ 1. the returns against the twin
@BOTH
@pytest.mark.parametrize("case,N,K,H,h1,h2", SHAPES, ids=IDS)
def test_returns_equal_the_per_step_twin(case, N, K, H, h1, h2, valued):
    r = _run(case, N, K, H, h1, h2)
    c = _pick(r, valued)
    got, want = c["returns"], c["twin_ret"]
    assert got.shape == (N, K) and got.dtype == np.float64 and c["best_length"].dtype == np.int32
    print(f"{case} N={N} K={K} H={H} widths {h1}x{h2} value={valued}: returns rel err {rel_err(got, want):.3e}, "
          f"{np.mean(_bits(got) != _bits(want)):.4f} of the returns differ in bits, lengths {r['twin_len'].min()} .. {r['twin_len'].max()}, "
          f"{int(r['ended'].sum())} of {N * K} candidates terminated")
    if r["cheetah"]:
        assert rel_err(got, want) <= 1e-9
    else:
        assert _same(got, want)
    assert np.array_equal(c["best_length"], r["twin_len"][np.arange(N), c["best_index"]])  # L(i, k) is unchanged by the value
    if K > 1:  # the candidates differ: the noise reached them, each under its own k
        a0 = r["acts"][0].reshape(N, K, -1)
        assert (a0[:, 1:] != a0[:, :1]).any()
    if CASES[case]["ends"] and H == 12 and N >= 67:  # enough different starts: episodes end inside H, and not all of them
        assert (r["twin_len"] < H).any() and (r["twin_len"] == H).any()
        assert r["ended"].any() and not r["ended"].all()  # both kinds of candidate for the value clause
    assert r["cap_hits"] == 0


@pytest.mark.parametrize("case,N,K,H,h1,h2", SHAPES, ids=IDS)
def test_the_value_reaches_exactly_the_candidates_that_never_terminated(case, N, K, H, h1, h2):
    r = _run(case, N, K, H, h1, h2)
    a, b, ended = r["plain"]["returns"], r["valued"]["returns"], r["ended"]
    assert np.array_equal(_bits(a)[ended], _bits(b)[ended])  # a candidate that terminated gets nothing, the last step included
    if not ended.all():
        assert (_bits(a)[~ended] != _bits(b)[~ended]).any()
    else:
        assert _same(a, b)


# ------------------------------------------------------------------------------------------------ 2. selection
@BOTH
@pytest.mark.parametrize("case,N,K,H,h1,h2", SHAPES, ids=IDS)
def test_selection_from_the_calls_own_returns(case, N, K, H, h1, h2, valued):
    r = _run(case, N, K, H, h1, h2)
    c = _pick(r, valued)
    best = SR.best_of(c["returns"])  # the planner's order: the first maximum, NaN last
    rows = np.arange(N)
    assert np.array_equal(c["best_index"], best.astype(np.int32)) and c["best_index"].dtype == np.int32
    assert _same(c["best_return"], c["returns"][rows, best])
    assert np.array_equal(c["best_length"], r["twin_len"][rows, best])
    want = r["acts"][0][rows, best]  # the twin's action of step 0: a pure function of (x_0, seed, g, k)
    assert c["best_action"].dtype == (np.int64 if r["act_dim"] == 0 else np.float32)
    assert _same(c["best_action"], want)


# ------------------------------------------------------------------------------------------------ 3. the weighted mean and the ESS
def _tree_sum(v):
    """[N, K] float64 -> [N]: lane l adds k = l, l + 64, .. in ascending order from 0.0, then the butterfly over the lanes"""
    lanes = np.zeros((v.shape[0], 64))
    for k in range(v.shape[1]):
        lanes[:, k % 64] = lanes[:, k % 64] + v[:, k]
    for d in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, np.arange(64) ^ d]
    return lanes[:, 0]


@BOTH
@pytest.mark.parametrize("case,N,K,H,h1,h2", SHAPES, ids=IDS)
def test_mean_and_ess_by_the_headers_weights_and_tree(case, N, K, H, h1, h2, valued):
    r = _run(case, N, K, H, h1, h2)
    c = _pick(r, valued)
    ret = c["returns"]
    rs = c["best_return"][:, None]
    with np.errstate(all="ignore"):
        w = np.where(np.isnan(rs), 1.0, np.where(np.isnan(ret), 0.0, np.where(ret == rs, 1.0, c["exp"])))
    Z, Z2 = _tree_sum(w), _tree_sum(w * w)
    first = r["acts"][0].reshape(N, K, -1).astype(np.float32).astype(np.float64)
    mean = np.stack([(_tree_sum(w * first[:, :, a]) / Z).astype(np.float32) for a in range(first.shape[2])], axis=1)
    got = c["mean_action"].reshape(N, -1)
    ess = Z * Z / Z2
    print(f"{case} N={N} K={K} H={H} T={c['T']:.4g} value={valued}: max |mean - ref| = {np.abs(got.astype(np.float64) - mean).max():.3e}, "
          f"ess rel err {np.abs(c['ess'] - ess).max():.3e}, ess {ess.min():.3f} .. {ess.max():.3f}")
    assert c["mean_action"].dtype == np.float32 and c["ess"].dtype == np.float64
    assert _same(got, mean)
    assert _same(c["ess"], ess)
    lo, hi = (0.0, 1.0) if r["act_dim"] == 0 else PR.ctrl_range(CASES[case]["env"])
    assert got.min() >= lo and got.max() <= hi and (ess >= 1.0).all() and (ess <= K).all()
    if K == 1:
        assert (ess == 1.0).all() and _same(got, first[:, 0].astype(np.float32))


# ------------------------------------------------------------------------------------------------ 4. candidate 0
@BOTH
@pytest.mark.parametrize("case,N,K,H,h1,h2", SHAPES, ids=IDS)
def test_candidate_zero_is_the_deterministic_policy(case, N, K, H, h1, h2, valued):
    r = _run(case, N, K, H, h1, h2)
    c = _pick(r, valued)
    got = c["returns"][:, 0]  # against evaluate_policies of the deep policy (with a value: after adding the twin's term)
    if r["cheetah"]:
        assert rel_err(got, c["pol_ret"]) <= 1e-9
    else:
        assert _same(got, c["pol_ret"])
    assert np.array_equal(r["twin_len"][:, 0], r["pol_len"])
    assert (c["best_return"] >= got).all()  # never worse than the prior under the model
    if K == 1:
        assert (c["best_index"] == 0).all() and np.array_equal(c["best_length"], r["pol_len"])


# ------------------------------------------------------------------------------------------------ 5. at the cap: the 64 KiB tile
@pytest.mark.parametrize("case,env_kw", [("cartpole-balancing", ()), ("cheetah", ())], ids=["cartpole-balancing", "cheetah"])
def test_widths_256_for_policy_and_value(case, env_kw):
    """the launch that needs the opt-in for 64 KiB of dynamic LDS on the new kernels"""
    N, K, H = 3, 5, 1
    r = _run(case, N, K, H, 256, 256, env_kw)
    for valued in (False, True):
        c = _pick(r, valued)
        got, want = c["returns"], c["twin_ret"]
        print(f"{case} 256x256 value={valued}: returns rel err {rel_err(got, want):.3e}")
        if r["cheetah"]:
            assert rel_err(got, want) <= 1e-9
        else:
            assert _same(got, want)
        rows = np.arange(N)
        assert np.array_equal(c["best_length"], r["twin_len"][rows, c["best_index"]])
        assert _same(c["best_action"], r["acts"][0][rows, c["best_index"]])
    if not r["ended"].all():
        assert (_bits(r["plain"]["returns"])[~r["ended"]] != _bits(r["valued"]["returns"])[~r["ended"]]).any()
    assert r["cap_hits"] == 0


# ------------------------------------------------------------------------------------------------ 6. edge cases and the contract
def _pair(eng, seed=0):
    """a deep policy and a value whose first layer is the wider one, bound to `eng`"""
    return _policy(eng, 5, 3, seed=seed), _value(eng, 9, 2, seed=seed)


def _value_term(eng, value, obs, ended, gamma, H):
    v = value.bind(eng)(obs).cpu().numpy().astype(np.float64)
    return np.where(ended, 0.0, _g_H(gamma, H) * v)


@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating"])
def test_zero_noise_makes_every_candidate_the_policy(case):
    eng = _engine(case, 5)
    pol, value = _pair(eng)
    start = _start(eng, case)
    H, gamma = 12, 0.9
    act, bret, idx, rets, ln = eng.plan_policy(H, 70, pol, _noise(eng, zero=True), discount=gamma, start_state=start, returns=True,
                                               length=True, value=value)
    pret, plen, pobs = eng.evaluate_policies(pol, H, discount=gamma, start_state=start, final_obs=True)
    # the deterministic rollout's terminal bits: its per-step loop
    eng.set_state(start)
    x, ended = eng.get_obs().to(torch.float32), np.zeros(5, bool)
    for t in range(H):
        obs, _, done = eng.step(pol(x))
        x = obs.clone()
        ended |= ((done & 1) != 0).cpu().numpy()
    pr = pret[0].cpu().numpy()
    want = np.where(ended, pr, pr + _value_term(eng, value, pobs[0], ended, gamma, H))
    rets = rets.cpu().numpy()
    assert _same(rets[:, 0], want) and np.array_equal(_bits(rets), _bits(np.repeat(rets[:, :1], 70, axis=1)))
    assert (idx == 0).all() and _same(bret.cpu().numpy(), want) and torch.equal(ln, plen[0])
    eng.set_state(start)
    assert torch.equal(act, pol(eng.get_obs().to(torch.float32)))
    # ... and K = 1 is the policy whatever the noise
    a1, r1, i1, l1 = eng.plan_policy(H, 1, pol, _noise(eng), discount=gamma, start_state=start, length=True, value=value)
    assert torch.equal(a1, act) and _same(r1.cpu().numpy(), want) and (i1 == 0).all() and torch.equal(l1, plen[0])
    eng.close()


def _outputs(eng, H, K, pol, noise, value, **kw):
    return eng.plan_policy(H, K, pol, noise, returns=True, length=True, ess=True, value=value, **kw)


def test_handle_untouched():
    case, N = "hopper-terminating", 96
    a, b = _engine(case, N, max_episode_steps=9), _engine(case, N, max_episode_steps=9)
    g = torch.Generator(device=a.device).manual_seed(9)
    step_acts = torch.rand((20, N, a.act_dim), generator=g, device=a.device) * 2 - 1
    for e in (a, b):
        e.rollout(step_acts[:7], auto_reset=True)
        e.freeze()
        e.rollout(step_acts[7:12], auto_reset=True)
    kernel = a.last_kernel()
    pol, value = _pair(a)
    _outputs(a, 12, 5, pol, _noise(a), value, discount=0.9, temperature=0.5)
    assert a.last_kernel() == kernel == b.last_kernel()
    assert torch.equal(a.get_state(), b.get_state()) and torch.equal(a.compact_done(), b.compact_done())
    for x, y in zip(a.get_counters(), b.get_counters()):
        assert torch.equal(x, y)
    outs = [e.rollout(step_acts, auto_reset=True) for e in (a, b)]  # auto-reset: the reset key is the handle's own still
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    for e in (a, b):
        e.unfreeze()  # the snapshot is the one freeze() took
    assert torch.equal(a.get_state(), b.get_state())
    for e in (a, b):
        e.close()


def test_start_state_argument_equals_set_state():
    case = "cartpole-balancing"
    eng = _engine(case, 67)
    (pol, value), noise = _pair(eng), _noise(eng)
    start = _start(eng, case) + 0.01
    want = _outputs(eng, 12, 5, pol, noise, value, discount=0.99, temperature=0.7, start_state=start)
    assert torch.equal(eng.get_state(), _engine(case, 67).get_state())  # the handle's own state is not the start
    eng.set_state(start)
    got = _outputs(eng, 12, 5, pol, noise, value, discount=0.99, temperature=0.7)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    eng.close()


def test_shards_give_the_whole():
    case, N, K, H = "hopper-terminating", 134, 5, 12
    whole = _engine(case, N)
    (pol, value), noise = _pair(whole), _noise(whole)
    start = _start(whole, case)
    want = _outputs(whole, H, K, pol, noise, value, discount=0.97, temperature=0.6, start_state=start)
    got = []
    for o, n in ((0, 67), (67, 67)):
        part = _engine(case, n, env_index_offset=OFFSET + o)
        p, v = _pair(part)
        got.append(_outputs(part, H, K, p, _noise(part), v, discount=0.97, temperature=0.6, start_state=start[o:o + n].contiguous()))
        part.close()
    for q, w in enumerate(want):
        assert torch.equal(torch.cat([g[q] for g in got]), w), q
    assert not torch.equal(want[4][:67], want[4][67:])  # the shards do not simply repeat each other
    whole.close()


def _raw(eng, H, K, pol, noise, value, skip=None):
    """the ABI call with every optional output, or with `skip` NULL -> {name: tensor}"""
    from emei_amd import _lib as L
    from emei_amd.engine import _ACT_DTYPES, _ptr, _stream

    N = eng.n_envs
    ps, ns, vs = pol.bind(eng).struct(), noise.bind(eng).struct(pol.hidden2), value.bind(eng).struct()
    dtype = torch.int64 if eng.act_dim == 0 else torch.float32
    new = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=eng.device)
    out = dict(best_action=new((N,) + eng._act_tail, dtype), mean_action=new((N,) + eng._act_tail, torch.float32),
               best_return=new((N,), torch.float64), best_index=new((N,), torch.int32), best_length=new((N,), torch.int32),
               returns=new((N, K), torch.float64), ess=new((N,), torch.float64))
    p = {k: (None if k == skip else _ptr(v)) for k, v in out.items()}
    ws = torch.empty(L.lib().emei_plan_policy_workspace_bytes(N, K) // 8, dtype=torch.float64, device=eng.device)
    with torch.cuda.device(eng.device):
        L.check(L.lib().emei_plan_policy_deep(eng._h, H, K, C.byref(ps), C.byref(ns), C.byref(vs), 0.97, 0.5, None, _ptr(ws), p["best_action"],
                                              _ACT_DTYPES[dtype], p["mean_action"], p["best_return"], p["best_index"], p["best_length"],
                                              p["returns"], p["ess"], _stream()))
    torch.cuda.synchronize()
    return out


def test_null_outputs_one_at_a_time():
    eng = _engine("cartpole-balancing", 67)
    eng.set_state(_start(eng, "cartpole-balancing"))
    (pol, value), noise = _pair(eng), _noise(eng)
    full = _raw(eng, 12, 5, pol, noise, value)
    assert all(not (v == 77).all() for v in full.values())
    for skip in ("mean_action", "best_return", "best_index", "best_length", "returns", "ess"):
        got = _raw(eng, 12, 5, pol, noise, value, skip=skip)
        for k, v in got.items():
            if k == skip:
                assert (v == 77).all(), k  # not written
            else:
                assert torch.equal(v, full[k]), (skip, k)
    eng.close()


def test_capture_replays_the_same_result():
    N, K, H = 67, 5, 12
    eng = _engine("hopper-terminating", N)
    (pol, value), noise = _pair(eng), _noise(eng)
    want = _outputs(eng, H, K, pol, noise, value, discount=0.99, temperature=0.4)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one linear chain: plan, finish
        got = _outputs(eng, H, K, pol, noise, value, discount=0.99, temperature=0.4)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for x in got:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. TANH and GAUSS_HEAD at H = 1
@pytest.mark.parametrize("out", ["clip", "tanh"])
@pytest.mark.parametrize("case", ["hopper-terminating", "cheetah"])
def test_head_and_tanh_first_actions_within_the_derived_bounds(case, out):
    """tests/test_gpu_policy_plan.py section 7 on the deep network, the head reading h2: H = 1 and a temperature so cold that only the
    winner weighs, so best_action and mean_action are candidate k*'s first action.  It lies within the bounds derived there for the
    numpy clause on the row the policy saw with the device's normals: under CLIP |a - a_ref| <= 2^-23 (s_ref |z| + |y_ref|) + the
    smallest subnormal; under TANH one spacing at max(|lo|, |hi|) plus half * 2^-23 * s_ref |z|.  Nothing is pinned bitwise here."""
    from emei_amd.policy import PolicyNoise

    N, K, h1, h2 = 67, 5, 8, 5
    eng = _engine(case, N)
    pol = _policy(eng, h1, h2, out=out, seed=3, gain=0.6)  # small weights: the outputs stay off the ends of the ctrlrange
    w = pol.numpy_weights
    n_out = eng.act_dim
    rng = np.random.default_rng(5 + h2)
    ws = (rng.standard_normal((n_out, h2)) * 2.0 / np.sqrt(h2)).astype(np.float32)
    bs = (rng.standard_normal(n_out) - 1.0).astype(np.float32)
    seed, rg = 424242, (-3.0, 0.5)
    noise = PolicyNoise(seed, log_std_head=(ws, bs), log_std_range=rg)
    nref = types.SimpleNamespace(mode="head", seed=seed, ws=ws, bs=bs, log_std_min=rg[0], log_std_max=rg[1])
    act, bret, idx, mean, rets = eng.plan_policy(1, K, pol, noise, temperature=1e-300, returns=True, value=_value(eng, 3, 4))
    idx = idx.cpu().numpy()
    x0 = eng.get_obs().to(torch.float32).cpu().numpy()
    z = np.stack([noise.draws(eng, 0, candidate=k).cpu().numpy().reshape(N, n_out) for k in range(K)], axis=1)  # [N, K, n_out]
    z[:, 0] = 0.0  # candidate 0 takes no noise
    zk = z[np.arange(N), idx]
    lo, hi = PR.ctrl_range(eng.env_name)
    # tests/policy_reference.py's ascending sums serve the deep net once the first layer is applied: its hidden layer is the deep
    # net's second, its input the deep net's h1 — which is what the head reads through
    first = types.SimpleNamespace(w1=None, b1=None, w2=w.w1, b2=w.b1)
    zz = PR.mlp_logits(first, x0).astype(np.float32)
    h1_rows = np.where(zz > np.float32(0), zz, np.float32(0))
    pseudo = types.SimpleNamespace(out=out, w1=w.w2, b1=w.b2, w2=w.w3, b2=w.b3)
    yn, y, s = NR.noisy_logits(pseudo, nref, h1_rows, zk)
    want = NR.output_clause(yn, out, lo, hi)
    got = act.cpu().numpy().reshape(N, n_out)
    sz = s.astype(np.float64) * np.abs(zk).astype(np.float64)
    if out == "clip":
        tol = 2.0 ** -23 * (sz + np.abs(y)) + float(np.finfo(np.float32).smallest_subnormal)
    else:
        tol = float(np.spacing(np.float32(max(abs(lo), abs(hi))))) + 0.5 * (float(hi) - float(lo)) * 2.0 ** -23 * sz
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{case} {out}: max |a - ref| = {err.max():.3e}, max err / bound = {(err / tol).max():.3f}, winners {np.bincount(idx, minlength=K)}")
    assert (err <= tol).all(), float((err - tol).max())
    # only the maximisers weigh at this temperature: where the winner is alone, the mean is its action
    rets = rets.cpu().numpy()
    alone = (rets == rets[np.arange(N), idx][:, None]).sum(1) == 1
    assert alone.any() and np.array_equal(mean.cpu().numpy().reshape(N, n_out)[alone], got[alone])
    assert len(np.unique(idx)) > 1  # the noise decides the winner
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. refusals that need a handle
def test_refusals_on_a_handle():
    from emei_amd import _lib as L
    from emei_amd.engine import Engine, _ptr, _stream
    from emei_amd.policy import PolicyNoise

    FN = "emei_plan_policy_deep:"
    eng = Engine("HopperRunning", 4, **BODY)
    pol, value = _pair(eng)
    with pytest.raises(AssertionError):  # EMEI_ERR_STATE: no reset yet and no start_state
        eng.plan_policy(3, 2, pol, _noise(eng), value=value)
    out = eng.plan_policy(3, 2, pol, _noise(eng), value=value,
                          start_state=torch.zeros((4, eng.state_dim), dtype=torch.float64, device=eng.device))
    assert tuple(out[0].shape) == (4, 3)  # a start_state stands in for the state
    eng.reset(seed=0)
    # a noise mode that does not fit the env kind: refused by the library itself (the Python layer refuses it earlier, on bind)
    ps, vs = pol.bind(eng).struct(), value.bind(eng).struct()
    ns = PolicyNoise(1, epsilon=0.1).struct()
    ws = torch.empty(L.lib().emei_plan_policy_workspace_bytes(4, 2) // 8, dtype=torch.float64, device=eng.device)
    act = torch.empty((4, 3), dtype=torch.float32, device=eng.device)

    def call(ns, dtype=L.ACT_F32, work=ws, act=act, K=2):
        with torch.cuda.device(eng.device):
            rc = L.lib().emei_plan_policy_deep(eng._h, 3, K, C.byref(ps), C.byref(ns), C.byref(vs), 1.0, 1.0, None, _ptr(work), _ptr(act),
                                               dtype, None, None, None, None, None, None, _stream())
        return rc, L.lib().emei_last_error().decode()

    rc, msg = call(ns)
    assert rc == L.ERR_INVALID and msg.startswith(FN) and "noise.mode" in msg, msg
    good = _noise(eng).bind(eng).struct()
    # ... after n_envs * n_candidates, the dtype, the workspace and best_action_out, in the header's order
    for kw, word in ((dict(dtype=L.ACT_U8), "action_dtype"), (dict(work=None), "workspace"), (dict(act=None), "best_action_out"),
                     (dict(K=2 ** 30), "n_envs * n_candidates")):
        rc, msg = call(good, **kw)
        assert rc == L.ERR_INVALID and msg.startswith(FN) and word in msg, (kw, msg)
        rc, msg = call(ns, **kw)
        assert word in msg, (kw, msg)
    assert "n_envs * n_candidates" in call(good, K=2 ** 30, dtype=L.ACT_U8, work=None, act=None)[1]
    assert "action_dtype" in call(good, dtype=L.ACT_U8, work=None, act=None)[1]
    assert "workspace" in call(good, work=None, act=None)[1]
    assert call(good)[0] == L.OK
    with pytest.raises(ValueError, match="continuous"):
        eng.plan_policy(3, 2, pol, PolicyNoise(1, epsilon=0.1), value=value)
    cart = Engine("CartPoleSwingUp", 4)
    cart.reset(seed=0)
    cpol, cval = _pair(cart)
    with pytest.raises(ValueError, match="discrete"):
        cart.plan_policy(3, 2, cpol, PolicyNoise(1, std=0.1), value=cval)
    cs, cv = cpol.bind(cart).struct(), cval.bind(cart).struct()
    gauss = PolicyNoise(1, std=0.1).struct()
    a8 = torch.empty(4, dtype=torch.uint8, device=cart.device)
    with torch.cuda.device(cart.device):
        rc = L.lib().emei_plan_policy_deep(cart._h, 3, 2, C.byref(cs), C.byref(gauss), C.byref(cv), 1.0, 1.0, None, _ptr(ws), _ptr(a8),
                                           L.ACT_U8, None, None, None, None, None, None, _stream())
    assert rc == L.ERR_INVALID and "noise.mode" in L.lib().emei_last_error().decode()
    with pytest.raises(ValueError, match="ess=True needs a temperature"):
        eng.plan_policy(3, 2, pol, _noise(eng), ess=True, value=value)
    with pytest.raises(ValueError, match="two-hidden-layer call"):
        from emei_amd.policy import MLPPolicy

        eng.plan_policy(3, 2, MLPPolicy(torch.zeros(3, 11), torch.zeros(3)), _noise(eng), value=value)
    eng.close()
    cart.close()
