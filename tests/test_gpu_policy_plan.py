"""emei_plan_policy on the GPU (Engine.plan_policy: pend_policy_plan_kernel / body_policy_plan_kernel, then plan_policy_finish_kernel).

The yardstick is the per-step twin.  For each candidate k the envs are put back to the start rows and stepped with step() under
policy(obs) (k = 0: candidate 0 takes no noise) or policy(obs, noise, t, candidate=k), whose exploration term is the DEVICE's own
draw (PolicyNoise.draws through emei_sample_candidates); the stacked [H, N, K] actions go to evaluate_sequences.  The call's returns
and lengths equal that composition bit for bit (out="clip" with a given std, and epsilon-greedy); on the HalfCheetah the returns are
held to 1e-9 relative, the project's documented lane-lending bound (the twin's wave-mates are not the call's), and the lengths are
equal.  Selection is recomputed from the call's own return_out under the planner's order.  The weighted mean and the effective
sample size are recomputed from the call's return_out and the twin's first actions with the header's case analysis and summation
tree (lane l adds k = l, l + 64, .. in ascending order, then the butterfly d = 1 .. 32) in float64 NumPy, the one transcendental —
exp((r_k - r*) / temperature) — taken from the device's own float64 exp (torch.exp on the device: the header defines the weights
with it), and must match bit for bit.

Shapes: (N = 3, K = 70) one env spanning two waves, (67, 5) segments straddling wave edges with a ragged last wave, (1, 1); H in
{1, 12}; hidden in {0, 5}.  A case runs once and is shared by the tests that read it."""
import ctypes as C
import functools

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
# env, engine kwargs, where the start rows come from ("reset": the handle's own reset, init noise included; "rows": the start rows
# tests/test_gpu_policy_population.py uses, which let episodes end inside H), discount, does an episode end inside H = 12
CASES = {
    "cartpole-balancing": dict(env="CartPoleBalancing", kw={}, start="rows", discount=1.0, ends=True),
    "ip-boundary-balancing-rk4": dict(env="BoundaryInvertedPendulumBalancing", kw=dict(integrator="rk4", init_noise=0.2), start="reset",
                                      discount=0.97, ends=True),
    "idp-ref": dict(env="ReboundInvertedDoublePendulumSwingUp", kw=dict(init_noise=0.05), start="reset", discount=0.99, ends=False),
    "idp-f32": dict(env="ReboundInvertedDoublePendulumSwingUp", kw=dict(init_noise=0.05, precision="f32"), start="reset", discount=1.0,
                    ends=False),
    "hopper-terminating": dict(env="HopperRunning", kw=dict(PP.HOPPER_TERMINATING), start="rows", discount=0.97, ends=True),
    "cheetah": dict(env="HalfCheetahRunning", kw=dict(init_noise=0.1, **BODY), start="reset", discount=0.99, ends=False),
}
# (case, N, K, H, hidden)
SHAPES = [
    ("cartpole-balancing", 3, 70, 12, 5), ("cartpole-balancing", 67, 5, 12, 0), ("cartpole-balancing", 67, 5, 1, 5),
    ("cartpole-balancing", 1, 1, 1, 0),
    ("ip-boundary-balancing-rk4", 3, 70, 12, 0), ("ip-boundary-balancing-rk4", 67, 5, 12, 5),
    ("idp-ref", 3, 70, 12, 5), ("idp-ref", 1, 1, 12, 0), ("idp-f32", 67, 5, 12, 0),
    ("hopper-terminating", 3, 70, 12, 5), ("hopper-terminating", 67, 5, 12, 0), ("hopper-terminating", 3, 70, 1, 0),
    ("cheetah", 3, 70, 1, 5), ("cheetah", 67, 5, 12, 0),
]
IDS = ["%s-N%d-K%d-H%d-h%d" % s for s in SHAPES]


def _engine(case, n, **over):
    from emei_amd.engine import Engine

    kw = dict(seed=11, env_index_offset=OFFSET)
    kw.update(CASES[case]["kw"])
    kw.update(over)
    eng = Engine(CASES[case]["env"], n, **kw)
    eng.reset(11)
    return eng


def _policy(eng, hidden, out="clip", seed=0, gain=1.5):
    from emei_amd.policy import MLPPolicy

    rng = np.random.default_rng(2000 + 17 * hidden + eng.obs_dim + seed)
    n_out = max(eng.act_dim, 1)
    f = lambda *s: (rng.standard_normal(s) * gain / np.sqrt(s[-1])).astype(np.float32)
    if hidden == 0:
        return MLPPolicy(f(n_out, eng.obs_dim), f(n_out).reshape(n_out), out=out)
    return MLPPolicy(f(n_out, hidden), f(n_out).reshape(n_out), f(hidden, eng.obs_dim), f(hidden).reshape(hidden), out=out)


def _noise(eng, seed=2 ** 64 - 5, zero=False):
    """a std per component (the Hopper's three: the odd Box-Muller pairing) or epsilon-greedy; the seed wraps inside H = 12"""
    from emei_amd.policy import PolicyNoise

    if eng.act_dim == 0:
        return PolicyNoise(seed, epsilon=0.0 if zero else EPSILON)
    n_out = eng.act_dim
    scale = 0.0 if zero else 1.0
    return PolicyNoise(seed, std=(scale * (0.2 + 0.3 * np.arange(1, n_out + 1, dtype=np.float32) / n_out)).astype(np.float32))


def _start(eng, case):
    if CASES[case]["start"] == "reset":
        st = eng.get_state().clone()
        if CASES[case]["env"] == "BoundaryInvertedPendulumBalancing":
            # the Balancing reward is 1 per step until the pole passes the horizontal (cos theta < 0) or the cart leaves the rail:
            # lean the poles (state [x, theta, xdot, thetadot]) by 0.3 .. 1.55 rad to either side, so that some candidates end
            # inside H, some do not, and the returns differ
            g = torch.Generator(device=eng.device).manual_seed(17)
            u = torch.rand((2, eng.n_envs), generator=g, device=eng.device, dtype=torch.float64)
            st[:, 1] = torch.where(u[0] < 0.5, -1.0, 1.0) * (0.3 + 1.25 * u[1])
        return st.contiguous()
    rows = PP.gpu_start(CASES[case]["env"], eng.n_envs).copy()
    if CASES[case]["env"] == "CartPoleBalancing":
        rows[:, 2] *= 3.0  # the pole up to 0.15 rad from upright: some candidates cross the 12 degrees inside H
    return torch.as_tensor(rows, device=eng.device, dtype=torch.float64).contiguous()


def _twin_actions(eng, pol, noise, start, H, K):
    """[H, N, K(, act_dim)]: candidate k's actions by the per-step loop from the start rows"""
    per_k = []
    for k in range(K):
        eng.set_state(start)
        x = eng.get_obs().to(torch.float32)
        seq = []
        for t in range(H):
            a = pol(x) if k == 0 else pol(x, noise, t, candidate=k)
            seq.append(a)
            x = eng.step(a)[0].clone()
        per_k.append(torch.stack(seq))
    eng.set_state(start)
    return torch.stack(per_k, dim=2).contiguous()


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


@functools.lru_cache(maxsize=None)
def _run(case, N, K, H, hidden):
    """one start: the twin's actions and their evaluate_sequences scores, the call with every output, evaluate_policies of the policy"""
    eng = _engine(case, N)
    pol, noise = _policy(eng, hidden).bind(eng), _noise(eng).bind(eng)
    gamma = CASES[case]["discount"]
    start = _start(eng, case)
    eng.set_state(start)
    acts = _twin_actions(eng, pol, noise, start, H, K)
    ret, length = eng.evaluate_sequences(acts, discount=gamma, start_state=start)
    T = _temperature(ret.cpu().numpy())
    out = eng.plan_policy(H, K, pol, noise, discount=gamma, temperature=T, start_state=start, returns=True, length=True, ess=True)
    names = ("best_action", "best_return", "best_index", "mean_action", "returns", "best_length", "ess")
    res = dict(zip(names, (t.cpu().numpy() for t in out)))
    # the device's float64 exp of the header's argument, for the weights
    r = res["returns"]
    rs = r[np.arange(N), res["best_index"]]
    with np.errstate(all="ignore"):
        arg = (r - rs[:, None]) / T
    res["exp"] = torch.exp(torch.as_tensor(arg, device=eng.device)).cpu().numpy()
    pret, plen = eng.evaluate_policies(pol, H, discount=gamma, start_state=start)
    res.update(acts=acts.cpu().numpy(), twin_ret=ret.cpu().numpy(), twin_len=length.cpu().numpy(), T=T, pol_ret=pret.cpu().numpy()[0],
               pol_len=plen.cpu().numpy()[0], cap_hits=eng.solver_cap_hits(), act_dim=eng.act_dim, cheetah=case == "cheetah")
    eng.close()
    return res


# ------------------------------------------------------------------------------------------------ 1. the returns against the twin
@pytest.mark.parametrize("case,N,K,H,hidden", SHAPES, ids=IDS)
def test_returns_equal_the_per_step_twin(case, N, K, H, hidden):
    r = _run(case, N, K, H, hidden)
    got, want = r["returns"], r["twin_ret"]
    assert got.shape == (N, K) and got.dtype == np.float64 and r["best_length"].dtype == np.int32
    best_len = r["twin_len"][np.arange(N), r["best_index"]]
    print(f"{case} N={N} K={K} H={H} hidden={hidden}: returns rel err {rel_err(got, want):.3e}, "
          f"{np.mean(_bits(got) != _bits(want)):.4f} of the returns differ in bits, lengths {r['twin_len'].min()} .. {r['twin_len'].max()}")
    if r["cheetah"]:
        assert rel_err(got, want) <= 1e-9
    else:
        assert _same(got, want)
    assert np.array_equal(r["best_length"], best_len)
    if K > 1:  # the candidates differ: the noise reached them, each under its own k
        a0 = r["acts"][0].reshape(N, K, -1)
        assert (a0[:, 1:] != a0[:, :1]).any()
    if CASES[case]["ends"] and H == 12 and N >= 67:  # enough different starts: episodes end inside H, and not all of them
        assert (r["twin_len"] < H).any() and (r["twin_len"] == H).any()
    assert r["cap_hits"] == 0


# ------------------------------------------------------------------------------------------------ 2. selection
@pytest.mark.parametrize("case,N,K,H,hidden", SHAPES, ids=IDS)
def test_selection_from_the_calls_own_returns(case, N, K, H, hidden):
    r = _run(case, N, K, H, hidden)
    best = SR.best_of(r["returns"])  # the planner's order: the first maximum, NaN last
    rows = np.arange(N)
    assert np.array_equal(r["best_index"], best.astype(np.int32)) and r["best_index"].dtype == np.int32
    assert _same(r["best_return"], r["returns"][rows, best])
    assert np.array_equal(r["best_length"], r["twin_len"][rows, best])
    want = r["acts"][0][rows, best]  # the twin's action of step 0: a pure function of (x_0, seed, g, k)
    assert r["best_action"].dtype == (np.int64 if r["act_dim"] == 0 else np.float32)
    assert _same(r["best_action"], want)


# ------------------------------------------------------------------------------------------------ 3. the weighted mean and the ESS
def _tree_sum(v):
    """[N, K] float64 -> [N]: lane l adds k = l, l + 64, .. in ascending order from 0.0, then the butterfly over the lanes"""
    lanes = np.zeros((v.shape[0], 64))
    for k in range(v.shape[1]):
        lanes[:, k % 64] = lanes[:, k % 64] + v[:, k]
    for d in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, np.arange(64) ^ d]
    return lanes[:, 0]


def _mean_and_ess(returns, best_return, exp, first):
    """(mean float32 [N, n_out], ess float64 [N]) of the header from the call's own returns [N, K], its best returns [N], the device's
    exp((r_k - r*) / temperature) [N, K] and the candidates' first actions [N, K, n_out] as float64"""
    rs = best_return[:, None]
    # tests/mppi_reference.py's case analysis, with the device's exp in its last branch
    with np.errstate(all="ignore"):
        w = np.where(np.isnan(rs), 1.0, np.where(np.isnan(returns), 0.0, np.where(returns == rs, 1.0, exp)))
    Z, Z2 = _tree_sum(w), _tree_sum(w * w)
    mean = np.stack([(_tree_sum(w * first[:, :, a]) / Z).astype(np.float32) for a in range(first.shape[2])], axis=1)
    return mean, Z * Z / Z2


@pytest.mark.parametrize("case,N,K,H,hidden", SHAPES, ids=IDS)
def test_mean_and_ess_by_the_headers_weights_and_tree(case, N, K, H, hidden):
    r = _run(case, N, K, H, hidden)
    first = r["acts"][0].reshape(N, K, -1).astype(np.float32).astype(np.float64)
    mean, ess = _mean_and_ess(r["returns"], r["best_return"], r["exp"], first)
    got = r["mean_action"].reshape(N, -1)
    print(f"{case} N={N} K={K} H={H} T={r['T']:.4g}: max |mean - ref| = {np.abs(got.astype(np.float64) - mean).max():.3e}, "
          f"ess rel err {np.abs(r['ess'] - ess).max():.3e}, ess {ess.min():.3f} .. {ess.max():.3f}")
    assert r["mean_action"].dtype == np.float32 and r["ess"].dtype == np.float64
    assert _same(got, mean)
    assert _same(r["ess"], ess)
    lo, hi = (0.0, 1.0) if r["act_dim"] == 0 else PR.ctrl_range(CASES[case]["env"])
    assert got.min() >= lo and got.max() <= hi and (ess >= 1.0).all() and (ess <= K).all()
    if K == 1:
        assert (ess == 1.0).all() and _same(got, first[:, 0].astype(np.float32))


# ------------------------------------------------------------------------------------------------ 4. candidate 0
@pytest.mark.parametrize("case,N,K,H,hidden", SHAPES, ids=IDS)
def test_candidate_zero_is_the_deterministic_policy(case, N, K, H, hidden):
    r = _run(case, N, K, H, hidden)
    got = r["returns"][:, 0]
    if r["cheetah"]:
        assert rel_err(got, r["pol_ret"]) <= 1e-9
    else:
        assert _same(got, r["pol_ret"])
    assert np.array_equal(r["twin_len"][:, 0], r["pol_len"])
    assert (r["best_return"] >= got).all()  # never worse than the prior under the model
    if K == 1:
        assert (r["best_index"] == 0).all() and np.array_equal(r["best_length"], r["pol_len"])


# ------------------------------------------------------------------------------------------------ 5. edge cases
@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating", "ip-boundary-balancing-rk4"])
def test_zero_noise_makes_every_candidate_the_policy(case):
    eng = _engine(case, 5)
    pol = _policy(eng, 5)
    start = _start(eng, case)
    act, bret, idx, rets, ln = eng.plan_policy(12, 70, pol, _noise(eng, zero=True), discount=0.9, start_state=start, returns=True, length=True)
    pret, plen = eng.evaluate_policies(pol, 12, discount=0.9, start_state=start)
    rets = rets.cpu().numpy()
    assert (rets == rets[:, :1]).all() and np.array_equal(rets[:, 0], pret[0].cpu().numpy())
    assert (idx == 0).all() and torch.equal(bret, pret[0]) and torch.equal(ln, plen[0])
    eng.set_state(start)
    assert torch.equal(act, pol(eng.get_obs().to(torch.float32)))
    # ... and K = 1 is the policy whatever the noise
    a1, r1, i1, l1 = eng.plan_policy(12, 1, pol, _noise(eng), discount=0.9, start_state=start, length=True)
    assert torch.equal(a1, act) and torch.equal(r1, pret[0]) and (i1 == 0).all() and torch.equal(l1, plen[0])
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. the call's contract
def _outputs(eng, H, K, pol, noise, **kw):
    return eng.plan_policy(H, K, pol, noise, returns=True, length=True, ess=True, **kw)


@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating"])
def test_handle_untouched(case):
    N = 96
    a, b = _engine(case, N, max_episode_steps=9), _engine(case, N, max_episode_steps=9)
    g = torch.Generator(device=a.device).manual_seed(9)
    step_acts = torch.randint(0, 2, (20, N), generator=g, device=a.device, dtype=torch.uint8) if a.act_dim == 0 \
        else torch.rand((20, N, a.act_dim), generator=g, device=a.device) * 2 - 1
    for e in (a, b):
        e.rollout(step_acts[:7], auto_reset=True)
        e.freeze()
        e.rollout(step_acts[7:12], auto_reset=True)
    kernel = a.last_kernel()
    _outputs(a, 12, 5, _policy(a, 5), _noise(a), discount=0.9, temperature=0.5)
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


@pytest.mark.parametrize("case", ["cartpole-balancing", "idp-f32"])
def test_start_state_argument_equals_set_state(case):
    eng = _engine(case, 67)
    pol, noise = _policy(eng, 5), _noise(eng)
    start = _start(eng, case) + 0.01
    want = _outputs(eng, 12, 5, pol, noise, discount=0.99, temperature=0.7, start_state=start)
    keep = eng.get_state().clone()
    assert torch.equal(keep, _engine(case, 67).get_state())  # the handle's own state is not the start
    eng.set_state(start)
    got = _outputs(eng, 12, 5, pol, noise, discount=0.99, temperature=0.7)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    eng.close()


@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating"])
def test_shards_give_the_whole(case):
    N, K, H = 134, 5, 12
    whole = _engine(case, N)
    pol, noise = _policy(whole, 5), _noise(whole)
    start = _start(whole, case)
    want = _outputs(whole, H, K, pol, noise, discount=0.97, temperature=0.6, start_state=start)
    got = []
    for o, n in ((0, 67), (67, 67)):
        part = _engine(case, n, env_index_offset=OFFSET + o)
        got.append(_outputs(part, H, K, _policy(part, 5), _noise(part), discount=0.97, temperature=0.6,
                            start_state=start[o:o + n].contiguous()))
        part.close()
    for q, w in enumerate(want):
        assert torch.equal(torch.cat([g[q] for g in got]), w), q
    assert not torch.equal(want[4][:67], want[4][67:])  # the shards do not simply repeat each other
    whole.close()


def _raw(eng, H, K, pol, noise, skip=None):
    """the ABI call with every optional output, or with `skip` NULL -> {name: tensor}"""
    from emei_amd import _lib as L
    from emei_amd.engine import _ACT_DTYPES, _ptr, _stream

    N = eng.n_envs
    pol.bind(eng)
    ps, ns = pol.struct(), noise.bind(eng).struct(pol.hidden if pol.hidden else pol.obs_dim)
    dtype = torch.int64 if eng.act_dim == 0 else torch.float32
    new = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=eng.device)
    out = dict(best_action=new((N,) + eng._act_tail, dtype), mean_action=new((N,) + eng._act_tail, torch.float32),
               best_return=new((N,), torch.float64), best_index=new((N,), torch.int32), best_length=new((N,), torch.int32),
               returns=new((N, K), torch.float64), ess=new((N,), torch.float64))
    p = {k: (None if k == skip else _ptr(v)) for k, v in out.items()}
    ws = torch.empty(L.lib().emei_plan_policy_workspace_bytes(N, K) // 8, dtype=torch.float64, device=eng.device)
    with torch.cuda.device(eng.device):
        L.check(L.lib().emei_plan_policy(eng._h, H, K, C.byref(ps), C.byref(ns), 0.97, 0.5, None, _ptr(ws), p["best_action"],
                                         _ACT_DTYPES[dtype], p["mean_action"], p["best_return"], p["best_index"], p["best_length"],
                                         p["returns"], p["ess"], _stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating"])
def test_null_outputs_one_at_a_time(case):
    eng = _engine(case, 67)
    pol, noise = _policy(eng, 5), _noise(eng)
    full = _raw(eng, 12, 5, pol, noise)
    assert all(not (v == 77).all() for v in full.values())
    for skip in ("mean_action", "best_return", "best_index", "best_length", "returns", "ess"):
        got = _raw(eng, 12, 5, pol, noise, skip=skip)
        for k, v in got.items():
            if k == skip:
                assert (v == 77).all(), k  # not written
            else:
                assert torch.equal(v, full[k]), (skip, k)
    eng.close()


def test_capture_replays_the_same_result():
    N, K, H = 67, 5, 12
    eng = _engine("hopper-terminating", N)
    pol, noise = _policy(eng, 5), _noise(eng)
    want = _outputs(eng, H, K, pol, noise, discount=0.99, temperature=0.4)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one linear chain: plan, finish
        got = _outputs(eng, H, K, pol, noise, discount=0.99, temperature=0.4)
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
@pytest.mark.parametrize("hidden", [5, 0])
@pytest.mark.parametrize("out", ["clip", "tanh"])
@pytest.mark.parametrize("case", ["hopper-terminating", "cheetah"])
def test_head_and_tanh_first_actions_within_the_derived_bounds(case, out, hidden):
    """(The two envs whose reward of the FIRST step depends on the action, through the control cost: on the pendulums every candidate
    ties at H = 1 and the winner is candidate 0, which takes no noise.)
    H = 1 and a temperature so cold that only the winner weighs: best_action and mean_action are candidate k*'s first action.  It
    lies within the bounds tests/test_gpu_policy_noise.py::test_head_teacher_forced derives for the numpy clause on the row the policy
    saw with the device's normals: under CLIP |a - a_ref| <= 2^-23 (s_ref |z| + |y_ref|) + the smallest subnormal; under TANH one
    spacing at max(|lo|, |hi|) plus half * 2^-23 * s_ref |z|.  Nothing is pinned bitwise here."""
    import types

    from emei_amd.policy import PolicyNoise

    N, K = 67, 5
    eng = _engine(case, N)
    pol = _policy(eng, hidden, out=out, seed=3, gain=0.3)  # small weights: the outputs stay off the ends of the ctrlrange
    n_out, n_in = eng.act_dim, hidden if hidden else eng.obs_dim
    rng = np.random.default_rng(5 + hidden)
    ws = (rng.standard_normal((n_out, n_in)) * 2.0 / np.sqrt(n_in)).astype(np.float32)
    bs = (rng.standard_normal(n_out) - 1.0).astype(np.float32)
    seed, rg = 424242, (-3.0, 0.5)
    noise = PolicyNoise(seed, log_std_head=(ws, bs), log_std_range=rg)
    nref = types.SimpleNamespace(mode="head", seed=seed, ws=ws, bs=bs, log_std_min=rg[0], log_std_max=rg[1])
    ref = types.SimpleNamespace(out=out, w1=None if pol.w1 is None else pol.w1.cpu().numpy(), b1=None if pol.b1 is None else pol.b1.cpu().numpy(),
                                w2=pol.w2.cpu().numpy(), b2=pol.b2.cpu().numpy())
    act, bret, idx, mean, rets = eng.plan_policy(1, K, pol, noise, temperature=1e-300, returns=True)
    idx = idx.cpu().numpy()
    x0 = eng.get_obs().to(torch.float32).cpu().numpy()
    z = np.stack([noise.draws(eng, 0, candidate=k).cpu().numpy().reshape(N, n_out) for k in range(K)], axis=1)  # [N, K, n_out]
    z[:, 0] = 0.0  # candidate 0 takes no noise
    zk = z[np.arange(N), idx]
    lo, hi = PR.ctrl_range(eng.env_name)
    yn, y, s = NR.noisy_logits(ref, nref, x0, zk)
    want = NR.output_clause(yn, out, lo, hi)
    got = act.cpu().numpy().reshape(N, n_out)
    sz = s.astype(np.float64) * np.abs(zk).astype(np.float64)
    if out == "clip":
        tol = 2.0 ** -23 * (sz + np.abs(y)) + float(np.finfo(np.float32).smallest_subnormal)
    else:
        tol = float(np.spacing(np.float32(max(abs(lo), abs(hi))))) + 0.5 * (float(hi) - float(lo)) * 2.0 ** -23 * sz
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{case} {out} hidden={hidden}: max |a - ref| = {err.max():.3e}, max err / bound = {(err / tol).max():.3f}, winners {np.bincount(idx, minlength=K)}")
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

    eng = Engine("HopperRunning", 4, **BODY)
    pol = _policy(eng, 5)
    with pytest.raises(AssertionError):  # EMEI_ERR_STATE: no reset yet and no start_state
        eng.plan_policy(3, 2, pol, _noise(eng))
    out = eng.plan_policy(3, 2, pol, _noise(eng), start_state=torch.zeros((4, eng.state_dim), dtype=torch.float64, device=eng.device))
    assert tuple(out[0].shape) == (4, 3)  # a start_state stands in for the state
    eng.reset(seed=0)
    # a noise mode that does not fit the env kind: refused by the library itself (the Python layer refuses it earlier, on bind)
    ps = pol.bind(eng).struct()
    ns = PolicyNoise(1, epsilon=0.1).struct()
    ws = torch.empty(L.lib().emei_plan_policy_workspace_bytes(4, 2) // 8, dtype=torch.float64, device=eng.device)
    act = torch.empty((4, 3), dtype=torch.float32, device=eng.device)

    def call(ns, dtype=L.ACT_F32, work=ws, act=act, K=2):
        with torch.cuda.device(eng.device):
            rc = L.lib().emei_plan_policy(eng._h, 3, K, C.byref(ps), C.byref(ns), 1.0, 1.0, None, _ptr(work), _ptr(act), dtype, None, None,
                                          None, None, None, None, _stream())
        return rc, L.lib().emei_last_error().decode()

    rc, msg = call(ns)
    assert rc == L.ERR_INVALID and msg.startswith("emei_plan_policy:") and "noise.mode" in msg, msg
    good = _noise(eng).bind(eng).struct()
    # ... after the dtype, the workspace and best_action_out, in the header's order
    for kw, word in ((dict(dtype=L.ACT_U8), "action_dtype"), (dict(work=None), "workspace"), (dict(act=None), "best_action_out"),
                     (dict(K=2 ** 30), "n_envs * n_candidates")):
        rc, msg = call(good, **kw)
        assert rc == L.ERR_INVALID and msg.startswith("emei_plan_policy:") and word in msg, (kw, msg)
        rc, msg = call(ns, **kw)
        assert word in msg, (kw, msg)
    assert call(good)[0] == L.OK
    with pytest.raises(ValueError, match="continuous"):
        eng.plan_policy(3, 2, pol, PolicyNoise(1, epsilon=0.1))
    cart = Engine("CartPoleSwingUp", 4)
    cart.reset(seed=0)
    with pytest.raises(ValueError, match="discrete"):
        cart.plan_policy(3, 2, _policy(cart, 0), PolicyNoise(1, std=0.1))
    cs = _policy(cart, 0).bind(cart).struct()
    gauss = PolicyNoise(1, std=0.1).struct()
    a8 = torch.empty(4, dtype=torch.uint8, device=cart.device)
    with torch.cuda.device(cart.device):
        rc = L.lib().emei_plan_policy(cart._h, 3, 2, C.byref(cs), C.byref(gauss), 1.0, 1.0, None, _ptr(ws), _ptr(a8), L.ACT_U8, None, None,
                                      None, None, None, None, _stream())
    assert rc == L.ERR_INVALID and "noise.mode" in L.lib().emei_last_error().decode()
    with pytest.raises(ValueError, match="ess=True needs a temperature"):
        eng.plan_policy(3, 2, pol, _noise(eng), ess=True)
    eng.close()
    cart.close()
