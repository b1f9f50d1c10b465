"""emei_evaluate_policies on the GPU (pend_policy_eval_kernel / body_policy_eval_kernel).

The reference is the REPLAY route of the header's stated consequence, built from two calls existing tests already pin to the CPU
oracle: for each member p, set_state(start) and rollout_policy(H, pop[p], auto_reset=False) give the actions the policy takes;
stacked as [H, N, P] candidates, evaluate_sequences(final_obs=True) from the same start scores them.  evaluate_policies must give
the same lengths, returns and final observations, transposed — bit for bit, except on the HalfCheetah, whose constraint-slot lending
makes a lane depend on its wave-mates (they differ between the [N, P] candidate layout and the policy-major one): there the returns
are held to 1e-9 relative, the bound the header documents, the lengths stay equal, and a final observation (float32) may round the
other way: one float32 spacing.

Shapes: N = 130 on the 4-state envs (one 256-thread block per policy: two full waves and a ragged one of 2 lanes), P = 3 distinct
members, hidden in {0, 5}, H = 40; on the bodies N = 70 (a full wave and a ragged one), P = 2, H = 12.  A case runs once and is shared
by the tests that read it.  Start rows and weights come from tests/policy_population_reference.py, where the CPU oracle shows that
they exercise the early exit (tests/test_policy_population_reference.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import plan_reference as R
import policy_population_reference as PP
import policy_reference as PR
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BODY = dict(R.MUJOCO)
# name -> (env id, Engine keyword arguments, N, P, H)
CASES = {
    "cartpole-balancing": ("CartPoleBalancing", {}, 130, 3, 40),
    "cartpole-swingup-rk4": ("CartPoleSwingUp", dict(ode_method="rk4"), 130, 3, 40),
    "ip-rebound-balancing": ("ReboundInvertedPendulumBalancing", {}, 130, 3, 40),
    "idp-rk4": ("ReboundInvertedDoublePendulumSwingUp", dict(integrator="rk4"), 70, 2, 12),
    "idp-rk4-f32": ("ReboundInvertedDoublePendulumSwingUp", dict(integrator="rk4", precision="f32"), 70, 2, 12),
    "hopper": ("HopperRunning", dict(BODY), 70, 2, 12),  # default parameters: no step is ever terminal (hopper.py:104-106)
    "hopper-terminating": ("HopperRunning", dict(PP.HOPPER_TERMINATING), 70, 2, 12),
    "cheetah": ("HalfCheetahRunning", dict(BODY), 70, 2, 12),
}
REPLAY = [(c, h) for c in CASES for h in (0, 5) if c != "idp-rk4-f32"] + [("idp-rk4-f32", 5)]


def _engine(case, n=None, **over):
    from emei_amd.engine import Engine

    name, kw, N = CASES[case][:3]
    return Engine(name, n or N, **dict(dict(seed=11, env_index_offset=4000, **kw), **over))


def _weights(case, hidden, out="clip"):
    """the members of the case's population as policy_population_reference.Weights"""
    name, _, _, P, _ = CASES[case]
    if case == "cartpole-balancing":
        return PP.cartpole_balancing_population(hidden)
    if name == "HopperRunning":
        return PP.hopper_population(hidden, out)
    obs_dim, n_out = {"CartPoleSwingUp": (4, 1), "ReboundInvertedPendulumBalancing": (4, 1), "ReboundInvertedDoublePendulumSwingUp": (6, 1),
                      "HalfCheetahRunning": (18, 6)}[name]
    return PP.random_population(obs_dim, n_out, hidden, P, 600 + len(case), out=out)


def _population(weights):
    from emei_amd.policy import MLPPolicy, PolicyPopulation

    return PolicyPopulation.from_policies([MLPPolicy(w.w2, w.b2, w.w1, w.b1, out=w.out) for w in weights])


def _start(case, eng):
    return torch.as_tensor(PP.gpu_start(CASES[case][0], eng.n_envs), device=eng.device)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _np(ts):
    return tuple(t.cpu().numpy() for t in ts)


def _replay(eng, pop, start, H, discount):
    """the reference route -> (ret [P, N], L [P, N], final_obs [P, N, obs_dim], actions [P, H, N(, act_dim)]) as numpy arrays"""
    acts = []
    for p in range(len(pop)):
        eng.set_state(start)
        acts.append(eng.rollout_policy(H, pop[p], auto_reset=False)[0])
    cand = torch.stack(acts, dim=2).contiguous()  # [H, N, P(, act_dim)]
    eng.set_state(start)
    ret, L, fo = eng.evaluate_sequences(cand, discount=discount, start_state=None, final_obs=True)
    return _np((ret.T.contiguous(), L.T.contiguous(), fo.transpose(0, 1).contiguous(), torch.stack(acts)))


def _run(case, hidden, discount=1.0, out="clip"):
    return _run_once(case, hidden, float(discount), out)


@functools.lru_cache(maxsize=None)
def _run_once(case, hidden, discount, out):
    _, _, N, P, H = CASES[case]
    eng = _engine(case)
    weights = _weights(case, hidden, out)
    pop = _population(weights)
    start = _start(case, eng)
    ref = _replay(eng, pop, start, H, discount)
    eng.set_state(start)
    got = _np(eng.evaluate_policies(pop, H, discount=discount, final_obs=True))
    eng.close()
    for a in ref + got:
        a.setflags(write=False)
    return dict(ref=ref, got=got, weights=weights)


def _check_replay(case, r):
    _, _, N, P, H = CASES[case]
    (ret, L, fo), (e_ret, e_L, e_fo, _) = r["got"], r["ref"]
    assert ret.shape == (P, N) and ret.dtype == np.float64 and L.shape == (P, N) and L.dtype == np.int32
    assert fo.shape == e_fo.shape == (P, N, fo.shape[2]) and fo.dtype == np.float32
    assert np.array_equal(L, e_L)
    if case == "cheetah":
        print(f"{case}: returns rel_err {rel_err(ret, e_ret):.3e} (bound 1e-9), final_obs rel_err {rel_err(fo, e_fo):.3e} (bound 2^-23)")
        assert rel_err(ret, e_ret) <= 1e-9
        assert rel_err(fo, e_fo) <= 2.0 ** -23
    else:
        assert _same(ret, e_ret) and _same(fo, e_fo)


@pytest.mark.parametrize("case,hidden", REPLAY)
def test_replay_identity(case, hidden):
    _check_replay(case, _run(case, hidden))


@pytest.mark.parametrize("hidden", [0, 5])
@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating"])
def test_the_early_exit_is_exercised(case, hidden):
    """on the REFERENCE's lengths: pairs that end before the horizon and pairs that run all of it; and the members are told apart.
    (The Hopper terminates only with terminate_when_unhealthy=False; with the default no step is ever terminal, and the default
    case "hopper" of the replay test accordingly has every length equal to H: asserted below, also on the reference.)"""
    H, P = CASES[case][4], CASES[case][3]
    r = _run(case, hidden)
    e_ret, e_L = r["ref"][0], r["ref"][1]
    assert (e_L < H).any() and (e_L == H).any()
    for p in range(P):
        for q in range(p):
            assert not np.array_equal(e_ret[p], e_ret[q]), (p, q)
    _check_replay(case, r)
    if case == "hopper-terminating":
        assert (_run("hopper", hidden)["ref"][1] == H).all()


@pytest.mark.parametrize("hidden", [0, 5])
def test_against_the_numpy_twin(hidden):
    """CartPoleBalancing, every env and member: the lengths of the CPU twin, its returns within the per-step reward tolerance the
    plan-oracle test uses (plan_reference.ret_bound: 1e-5 per counted discounted step)"""
    case = "cartpole-balancing"
    name, kw, N, P, H = CASES[case]
    for discount in (1.0, 0.95):
        r = _run(case, hidden, discount)
        twin = PP.evaluate_policies(name, kw, PP.gpu_start(name, N), r["weights"], H, discount)
        ret, L, fo = r["got"]
        assert np.array_equal(L, twin["L"])
        for p in range(P):
            bound = R.ret_bound(twin["reward"][p], twin["L"][p], discount, R.TOL_R["cartpole"])
            ratio = (np.abs(ret[p] - twin["ret"][p]) / bound).max()
            print(f"hidden {hidden} discount {discount} member {p}: worst |ret - twin| / bound = {ratio:.3e}")
            assert ratio <= 1.0
        assert rel_err(fo, twin["final_obs"]) <= R.TOL_OBS


@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating"])
def test_the_handle_is_untouched(case):
    from emei_amd.policy import MLPPolicy

    _, _, N, P, H = CASES[case]
    eng = _engine(case, max_episode_steps=5)
    pop = _population(_weights(case, 5))
    eng.reset(3)
    stepper = MLPPolicy(pop[1].w2.clone(), pop[1].b2.clone(), pop[1].w1.clone(), pop[1].b1.clone())
    eng.rollout_policy(7, stepper, auto_reset=True)  # counters, episodes and a done mask that are not the initial ones
    frozen = eng.get_state().clone()
    eng.freeze()
    eng.rollout_policy(5, stepper, auto_reset=False)  # ends on the TimeLimit: compact_done() is not empty

    def snapshot():
        steps, epi = eng.get_counters()
        return _np((eng.get_state(), steps, epi, eng.compact_done())) + (eng.last_kernel(),)

    before = snapshot()
    assert before[3].size > 0 and before[1].any() and before[2].any()
    out = eng.evaluate_policies(pop, H, discount=0.9, final_obs=True)
    other = eng.evaluate_policies(pop, H, discount=0.9, start_state=_start(case, eng), final_obs=True)
    torch.cuda.synchronize()
    assert not torch.equal(out[0], other[0])
    after = snapshot()
    for a, b in zip(before[:4], after[:4]):
        assert _same(a, b)
    assert before[4] == after[4]
    eng.unfreeze()  # the frozen snapshot is what it was
    assert torch.equal(eng.get_state(), frozen)
    eng.close()


@pytest.mark.parametrize("case", ["cartpole-swingup-rk4", "idp-rk4-f32", "cheetah"])
def test_start_state_argument_equals_set_state(case):
    _, _, N, P, H = CASES[case]
    eng = _engine(case)
    pop = _population(_weights(case, 5))
    eng.reset(1)
    rows = _start(case, eng)
    given = eng.evaluate_policies(pop, H, discount=0.97, start_state=rows, final_obs=True)
    assert not torch.equal(eng.get_state(), rows)
    eng.set_state(rows)
    current = eng.evaluate_policies(pop, H, discount=0.97, final_obs=True)
    for x, y in zip(given, current):
        assert torch.equal(x, y)
    eng.close()


@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating"])
def test_a_population_of_one_equals_the_policy_itself(case):
    import emei_amd

    _, _, N, P, H = CASES[case]
    eng = _engine(case)
    pop = _population(_weights(case, 5))
    eng.set_state(_start(case, eng))
    whole = eng.evaluate_policies(pop, H, final_obs=True)
    for p in range(P):
        member = pop[p]
        assert isinstance(member, emei_amd.MLPPolicy)
        alone = eng.evaluate_policies(member, H, final_obs=True)
        one = eng.evaluate_policies(emei_amd.PolicyPopulation.from_policies([member]), H, final_obs=True)
        for w, a, o in zip(whole, alone, one):
            assert tuple(a.shape[:2]) == (1, N) and torch.equal(a, o) and torch.equal(a[0], w[p]), p
    assert len(eng.evaluate_policies(pop, H)) == 2
    eng.close()


@pytest.mark.parametrize("case,hidden", [("cartpole-balancing", 5), ("ip-rebound-balancing", 0), ("hopper-terminating", 0)])
def test_discount_below_one(case, hidden):
    r = _run(case, hidden, 0.9)
    _check_replay(case, r)
    assert not np.array_equal(r["got"][0], _run(case, hidden)["got"][0])


@pytest.mark.parametrize("case", ["cartpole-balancing", "hopper-terminating"])
def test_null_outputs_one_at_a_time(case):
    from emei_amd import _lib as L
    from emei_amd.engine import _ptr, _stream

    _, _, N, P, H = CASES[case]
    full = _run(case, 5)["got"]
    eng = _engine(case)
    pop = _population(_weights(case, 5)).bind(eng)
    eng.set_state(_start(case, eng))
    for skip in ("length", "final_obs"):
        bufs = dict(ret=torch.empty((P, N), dtype=torch.float64, device=eng.device),
                    length=torch.empty((P, N), dtype=torch.int32, device=eng.device),
                    final_obs=torch.empty((P, N, eng.obs_dim), dtype=torch.float32, device=eng.device))
        p = {k: (None if k == skip else _ptr(v)) for k, v in bufs.items()}
        ps = pop.struct()
        with torch.cuda.device(eng.device):
            L.check(L.lib().emei_evaluate_policies(eng._h, H, P, C.byref(ps), 1.0, None, p["ret"], p["length"], p["final_obs"], _stream()))
        torch.cuda.synchronize()
        for k, want in zip(("ret", "length", "final_obs"), full):
            if k != skip:
                assert _same(bufs[k].cpu().numpy(), want), (skip, k)
    eng.close()


@pytest.mark.parametrize("case", ["cartpole-balancing", "idp-rk4"])
def test_shard_invariance(case):
    """envs [0, 64) and [64, 130) as two engines with env_index_offset against one engine of 130"""
    _, _, _, P, H = CASES[case]
    N = 130
    rows = PP.gpu_start(CASES[case][0], N)
    weights = _weights(case, 5)
    outs = []
    for parts in (((0, 130),), ((0, 64), (64, 130))):
        got = []
        for lo, hi in parts:
            eng = _engine(case, n=hi - lo, env_index_offset=4000 + lo)
            eng.set_state(torch.as_tensor(rows[lo:hi].copy(), device=eng.device))
            got.append(_np(eng.evaluate_policies(_population(weights), H, discount=0.97, final_obs=True)))
            eng.close()
        outs.append([np.concatenate([g[k] for g in got], axis=1) for k in range(3)])
    for a, b in zip(*outs):
        assert a.shape[:2] == (P, N) and _same(a, b)


def test_tanh_mode():
    """out="tanh" on a continuous env, through the same replay route.  The device's float64 tanh is not pinned against a host's: the
    actions the members take lie within ONE float32 spacing at max(|lo|, |hi|) of the numpy reference (test_gpu_policy.py's derived
    bound).  The two device routes evaluate the same device function on the same rows, so between THEM the replay identity holds
    as in the clip mode."""
    case, hidden = "ip-rebound-balancing", 5
    name, _, N, P, H = CASES[case]
    r = _run(case, hidden, 1.0, "tanh")
    _check_replay(case, r)
    (e_ret, e_L, e_fo, acts) = r["ref"]
    lo, hi = PR.ctrl_range(name)
    x0 = PP.first_observation(name, PP.gpu_start(name, N)).astype(np.float32)
    tol = np.spacing(np.float32(max(abs(lo), abs(hi))))
    for p in range(P):  # the first action of every member, from x_0 (later rows are the device's own and not outputs of this route)
        want = PR.mlp_actions(r["weights"][p], x0, lo, hi, False)[:, 0]
        err = np.abs(acts[p][0].reshape(-1).astype(np.float64) - want.astype(np.float64)).max()
        print(f"member {p}: max |action - reference| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol
    assert (np.abs(acts) <= hi).all() and (np.abs(acts) < hi).any()
    assert not np.array_equal(r["got"][0], _run(case, hidden)["got"][0])  # and it is not the clip mode's result


def test_handle_dependent_refusals():
    from emei_amd import _lib as L
    from emei_amd.engine import _ptr, _stream

    case = "cartpole-balancing"
    _, _, N, P, H = CASES[case]
    eng = _engine(case)
    pop = _population(_weights(case, 5))
    with pytest.raises(AssertionError, match="emei_evaluate_policies: call reset"):
        eng.evaluate_policies(pop, H)  # EMEI_ERR_STATE: no state and no start_state
    rows = _start(case, eng)
    first = eng.evaluate_policies(pop, H, start_state=rows)  # ... a start_state serves a handle that was never reset
    eng.set_state(rows)
    for x, y in zip(first, eng.evaluate_policies(pop, H)):
        assert torch.equal(x, y)
    ret = torch.empty((P, N), dtype=torch.float64, device=eng.device)
    ps = pop.struct()

    def call(n_policies=P, ret_ptr=_ptr(ret)):
        with torch.cuda.device(eng.device):
            return L.lib().emei_evaluate_policies(eng._h, H, n_policies, C.byref(ps), 1.0, None, ret_ptr, None, None, _stream())

    too_many = (2**31 - 1) // N + 1
    assert call(too_many) == L.ERR_INVALID
    msg = L.lib().emei_last_error().decode()
    assert msg.startswith("emei_evaluate_policies:") and "n_envs * n_policies" in msg, msg
    assert call(ret_ptr=None) == L.ERR_INVALID
    msg = L.lib().emei_last_error().decode()
    assert msg.startswith("emei_evaluate_policies:") and "return_out" in msg, msg
    assert call(too_many, None) == L.ERR_INVALID and "return_out" in L.lib().emei_last_error().decode()  # in the header's order
    with pytest.raises(ValueError, match="CartPoleBalancing"):
        eng.evaluate_policies(_population(_weights("cheetah", 5)), H)  # shapes of another env
    with pytest.raises(TypeError):
        eng.evaluate_policies(lambda o: o, H)
    eng.close()


def test_env_surface():
    import emei_amd

    env = emei_amd.make("CartPoleBalancing-v0", num_envs=5)
    pop = _population(_weights("cartpole-balancing", 0))
    with pytest.raises(AssertionError):
        env.evaluate_policies(pop, 10)
    env.reset(seed=0)
    before = env.engine.get_state().clone()
    ret, L, fo = env.evaluate_policies(pop, 10, discount=0.99, final_obs=True)
    assert ret.shape == (3, 5) and ret.dtype == torch.float64 and L.dtype == torch.int32 and fo.shape == (3, 5, 4)
    assert torch.equal(env.engine.get_state(), before)
    again = env.evaluate_policies(pop, 10, discount=0.99, start_state=before.cpu().numpy())
    assert torch.equal(again[0], ret) and torch.equal(again[1], L)


def test_capture_replays_the_same_result():
    case = "cartpole-balancing"
    _, _, N, P, H = CASES[case]
    eng = _engine(case)
    pop = _population(_weights(case, 5))
    eng.set_state(_start(case, eng))
    want = eng.evaluate_policies(pop, H, 0.99, final_obs=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = eng.evaluate_policies(pop, H, 0.99, final_obs=True)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    eng.close()
