"""The refusals of the policy entry points and the nominal controllers that need a handle, pinned to their code, whole text and order,
and one valid call of each behind them, per kernel family: emei_rollout_policy, emei_rollout_policy_noisy, emei_rollout_policy_deep,
emei_evaluate_policies, emei_evaluate_policies_deep, emei_plan_policy, emei_plan_policy_deep, emei_mpc_policy, emei_mpc_mppi and
emei_mpc_cem (what they refuse without a handle: tests/test_policy_refusals.py; the planner calls: tests/test_gpu_plan_refusals.py).

The refusals: handles of n_envs = 2 — CartPoleSwingUp (discrete, the 4-state kernels), ReboundInvertedPendulumBalancing (continuous,
the 4-state kernels), ReboundInvertedDoublePendulumBalancing (the body kernels, with fused controllers) and HopperRunning (the body
kernels, without).  Every refusal returns before a launch; the raw C ABI is called so that NULL pointers and wrong dtypes, which Engine
refuses itself, reach the library.  Every pointer is a device buffer large enough for the call's shape all the same.  ORDER lists
each call's refusals in the header's order; every two of them at once must name the earlier one.

The valid calls: N = 65 (one full wave and one lane), T = 2, H = 2, K = 3, hidden 4 (the deep networks 8-8), a population of 2, on
one row of tests/kernel_matrix.py per route — the 4-state route on a CartPole and an InvertedPendulum row, the body route on an
InvertedDoublePendulum row for the controllers and a Hopper row for the rest — each through the check of
tests/test_gpu_kernel_matrix.py (tests/test_gpu_mpc_policy.py for emei_mpc_policy) at these shapes: bit for bit against the loop or
the composition the call is defined by, with max_episode_steps = 1 so that every env crosses a device reset within T = 2.  A launch
descriptor that loses or swaps a field between the entry point and the kernel, or a wrong grid, fails here in seconds."""
import ctypes as C

import pytest

import kernel_matrix as KM
from emei_amd import _lib
from test_gpu_mppi import CH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, T, H, K = 65, 2, 2, 3
INV, STATE, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_STATE, _lib.ERR_UNSUPPORTED
GAUSS, HEAD, EPS = _lib.POLICY_NOISE_GAUSS, _lib.POLICY_NOISE_GAUSS_HEAD, _lib.POLICY_NOISE_EPS_GREEDY
BIG = 2 ** 31 - 1
OVERFLOW = "n_envs * n_candidates = 4294967294 exceeds 2^31 - 1"  # n_envs = 2
POP_OVERFLOW = "n_envs * n_policies = 4294967294 exceeds 2^31 - 1"
NO_STATE = "call reset before using the state"
PEERS = "observation peers are set (emei_set_obs_peers), which this kernel does not serve"
ON_BODY = ("this handle steps on the body kernels (a multi-body env, or an InvertedPendulum with a non-euler integrator or observation "
           "noise); the fused controller serves the 4-state kernels only")
OBS_NOISE = ("this InvertedDoublePendulum handle has observation noise (obs_sigma[0]=0.001), which the fused controller does not serve: "
             "its plan steps the model without it")
WHOLE = ("discrete-action", "continuous-action", "bad action_dtype")  # check_action_dtype's messages carry no entry point
PEND = dict(freq_rate=4, real_time_scale=0.02)
KINDS = {"cartpole": ("CartPoleSwingUp", {}), "invpend": ("ReboundInvertedPendulumBalancing", {}),
         "dpend": ("ReboundInvertedDoublePendulumBalancing", PEND), "hopper": ("HopperRunning", CH)}

ROLLOUTS = ("emei_rollout_policy", "emei_rollout_policy_noisy", "emei_rollout_policy_deep")
POPULATIONS = ("emei_evaluate_policies", "emei_evaluate_policies_deep")
PLANS = ("emei_plan_policy", "emei_plan_policy_deep")
CONTROLLERS = ("emei_mpc_policy", "emei_mpc_mppi", "emei_mpc_cem")
NOMINAL = ("emei_mpc_mppi", "emei_mpc_cem")
ALL_FNS = ROLLOUTS + POPULATIONS + PLANS + CONTROLLERS
OUT_NAME = {fn: "best_action_out" if fn in PLANS else "actions_out" for fn in ROLLOUTS + PLANS + ("emei_mpc_policy",)}
STRUCT_ARGS = ("policy", "stacked", "noise", "value")


def _dtype_text(fn, d):
    return f"action_dtype={d}: {OUT_NAME[fn]} is uint8 / int32 / int64 for the discrete envs, float32 for the continuous ones"


def _noise_text(mode):
    return f"noise.mode={mode}: the Gaussian modes are for the continuous envs, EMEI_POLICY_NOISE_EPS_GREEDY for the discrete ones"


class Handle:
    """an engine and 24 separate 4 KiB device buffers, enough for every array of a call at n_envs = 2, T = H = 2, K = 3"""

    def __init__(self, kind, reset=True, **kw):
        from emei_amd.engine import Engine

        name, base = KINDS[kind]
        self.eng = Engine(name, 2, **dict(base, **kw))
        if reset:
            self.eng.reset(seed=3)
        self.buf = torch.zeros((24, 512), dtype=torch.float64, device=self.eng.device)
        self.discrete = self.eng.act_dim == 0
        self.good = _lib.ACT_U8 if self.discrete else _lib.ACT_F32  # an action dtype the env's kind takes
        self.wrong = _lib.ACT_F32 if self.discrete else _lib.ACT_U8
        self.noise = dict(mode=EPS, sigma=0.25) if self.discrete else dict(mode=GAUSS, sigma=0.1)  # a noise the env's kind takes
        self.wrong_noise = dict(mode=GAUSS, sigma=0.1) if self.discrete else dict(mode=EPS, sigma=0.25)

    def p(self, i):
        return self.buf[i].data_ptr()

    def struct(self, fn, arg, over):
        """the struct argument `arg` of `fn`: zero weights on the device, hidden 4 (deep: 8-8), with `over`'s fields replaced"""
        if over is None:
            return None
        p = self.p
        if arg == "noise":
            f = dict(struct_size=64, seed=7, std=None, ws=p(20), bs=p(21), log_std_min=-1.0, log_std_max=1.0, reserved=0, **self.noise)
            return C.byref(_lib.EmeiPolicyNoise(**dict(f, **over)))
        if fn.endswith("_deep"):
            f = dict(struct_size=72, hidden1=8, hidden2=8, out_mode=0, w1=p(14), b1=p(15), w2=p(16), b2=p(17), w3=p(18), b3=p(19), reserved=0)
            return C.byref(_lib.EmeiPolicyDeep(**dict(f, **over)))
        f = dict(struct_size=48, hidden=4, out_mode=0, reserved=0, w1=p(14), b1=p(15), w2=p(16), b2=p(17))
        return C.byref(_lib.EmeiPolicy(**dict(f, **over)))

    def defaults(self, fn):
        """the arguments of a valid call of `fn` between the handle and the stream, in the ABI's order ({}: a good struct)"""
        p, dt = self.p, self.good
        outs = dict(act=p(2), dtype=dt, obs=p(3), rew=p(4), done=p(5))
        plan = dict(discount=1.0, temperature=1.0, start=None, ws=p(1), act=p(2), dtype=dt, mean=None, ret=p(6), idx=p(7), length=None,
                    returns=None, ess=None)
        nominal = dict(refill=0.5, lo=-1.0, hi=1.0, ws=p(1), **outs, plan_return=None, aux=None, flags=0)
        return {
            "emei_rollout_policy": dict(n_steps=T, policy={}, **outs, flags=0),
            "emei_rollout_policy_noisy": dict(n_steps=T, policy={}, noise={}, **outs, flags=0),
            "emei_rollout_policy_deep": dict(n_steps=T, policy={}, noise={}, **outs, flags=0),
            "emei_evaluate_policies": dict(horizon=H, k=2, stacked={}, discount=1.0, start=None, ret=p(6), length=p(7), final=None),
            "emei_evaluate_policies_deep": dict(horizon=H, k=2, stacked={}, discount=1.0, start=None, ret=p(6), length=p(7), final=None),
            "emei_plan_policy": dict(horizon=H, k=K, policy={}, noise={}, **plan),
            "emei_plan_policy_deep": dict(horizon=H, k=K, policy={}, noise={}, value=None, **plan),
            "emei_mpc_policy": dict(n_steps=T, horizon=H, k=K, policy={}, noise={}, stride=H, act_mode=_lib.MPC_POLICY_ACT_BEST, discount=1.0,
                                    temperature=1.0, ws=p(1), **outs, plan_return=None, plan_index=None, ess=None, flags=0),
            "emei_mpc_mppi": dict(n_steps=T, horizon=H, k=K, seed=7, nominal=p(0), sigma=0.5, discount=1.0, temperature=1.0, **nominal),
            "emei_mpc_cem": dict(n_steps=T, horizon=H, k=K, n_elites=2, iterations=1, seed=7, nominal=p(0), sigma=0.5, sigma_min=0.0,
                                 discount=1.0, **nominal),
        }[fn]

    def call(self, fn, **over):
        args = self.defaults(fn)
        assert set(over) <= set(args), (fn, over)
        args.update(over)
        for arg in STRUCT_ARGS:
            if arg in args:
                args[arg] = self.struct(fn, arg, args[arg])
        lib = _lib.lib()
        rc = getattr(lib, fn)(self.eng._h, *args.values(), None)
        return rc, lib.emei_last_error().decode()

    def refused(self, fn, code, text, **over):
        if not text.startswith(WHOLE):
            text = f"{fn}: {text}"
        assert self.call(fn, **over) == (code, text), (self.eng.env_name, fn, over)

    def accepted(self, fn, **over):
        rc, msg = self.call(fn, **over)
        torch.cuda.synchronize()
        assert rc == _lib.OK, (self.eng.env_name, fn, over, msg)

    def set_peers(self, on):
        """one observation peer of 16 rows (never written: every call under it is refused), or none"""
        arr = (C.c_void_p * 1)(self.p(22))
        rc = _lib.lib().emei_set_obs_peers(self.eng._h, 1 if on else 0, arr, 2, 0, 16)
        assert rc == _lib.OK, _lib.lib().emei_last_error().decode()


@pytest.fixture(scope="module")
def handles():
    return {kind: Handle(kind) for kind in KINDS}


def _weights(fn):
    """(struct argument, [weight pointer names]) of the call's network, in the order they are checked"""
    arg = "stacked" if fn in POPULATIONS else "policy"
    return arg, ("w1", "b1", "w2", "b2", "w3", "b3") if fn.endswith("_deep") else ("w2", "b2", "w1", "b1")


def _null_weight(fn, arg, name):
    one_layer_first = not fn.endswith("_deep") and arg != "value" and name in ("w1", "b1")
    return f"null {arg}.{name}" + (" with hidden=4" if one_layer_first else "")


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_null_weights(handles, kind):
    h = handles[kind]
    for fn in ROLLOUTS + POPULATIONS + PLANS + ("emei_mpc_policy",):
        arg, names = _weights(fn)
        for name in names:
            h.refused(fn, INV, _null_weight(fn, arg, name), **{arg: {name: None}})
    for name in ("w1", "b1", "w2", "b2", "w3", "b3"):
        h.refused("emei_plan_policy_deep", INV, f"null value.{name}", value={name: None})
    # the affine policy has no first layer
    h.refused("emei_rollout_policy", INV, "null policy.b2", policy=dict(hidden=0, w1=None, b1=None, b2=None))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_wrong_action_dtype(handles, kind):
    h = handles[kind]
    for fn in OUT_NAME:
        for d in (h.wrong, 7, -1):
            h.refused(fn, INV, _dtype_text(fn, d), dtype=d)
    general = "discrete-action envs take uint8/int32/int64 actions [n]" if h.discrete else \
        f"continuous-action envs take float32 actions [n,{h.eng.act_dim}]"
    for fn in NOMINAL:
        h.refused(fn, INV, general, dtype=h.wrong)
        h.refused(fn, INV, "bad action_dtype 7", dtype=7)
        h.refused(fn, INV, "bad action_dtype -1", dtype=-1)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_unknown_flags(handles, kind):
    h = handles[kind]
    for fn in ROLLOUTS + CONTROLLERS:
        h.refused(fn, INV, "unknown flags 0x2", flags=2)
        h.refused(fn, INV, "unknown flags 0x80000001", flags=0x80000001)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_noise_kind_against_env_kind(handles, kind):
    h = handles[kind]
    for fn in ("emei_rollout_policy_noisy", "emei_rollout_policy_deep") + PLANS + ("emei_mpc_policy",):
        h.refused(fn, INV, _noise_text(h.wrong_noise["mode"]), noise=h.wrong_noise)
        if h.discrete:
            h.refused(fn, INV, _noise_text(HEAD), noise=dict(mode=HEAD))
    h.accepted("emei_rollout_policy_deep", noise=None)  # its noise is optional


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_null_pointers(handles, kind):
    h = handles[kind]
    for fn in POPULATIONS:
        h.refused(fn, INV, "null return_out", ret=None)
    for fn in PLANS:
        h.refused(fn, INV, "null workspace", ws=None)
        h.refused(fn, INV, "null best_action_out", act=None)
    for fn in CONTROLLERS:
        h.refused(fn, INV, "null workspace", ws=None)
        h.refused(fn, INV, "null actions_out", act=None)
    for fn in NOMINAL:
        h.refused(fn, INV, "null nominal", nominal=None)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_population_and_candidate_bounds(handles, kind):
    h = handles[kind]
    for fn in POPULATIONS:
        h.refused(fn, INV, POP_OVERFLOW, k=BIG)
        h.refused(fn, INV, "n_envs * n_policies = 2147483648 exceeds 2^31 - 1", k=2 ** 30)
    for fn in PLANS + CONTROLLERS:
        h.refused(fn, INV, OVERFLOW, k=BIG)
    if not h.discrete:
        for fn in NOMINAL:  # they always plan around a nominal: sigma counts
            h.refused(fn, INV, "sigma=0 with a nominal sequence must be finite and > 0", sigma=0.0)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_before_reset(handles, kind):
    h = Handle(kind, reset=False)
    for fn in ALL_FNS:
        h.refused(fn, STATE, NO_STATE)  # before the kernel family is looked at: the Hopper's handle too
    # the state is the last thing the calls without a start state look at
    h.refused("emei_rollout_policy", INV, "unknown flags 0x2", flags=2)
    h.refused("emei_evaluate_policies", INV, POP_OVERFLOW, k=BIG)
    h.refused("emei_plan_policy", INV, _noise_text(h.wrong_noise["mode"]), noise=h.wrong_noise)
    h.refused("emei_mpc_policy", INV, "null actions_out", act=None)
    h.refused("emei_mpc_cem", INV, "null actions_out", act=None)
    # with start rows the handle's state is not needed
    st = handles[kind].eng.get_state()
    for fn in POPULATIONS + PLANS:
        h.accepted(fn, start=st.data_ptr())


def test_observation_peers(handles):
    """the calls that emit observation rows refuse a handle with peers, after the state; the others do not look"""
    h, cold = handles["cartpole"], Handle("cartpole", reset=False)
    for x in (h, cold):
        x.set_peers(True)
    try:
        for fn in ROLLOUTS + CONTROLLERS:
            h.refused(fn, UNSUPPORTED, PEERS)
            h.refused(fn, INV, "unknown flags 0x2", flags=2)
            cold.refused(fn, STATE, NO_STATE)
        for fn in POPULATIONS + PLANS:
            h.accepted(fn)
    finally:
        for x in (h, cold):
            x.set_peers(False)
    h.accepted("emei_rollout_policy")


def test_the_handles_the_controllers_refuse(handles):
    noisy = Handle("dpend", obs_noise=1e-3)
    rk4 = Handle("invpend", integrator="rk4")  # an InvertedPendulum that steps on the body kernels
    for fn in CONTROLLERS:
        handles["hopper"].refused(fn, UNSUPPORTED, ON_BODY)
        rk4.refused(fn, UNSUPPORTED, ON_BODY)
        noisy.refused(fn, UNSUPPORTED, OBS_NOISE)
        noisy.refused(fn, INV, "null actions_out", act=None)
        for kind in ("cartpole", "invpend", "dpend"):
            handles[kind].accepted(fn)


def _order(h, fn):
    """the refusals of `fn` that need a (reset) handle, in the header's order: (arguments, message)"""
    arg, names = _weights(fn)
    rows = [({arg: {names[0]: None}}, _null_weight(fn, arg, names[0]))] if fn not in NOMINAL else []
    dtype = [({"dtype": h.wrong}, _dtype_text(fn, h.wrong))] if fn in OUT_NAME else []
    flags = [({"flags": 2}, "unknown flags 0x2")]
    noise = [({"noise": h.wrong_noise}, _noise_text(h.wrong_noise["mode"]))]
    if fn in ROLLOUTS:
        return rows + dtype + flags + (noise if fn != "emei_rollout_policy" else [])
    if fn in POPULATIONS:
        return rows + [({"ret": None}, "null return_out"), ({"k": BIG}, POP_OVERFLOW)]
    lanes = [({"k": BIG}, OVERFLOW)]
    if fn in PLANS:
        value = [({"value": {"b3": None}}, "null value.b3")] if fn.endswith("_deep") else []
        return rows + value + lanes + dtype + [({"ws": None}, "null workspace"), ({"act": None}, "null best_action_out")] + noise
    tail = [({"ws": None}, "null workspace"), ({"act": None}, "null actions_out")]
    if fn == "emei_mpc_policy":
        return rows + lanes + dtype + flags + tail + noise
    sigma = [] if h.discrete else [({"sigma": 0.0}, "sigma=0 with a nominal sequence must be finite and > 0")]
    general = "discrete-action envs take uint8/int32/int64 actions [n]" if h.discrete else \
        f"continuous-action envs take float32 actions [n,{h.eng.act_dim}]"
    return sigma + lanes + [({"dtype": h.wrong}, general)] + flags + [({"nominal": None}, "null nominal")] + tail


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_order_of_refusals(handles, kind):
    """a call that is bad in two ways names the earlier check; whatever needs no handle comes before all of them, the state after"""
    h, cold = handles[kind], Handle(kind, reset=False)
    for fn in ALL_FNS:
        rows = _order(h, fn)
        for i, (a, text) in enumerate(rows):
            for b, _ in rows[i + 1:]:
                h.refused(fn, INV, text, **dict(a, **b))
            cold.refused(fn, INV, text, **a)
            first = "n_steps" if "n_steps" in h.defaults(fn) else "horizon"
            h.refused(fn, INV, f"{first}=0 < 1", **dict(a, **{first: 0}))
    for fn in ("emei_plan_policy", "emei_plan_policy_deep"):
        h.refused(fn, INV, "temperature=0 must be finite and > 0", temperature=0.0, ess=h.p(8), policy={"w2": None})
    h.refused("emei_mpc_policy", INV, "unknown act_mode=2", act_mode=2, policy={"w2": None})
    h.refused("emei_mpc_mppi", INV, "horizon=257 exceeds EMEI_MPC_MAX_HORIZON=256 (the nominal lives in LDS)", horizon=257, k=BIG)
    h.refused("emei_mpc_cem", INV, "horizon=257 exceeds EMEI_MPC_MAX_HORIZON=256 (the mean and the sigma live in LDS)", horizon=257, k=BIG)


# ------------------------------------------------------------------------------------------------ one valid call per entry point and route
ROWS = {r.id: r for r in KM.ROWS}
FOUR_STATE, IDP, HOPPER = ("cp0_f64-euler", "ip0_f64-euler"), "dp0_f64-euler", "hp_f64-euler"
ENTRIES = [fn[len("emei_"):] for fn in ALL_FNS]
VALID = [(e, r) for r in FOUR_STATE for e in ENTRIES] + [(e, IDP if "mpc_" in e else HOPPER) for e in ENTRIES]


@pytest.fixture
def matrix(monkeypatch):
    """tests/test_gpu_kernel_matrix.py at this file's shapes: its runners read them from the module"""
    import test_gpu_kernel_matrix as M

    for name, value in dict(N=N, K=K, H=H, T=T).items():
        monkeypatch.setattr(M, name, value)
    engine, one_layer, deep = M._engine, M._one_layer, M._deep
    # every env crosses a device reset within T = 2: the runners' max_episode_steps = 4 becomes 1
    monkeypatch.setattr(M, "_engine", lambda row, n, **over: engine(row, n, **{k: 1 if k == "max_episode_steps" else v for k, v in over.items()}))
    monkeypatch.setattr(M, "_one_layer", lambda eng, seed: one_layer(eng, seed, hidden=4))
    monkeypatch.setattr(M, "_deep", lambda eng, seed, n_out=None: deep(eng, seed, n_out, 8, 8))
    return M


def _run_mpc_policy(row):
    """tests/test_gpu_mpc_policy.py:test_every_compiled_configuration at this file's shapes"""
    import test_gpu_mpc_policy as MP

    kw = dict(row.kw, seed=5, init_noise=0.05 if row.family != "cartpole" else 0.0, max_episode_steps=1)
    fused, loop = MP._engine(row.env, N, **kw), MP._engine(row.env, N, **kw)
    pol, mk = MP._policy(fused, 4), MP._noise_maker(fused)
    fused.reset(9), loop.reset(9)
    a, b = MP._run_both(fused, loop, T, H, K, pol, mk, None, start=False, act="mean", temperature=0.7, discount=0.97, auto_reset=True)
    MP._assert_equal(a, b, row.id)
    assert fused.last_kernel() == (_lib.KERNEL_BODY_MPC_POLICY if row.body else _lib.KERNEL_PEND_MPC_POLICY)
    assert bool((a["done"] != 0).all())  # every env crossed a device reset, every step


@pytest.mark.parametrize("entry,row", VALID, ids=[f"{e}-{r}" for e, r in VALID])
def test_valid_call_equals_its_definition(matrix, entry, row):
    row = ROWS[row]
    if entry == "mpc_policy":
        _run_mpc_policy(row)
    else:
        matrix.RUNNERS[entry](row)


def test_the_valid_calls_cover_both_routes():
    assert len(VALID) == 30 and len(set(VALID)) == 30
    assert not any(ROWS[r].body for r in FOUR_STATE) and ROWS[IDP].body and ROWS[HOPPER].body
    assert ROWS[FOUR_STATE[0]].family == "cartpole" and ROWS[FOUR_STATE[1]].family == "ip_staged"
