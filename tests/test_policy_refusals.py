"""The refusals of the policy entry points and the nominal controllers that need no handle, pinned to their whole text and order:
emei_rollout_policy, emei_rollout_policy_noisy, emei_rollout_policy_deep, emei_evaluate_policies, emei_evaluate_policies_deep,
emei_plan_policy, emei_plan_policy_deep, emei_mpc_policy, emei_mpc_mppi and emei_mpc_cem (the planner calls have
tests/test_plan_refusals.py; the *_api.py files of these calls check prefixes and argument names).

Every call has a NULL handle.  TABLE lists, per entry point and in the order include/emei_hip.h documents, the arguments that make it
refuse before it looks at the handle, each with the whole emei_last_error() string behind "<entry point>: ".  One test gives every bad
argument alone; another gives every two of them at once (where they can be combined) and wants the EARLIER one named, which pins the
order; the all-good call names the handle.  A change of the host plumbing that moves a check, rewords it or formats a value
differently fails here, without a GPU."""
import ctypes as C

import pytest

from emei_amd import _lib

INF, NAN = float("inf"), float("nan")
T, H, K = 2, 3, 5
_BUF = (C.c_double * 64)()
P = C.cast(_BUF, C.c_void_p).value  # never dereferenced: every call here returns before the handle is used
GAUSS, HEAD, EPS = _lib.POLICY_NOISE_GAUSS, _lib.POLICY_NOISE_GAUSS_HEAD, _lib.POLICY_NOISE_EPS_GREEDY
SIZES = {_lib.EmeiPolicy: 48, _lib.EmeiPolicyDeep: 72, _lib.EmeiPolicyNoise: 64}
GOOD = {
    _lib.EmeiPolicy: dict(struct_size=48, hidden=4, out_mode=0, reserved=0, w1=P, b1=P, w2=P, b2=P),
    _lib.EmeiPolicyDeep: dict(struct_size=72, hidden1=8, hidden2=8, out_mode=0, w1=P, b1=P, w2=P, b2=P, w3=P, b3=P, reserved=0),
    _lib.EmeiPolicyNoise: dict(struct_size=64, mode=GAUSS, seed=7, sigma=0.1, std=None, ws=P, bs=P, log_std_min=-1.0, log_std_max=1.0,
                               reserved=0),
}


def _struct(cls, over):
    """a good struct of `cls` with the fields of `over` replaced; over None -> a NULL pointer"""
    if over is None:
        return None
    return C.byref(cls(**dict(GOOD[cls], **over)))


# ------------------------------------------------------------------------------------------------ the calls, all arguments good
def _rollout_policy(lib, n_steps=T, policy={}, **_):
    return lib.emei_rollout_policy(None, n_steps, _struct(_lib.EmeiPolicy, policy), P, _lib.ACT_F32, P, P, P, 0, None)


def _rollout_policy_noisy(lib, n_steps=T, policy={}, noise={}, **_):
    return lib.emei_rollout_policy_noisy(None, n_steps, _struct(_lib.EmeiPolicy, policy), _struct(_lib.EmeiPolicyNoise, noise), P,
                                         _lib.ACT_F32, P, P, P, 0, None)


def _rollout_policy_deep(lib, n_steps=T, policy={}, noise={}, **_):
    return lib.emei_rollout_policy_deep(None, n_steps, _struct(_lib.EmeiPolicyDeep, policy), _struct(_lib.EmeiPolicyNoise, noise), P,
                                        _lib.ACT_F32, P, P, P, 0, None)


def _evaluate_policies(lib, horizon=H, k=2, stacked={}, discount=1.0, **_):
    return lib.emei_evaluate_policies(None, horizon, k, _struct(_lib.EmeiPolicy, stacked), discount, None, P, P, None, None)


def _evaluate_policies_deep(lib, horizon=H, k=2, stacked={}, discount=1.0, **_):
    return lib.emei_evaluate_policies_deep(None, horizon, k, _struct(_lib.EmeiPolicyDeep, stacked), discount, None, P, P, None, None)


def _plan_policy(lib, horizon=H, k=K, policy={}, noise={}, discount=1.0, temperature=1.0, mean=None, ess=None, **_):
    return lib.emei_plan_policy(None, horizon, k, _struct(_lib.EmeiPolicy, policy), _struct(_lib.EmeiPolicyNoise, noise), discount,
                                temperature, None, P, P, _lib.ACT_F32, mean, P, P, None, None, ess, None)


def _plan_policy_deep(lib, horizon=H, k=K, policy={}, noise={}, value=None, discount=1.0, temperature=1.0, mean=None, ess=None, **_):
    return lib.emei_plan_policy_deep(None, horizon, k, _struct(_lib.EmeiPolicyDeep, policy), _struct(_lib.EmeiPolicyNoise, noise),
                                     _struct(_lib.EmeiPolicyDeep, value), discount, temperature, None, P, P, _lib.ACT_F32, mean, P, P,
                                     None, None, ess, None)


def _mpc_policy(lib, n_steps=T, horizon=H, k=K, policy={}, noise={}, act_mode=_lib.MPC_POLICY_ACT_BEST, discount=1.0, temperature=1.0,
                ess=None, **_):
    return lib.emei_mpc_policy(None, n_steps, horizon, k, _struct(_lib.EmeiPolicy, policy), _struct(_lib.EmeiPolicyNoise, noise), 3,
                               act_mode, discount, temperature, P, P, _lib.ACT_F32, P, P, P, None, None, ess, 0, None)


def _mpc_mppi(lib, n_steps=T, horizon=H, k=K, discount=1.0, temperature=1.0, refill=0.0, lo=-1.0, hi=1.0, **_):
    return lib.emei_mpc_mppi(None, n_steps, horizon, k, 7, P, 0.5, discount, temperature, refill, lo, hi, P, P, _lib.ACT_F32, P, P, P, None,
                             None, 0, None)


def _mpc_cem(lib, n_steps=T, horizon=H, k=K, n_elites=2, iterations=1, sigma_min=0.0, discount=1.0, refill=0.0, lo=-1.0, hi=1.0, **_):
    return lib.emei_mpc_cem(None, n_steps, horizon, k, n_elites, iterations, 7, P, 0.5, sigma_min, discount, refill, lo, hi, P, P,
                            _lib.ACT_F32, P, P, P, None, None, 0, None)


# ------------------------------------------------------------------------------------------------ the refusals, in the header's order
N_STEPS = [({"n_steps": 0}, "n_steps=0 < 1"), ({"n_steps": -3}, "n_steps=-3 < 1")]
HORIZON = [({"horizon": 0}, "horizon=0 < 1")]
DISCOUNT = [({"discount": 0.0}, "discount=0 is outside (0, 1]"), ({"discount": 1.5}, "discount=1.5 is outside (0, 1]"),
            ({"discount": NAN}, "discount=nan is outside (0, 1]")]


def _count(name, **bad):
    return [(bad or {"k": 0}, f"{name}=0 < 1")]


def _temperature(**needs):
    """a temperature counts only where the call forms the weights: `needs` is what makes it"""
    return [(dict(needs, temperature=0.0), "temperature=0 must be finite and > 0"),
            (dict(needs, temperature=INF), "temperature=inf must be finite and > 0"),
            (dict(needs, temperature=NAN), "temperature=nan must be finite and > 0")]


def _policy(arg):
    return [({arg: None}, f"null {arg}"),
            ({arg: {"struct_size": 40}}, f"{arg}.struct_size=40 != sizeof(emei_policy)=48"),
            ({arg: {"hidden": -1}}, f"{arg}.hidden=-1 is outside [0, EMEI_POLICY_MAX_HIDDEN=1024]"),
            ({arg: {"hidden": 1025}}, f"{arg}.hidden=1025 is outside [0, EMEI_POLICY_MAX_HIDDEN=1024]"),
            ({arg: {"out_mode": 2}}, f"unknown {arg}.out_mode=2"),
            ({arg: {"reserved": 1}}, f"{arg}.reserved=1 must be 0")]


def _deep(arg, with_out_mode=True, optional=False):
    rows = [] if optional else [({arg: None}, f"null {arg}")]
    rows += [({arg: {"struct_size": 48}}, f"{arg}.struct_size=48 != sizeof(emei_policy_deep)=72"),
             ({arg: {"hidden1": 0}}, f"{arg}.hidden1=0 is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=256]"),
             ({arg: {"hidden1": 257}}, f"{arg}.hidden1=257 is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=256]"),
             ({arg: {"hidden2": 0}}, f"{arg}.hidden2=0 is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=256]"),
             ({arg: {"hidden2": 257}}, f"{arg}.hidden2=257 is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=256]")]
    if with_out_mode:
        rows.append(({arg: {"out_mode": -1}}, f"unknown {arg}.out_mode=-1"))
    return rows + [({arg: {"reserved": 2 ** 40}}, f"{arg}.reserved=1099511627776 must be 0")]


def _noise(optional=False):
    rows = [] if optional else [({"noise": None}, "null noise")]
    return rows + [
        ({"noise": {"struct_size": 56}}, "noise.struct_size=56 != sizeof(emei_policy_noise)=64"),
        ({"noise": {"mode": 3}}, "unknown noise.mode=3"),
        ({"noise": {"mode": -1}}, "unknown noise.mode=-1"),
        ({"noise": {"reserved": 5}}, "noise.reserved=5 must be 0"),
        ({"noise": {"mode": GAUSS, "sigma": -0.5}}, "noise.sigma=-0.5 must be finite and >= 0 (noise.std is null)"),
        ({"noise": {"mode": GAUSS, "sigma": INF}}, "noise.sigma=inf must be finite and >= 0 (noise.std is null)"),
        ({"noise": {"mode": EPS, "sigma": 1.5}}, "noise.sigma=1.5 (epsilon) is outside [0, 1]"),
        ({"noise": {"mode": EPS, "sigma": NAN}}, "noise.sigma=nan (epsilon) is outside [0, 1]"),
        ({"noise": {"mode": HEAD, "log_std_min": 1.0, "log_std_max": 0.5}}, "noise.log_std_min=1 > noise.log_std_max=0.5 (or a NaN)"),
        ({"noise": {"mode": HEAD, "log_std_max": NAN}}, "noise.log_std_min=-1 > noise.log_std_max=nan (or a NaN)"),
        ({"noise": {"mode": HEAD, "ws": None}}, "null noise.ws"),
        ({"noise": {"mode": HEAD, "bs": None}}, "null noise.bs")]


BOUNDS = [({"refill": INF}, "refill=inf must be finite"), ({"refill": NAN}, "refill=nan must be finite"),
          ({"lo": 1.0, "hi": 0.5}, "nominal_lo=1, nominal_hi=0.5: need nominal_lo <= nominal_hi"),
          ({"lo": NAN}, "nominal_lo=nan, nominal_hi=1: need nominal_lo <= nominal_hi")]
N_ELITES = [({"n_elites": 0}, "n_elites=0 is outside [1, n_candidates=5]"), ({"n_elites": K + 1}, "n_elites=6 is outside [1, n_candidates=5]")]

# entry point -> (its call, [(bad arguments, message)] in the order of its refusals); "null handle" ends every list
TABLE = {
    "emei_rollout_policy": (_rollout_policy, N_STEPS + _policy("policy")),
    "emei_rollout_policy_noisy": (_rollout_policy_noisy, N_STEPS + _policy("policy") + _noise()),
    "emei_rollout_policy_deep": (_rollout_policy_deep, N_STEPS + _deep("policy") + _noise(optional=True)),
    "emei_evaluate_policies": (_evaluate_policies, HORIZON + _count("n_policies") + DISCOUNT + _policy("stacked")),
    "emei_evaluate_policies_deep": (_evaluate_policies_deep, HORIZON + _count("n_policies") + DISCOUNT + _deep("stacked")),
    "emei_plan_policy": (_plan_policy, HORIZON + _count("n_candidates") + DISCOUNT + _temperature(ess=P) + _temperature(mean=P)
                         + _policy("policy") + _noise()),
    "emei_plan_policy_deep": (_plan_policy_deep, HORIZON + _count("n_candidates") + DISCOUNT + _temperature(ess=P) + _temperature(mean=P)
                              + _deep("policy") + _noise() + _deep("value", with_out_mode=False, optional=True)),
    "emei_mpc_policy": (_mpc_policy, N_STEPS + HORIZON + _count("n_candidates") + DISCOUNT
                        + [({"act_mode": 2}, "unknown act_mode=2"), ({"act_mode": -1}, "unknown act_mode=-1")]
                        + _temperature(act_mode=_lib.MPC_POLICY_ACT_MEAN) + _temperature(ess=P) + _policy("policy") + _noise()),
    "emei_mpc_mppi": (_mpc_mppi, N_STEPS + HORIZON + _count("n_candidates") + DISCOUNT + _temperature() + BOUNDS
                      + [({"horizon": 257}, "horizon=257 exceeds EMEI_MPC_MAX_HORIZON=256 (the nominal lives in LDS)")]),
    "emei_mpc_cem": (_mpc_cem, N_STEPS + HORIZON + _count("n_candidates") + N_ELITES + DISCOUNT
                     + [({"iterations": 0}, "iterations=0 < 1")] + BOUNDS
                     + [({"sigma_min": -1.0}, "sigma_min=-1 must be finite and >= 0"), ({"sigma_min": INF}, "sigma_min=inf must be finite and >= 0"),
                        ({"horizon": 257}, "horizon=257 exceeds EMEI_MPC_MAX_HORIZON=256 (the mean and the sigma live in LDS)")]),
}
SINGLE = [(fn, i) for fn, (_, rows) in TABLE.items() for i in range(len(rows))]


def _refused(fn, over):
    lib = _lib.lib()
    rc = TABLE[fn][0](lib, **over)
    return rc, lib.emei_last_error().decode()


def _merge(a, b):
    """both sets of bad arguments in one call, or None where they name the same argument (the same field of a struct)"""
    out = dict(a)
    for key, v in b.items():
        if key not in out:
            out[key] = v
        elif isinstance(v, dict) and isinstance(out[key], dict) and not set(v) & set(out[key]):
            out[key] = dict(out[key], **v)
        else:
            return None
    return out


def test_struct_sizes():
    for cls, size in SIZES.items():
        assert C.sizeof(cls) == size


@pytest.mark.parametrize("fn,i", SINGLE, ids=[f"{fn}-{i}" for fn, i in SINGLE])
def test_one_bad_argument(fn, i):
    over, text = TABLE[fn][1][i]
    assert _refused(fn, over) == (_lib.ERR_INVALID, f"{fn}: {text}"), over


@pytest.mark.parametrize("fn", sorted(TABLE))
def test_all_good_names_the_handle(fn):
    assert _refused(fn, {}) == (_lib.ERR_INVALID, f"{fn}: null handle")


@pytest.mark.parametrize("fn", sorted(TABLE))
def test_two_bad_arguments_name_the_earlier(fn):
    rows = TABLE[fn][1]
    pairs = 0
    for i, (a, text) in enumerate(rows):
        for b, _ in rows[i + 1:]:
            both = _merge(a, b)
            if both is None:
                continue
            pairs += 1
            assert _refused(fn, both) == (_lib.ERR_INVALID, f"{fn}: {text}"), both
    assert pairs >= len(rows)  # the table is dense enough to order every neighbour


def test_what_does_not_count():
    """arguments a call does not read are not refused: the next check (the handle) answers"""
    handle = lambda fn: (_lib.ERR_INVALID, f"{fn}: null handle")
    # a temperature without a weighted output
    for fn in ("emei_plan_policy", "emei_plan_policy_deep", "emei_mpc_policy"):
        assert _refused(fn, {"temperature": 0.0}) == handle(fn)
        assert _refused(fn, {"temperature": NAN}) == handle(fn)
    # emei_rollout_policy_deep's noise is optional; emei_plan_policy_deep's value too, and its out_mode is not read
    assert _refused("emei_rollout_policy_deep", {"noise": None}) == handle("emei_rollout_policy_deep")
    assert _refused("emei_plan_policy_deep", {"value": {}}) == handle("emei_plan_policy_deep")
    assert _refused("emei_plan_policy_deep", {"value": {"out_mode": 7}}) == handle("emei_plan_policy_deep")
    # a Gaussian noise with a std tensor does not read sigma; the head and epsilon-greedy modes do not read what the others do
    for fn in ("emei_rollout_policy_noisy", "emei_plan_policy", "emei_mpc_policy"):
        assert _refused(fn, {"noise": {"std": P, "sigma": -1.0}}) == handle(fn)
        assert _refused(fn, {"noise": {"mode": EPS, "sigma": 1.0, "ws": None, "bs": None, "log_std_min": 2.0}}) == handle(fn)
        assert _refused(fn, {"noise": {"mode": HEAD, "sigma": -1.0}}) == handle(fn)
    # emei_mpc_cem: n_elites is looked at only once horizon and n_candidates are good
    assert _refused("emei_mpc_cem", {"k": 0, "n_elites": 0}) == (_lib.ERR_INVALID, "emei_mpc_cem: n_candidates=0 < 1")
    # hidden = 0 is the affine policy
    assert _refused("emei_rollout_policy", {"policy": {"hidden": 0, "w1": None, "b1": None}}) == handle("emei_rollout_policy")


# sizeof(PlanPartial) = 16, one per (wave, env) segment bound; emei_plan_policy keeps a float64 return and six float32 first-action
# slots per candidate behind them; the controllers one float64 per candidate (emei_mpc_policy: and one float32, rounded up to 8 bytes)
WORKSPACE = {
    "emei_plan_policy_workspace_bytes": lambda n, k: 16 * ((n * k + 63) // 64 + n) + (8 + 6 * 4) * n * k,
    "emei_mpc_policy_workspace_bytes": lambda n, k: (12 * n * k + 7) // 8 * 8,
    "emei_mpc_cem_workspace_bytes": lambda n, k: 8 * n * k,
    "emei_mpc_mppi_workspace_bytes": lambda n, k: 8 * n * k,
}
SHAPES = [((0, 2), "n_envs=0"), ((2, 0), "n_candidates=0 < 1"), ((2, 2 ** 30), "n_envs * n_candidates = 2147483648 exceeds 2^31 - 1"),
          ((2 ** 31, 1), "n_envs=2147483648")]


@pytest.mark.parametrize("fn", sorted(WORKSPACE))
def test_workspace_bytes(fn):
    lib = _lib.lib()
    f = getattr(lib, fn)
    for shape, text in SHAPES:
        assert (f(*shape), lib.emei_last_error().decode()) == (_lib.ERR_INVALID, f"{fn}: {text}"), shape
    for n, k in ((65, 3), (1, 1), (3, 64), (2, 5), (1, 2 ** 31 - 1)):
        assert f(n, k) == WORKSPACE[fn](n, k), (n, k)
