"""The terminal value of the open-loop planners on the host: emei_evaluate_sequences_value, emei_plan_shooting_value,
emei_plan_mppi_value, emei_plan_cem_value and emei_plan_value_workspace_bytes are declared (additive under ABI 8: each prototype is its
plain call's with `const emei_policy_deep* value` after `discount`), exported and bound; the header carries the history line, the
terminal-value clause and the refusal order; every refusal that needs no device comes back EMEI_ERR_INVALID with the whole message, for
a NULL handle and before any HIP call, in the header's order — the plain call's scalars, NULL value, value.struct_size, .hidden1,
.hidden2, .reserved, then the handle; the workspace size is emei_plan_cem's.  And the host logic of the Python layer on CPU tensors:
DeepValueFunction.from_module / .to, the value= keyword of the Engine methods and the env-level wrappers, and its type check."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
H, K = 3, 5
_BUF = (C.c_double * 64)()
P = C.cast(_BUF, C.c_void_p).value  # never dereferenced: every call here returns before the handle is used
GOOD = dict(struct_size=72, hidden1=8, hidden2=8, out_mode=0, w1=P, b1=P, w2=P, b2=P, w3=P, b3=P, reserved=0)
VALUE_ARG = "const emei_policy_deep* value"
# new entry point -> (its plain counterpart, the index `value` takes in the argument list: behind `discount`)
PAIRS = {"emei_evaluate_sequences_value": ("emei_evaluate_sequences", 6), "emei_plan_shooting_value": ("emei_plan_shooting", 7),
         "emei_plan_mppi_value": ("emei_plan_mppi", 7), "emei_plan_cem_value": ("emei_plan_cem", 9)}


def _prototype(hdr, fn, ret="int"):
    m = re.search(r"EMEI_API\s+%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, fn), hdr)
    assert m, fn
    return [a.strip() for a in " ".join(m.group(1).split()).split(",")]


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    history = hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    for fn, (plain, at) in PAIRS.items():
        args, base = _prototype(hdr, fn), _prototype(hdr, plain)
        assert args == base[:at] + [VALUE_ARG] + base[at:], fn  # the plain prototype with `value` inserted
        assert base[at - 1] == "double discount", fn
        sym, psym = _lib.SYMBOLS[fn], _lib.SYMBOLS[plain]
        assert sym[0] is C.c_int and len(sym[1]) == len(args)
        assert sym[1][at]._type_ is _lib.EmeiPolicyDeep and list(sym[1][:at]) + list(sym[1][at + 1:]) == list(psym[1]), fn
        assert fn in exported and hasattr(lib, fn) and fn in history, fn
    ws = "emei_plan_value_workspace_bytes"
    assert _prototype(hdr, ws, "int64_t") == ["int64_t n_envs", "int32_t n_candidates"]
    assert _lib.SYMBOLS[ws] == _lib.SYMBOLS["emei_plan_cem_workspace_bytes"] and ws in exported and ws in history
    assert "terminal value" in history[history.index("emei_evaluate_sequences_value"):]
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr) and lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8  # additive
    # the prototypes stand behind the deep struct and every earlier call's text: nothing new in front of emei_mpc_policy
    assert hdr.index("EMEI_API int emei_mpc_policy(") < hdr.index("EMEI_API int64_t " + ws) < hdr.index("/* Which kernel the LAST emei_step")


def test_the_header_states_the_clause_and_the_refusal_order():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    after = hdr[hdr.index("EMEI_API int emei_mpc_policy("):]
    comment = after[:after.index("EMEI_API int64_t emei_plan_value_workspace_bytes(")]
    comment = " ".join(re.sub(r"\n \*", "\n", comment).split())  # one line, the comment's margin taken out
    for word in ("n_out = 1", "w3 [1, hidden2]", "b3 [1]", "widths are its own", "out_mode is ignored", "DEVICE pointers", "not retained",
                 "`value` is required", "clause for clause", "a pure function of (seed, g, k)", "start-state rule", "per-step arithmetic",
                 "L(i, k)", "untouched handle", "neither allocates nor synchronises",
                 "Terminal value.", "set no terminal bit in any of its `horizon` steps", "ret = ret + g_H * (double)v",
                 "after `horizon` multiplications", "v = (float)y_0", "emei_rollout_policy_deep's arithmetic", "float64 ascending sums",
                 "rounded to float32 before the ReLU", "NaN gives 0", "x_H", "step horizon - 1 emits", "the row final_obs_out holds",
                 "rounded to float64 and then added", "no fused multiply-add", "no output clause", "NaN y_0 makes the return NaN",
                 "planner's order puts it last", "terminated gets nothing", "the last one included",
                 "L and final_obs_out are unchanged by the value", "bootstrapped returns", "return_out", "(k*, r*)", "best_*",
                 "MPPI weights, mean and ESS", "CEM elite set, moments and elite_return_out", "redraw the same candidates",
                 "pend_plan_value_kernel", "body_plan_value_kernel", "ONE-WAVE", "dynamic LDS", "64 KiB", "no kernel id",
                 "emei_plan_value_workspace_bytes(n_envs, n_candidates)", "equals emei_plan_cem_workspace_bytes", "negative where that is",
                 "EMEI_ERR_INVALID before any HIP call", "naming the argument", "scalar checks in its order", "NULL value",
                 "value.struct_size, value.hidden1, value.hidden2, value.reserved", "a NULL handle", "NULL value w1, b1, w2, b2, w3, b3",
                 "remaining checks in its order", "EMEI_ERR_STATE where the plain call gives it"):
        assert word in comment, word
    order = [comment.index(w) for w in ("scalar checks in its order", "NULL value;", "value.struct_size", "a NULL handle",
                                        "NULL value w1", "remaining checks")]
    assert order == sorted(order)


# ------------------------------------------------------------------------------------------------ the calls, all arguments good
def _value(over):
    return None if over is None else C.byref(_lib.EmeiPolicyDeep(**dict(GOOD, **over)))


def _evaluate(lib, horizon=H, k=K, discount=1.0, value={}, **_):
    return lib.emei_evaluate_sequences_value(None, horizon, k, P, _lib.ACT_F32, discount, _value(value), None, P, P, None, None)


def _shooting(lib, horizon=H, k=K, discount=1.0, value={}, **_):
    return lib.emei_plan_shooting_value(None, horizon, k, 7, None, 0.0, discount, _value(value), None, P, P, _lib.ACT_F32, None, P, P, None,
                                        None)


def _mppi(lib, horizon=H, k=K, discount=1.0, temperature=1.0, value={}, **_):
    return lib.emei_plan_mppi_value(None, horizon, k, 7, None, 0.0, discount, _value(value), temperature, None, P, P, P, P, None, None)


def _cem(lib, horizon=H, k=K, n_elites=2, discount=1.0, value={}, **_):
    return lib.emei_plan_cem_value(None, horizon, k, n_elites, 7, None, 0.0, None, discount, _value(value), None, P, P, None, P, P, None,
                                   None)


HORIZON = [({"horizon": 0}, "horizon=0 < 1"), ({"horizon": -4}, "horizon=-4 < 1")]
COUNT = [({"k": 0}, "n_candidates=0 < 1")]
N_ELITES = [({"n_elites": 0}, "n_elites=0 is outside [1, n_candidates=5]"), ({"n_elites": K + 1}, "n_elites=6 is outside [1, n_candidates=5]")]
DISCOUNT = [({"discount": 0.0}, "discount=0 is outside (0, 1]"), ({"discount": 1.5}, "discount=1.5 is outside (0, 1]"),
            ({"discount": NAN}, "discount=nan is outside (0, 1]")]
TEMPERATURE = [({"temperature": 0.0}, "temperature=0 must be finite and > 0"), ({"temperature": INF}, "temperature=inf must be finite and > 0"),
               ({"temperature": NAN}, "temperature=nan must be finite and > 0")]
VALUE = [({"value": None}, "null value"),
         ({"value": {"struct_size": 48}}, "value.struct_size=48 != sizeof(emei_policy_deep)=72"),
         ({"value": {"hidden1": 0}}, "value.hidden1=0 is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=256]"),
         ({"value": {"hidden1": 257}}, "value.hidden1=257 is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=256]"),
         ({"value": {"hidden2": 0}}, "value.hidden2=0 is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=256]"),
         ({"value": {"hidden2": 257}}, "value.hidden2=257 is outside [1, EMEI_POLICY_DEEP_MAX_HIDDEN=256]"),
         ({"value": {"reserved": 2 ** 40}}, "value.reserved=1099511627776 must be 0")]
# entry point -> (its call, [(bad arguments, message)] in the order of its refusals); "null handle" ends every list
TABLE = {
    "emei_evaluate_sequences_value": (_evaluate, HORIZON + COUNT + DISCOUNT + VALUE),
    "emei_plan_shooting_value": (_shooting, HORIZON + COUNT + DISCOUNT + VALUE),
    "emei_plan_mppi_value": (_mppi, HORIZON + COUNT + DISCOUNT + TEMPERATURE + VALUE),
    "emei_plan_cem_value": (_cem, HORIZON + COUNT + N_ELITES + DISCOUNT + VALUE),
}
SINGLE = [(fn, i) for fn, (_, rows) in TABLE.items() for i in range(len(rows))]


def _refused(fn, over):
    lib = _lib.lib()
    rc = TABLE[fn][0](lib, **over)
    return rc, lib.emei_last_error().decode()


def _merge(a, b):
    """both sets of bad arguments in one call, or None where they name the same argument (the same field of the struct)"""
    out = dict(a)
    for key, v in b.items():
        if key not in out:
            out[key] = v
        elif isinstance(v, dict) and isinstance(out[key], dict) and not set(v) & set(out[key]):
            out[key] = dict(out[key], **v)
        else:
            return None
    return out


@pytest.mark.parametrize("fn,i", SINGLE, ids=[f"{fn}-{i}" for fn, i in SINGLE])
def test_one_bad_argument(fn, i):
    over, text = TABLE[fn][1][i]
    assert _refused(fn, over) == (_lib.ERR_INVALID, f"{fn}: {text}"), over


@pytest.mark.parametrize("fn", sorted(TABLE))
def test_all_good_names_the_handle(fn):
    assert _refused(fn, {}) == (_lib.ERR_INVALID, f"{fn}: null handle")
    # the value's out_mode is ignored, the edges of its widths pass, and its weights come after the handle
    for value in ({"out_mode": 7}, {"out_mode": -1}, {"hidden1": 1, "hidden2": 256}, {"hidden1": 256, "hidden2": 1},
                  {"w1": None}, {"b3": None}, {"w1": None, "b1": None, "w2": None, "b2": None, "w3": None, "b3": None}):
        assert _refused(fn, {"value": value}) == (_lib.ERR_INVALID, f"{fn}: null handle"), value


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


def test_cem_reads_n_elites_only_with_a_good_shape():
    assert _refused("emei_plan_cem_value", {"k": 0, "n_elites": 0}) == (_lib.ERR_INVALID, "emei_plan_cem_value: n_candidates=0 < 1")


def test_workspace_is_the_cem_workspace():
    lib = _lib.lib()
    fn = "emei_plan_value_workspace_bytes"
    for n, k in ((65, 3), (1, 1), (3, 64), (3, 70), (67, 5), (2, 5), (1, 2 ** 31 - 1)):
        got = lib.emei_plan_value_workspace_bytes(n, k)
        assert got == lib.emei_plan_cem_workspace_bytes(n, k) == 16 * ((n * k + 63) // 64 + n) + 8 * n * k, (n, k)
        assert got > lib.emei_plan_shooting_workspace_bytes(n, k)  # the shooting variant keeps every return
    for shape, text in (((0, 2), "n_envs=0"), ((2, 0), "n_candidates=0 < 1"),
                        ((2, 2 ** 30), "n_envs * n_candidates = 2147483648 exceeds 2^31 - 1"), ((2 ** 31, 1), "n_envs=2147483648")):
        assert lib.emei_plan_cem_workspace_bytes(*shape) < 0
        assert (lib.emei_plan_value_workspace_bytes(*shape), lib.emei_last_error().decode()) == (_lib.ERR_INVALID, f"{fn}: {text}"), shape


# ---------------------------------------------------------------------------------------------- the Python layer, on CPU tensors
torch = pytest.importorskip("torch")


def _engine(name, obs_dim, act_dim, n=3):
    """what the checks of the Python layer read of an Engine, without a handle (and the checker itself, which needs none)"""
    from emei_amd.engine import Engine

    return type("E", (), dict(env_name=name, obs_dim=obs_dim, act_dim=act_dim, n_envs=n, device=torch.device("cpu"),
                              _plan_value=Engine._plan_value))()


def _critic(obs_dim, h1, h2, n_out=1):
    torch.manual_seed(100 * h1 + h2)
    lin, relu = torch.nn.Linear, torch.nn.ReLU
    return torch.nn.Sequential(lin(obs_dim, h1), relu(), lin(h1, h2), relu(), lin(h2, n_out))


def test_from_module_round_trips_a_sequential():
    import emei_amd
    from emei_amd.policy import DeepValueFunction

    assert emei_amd.DeepValueFunction is DeepValueFunction
    seq = _critic(11, 9, 2)
    val = DeepValueFunction.from_module(seq)
    assert type(val) is DeepValueFunction and (val.obs_dim, val.hidden1, val.hidden2) == (11, 9, 2)
    for k, m, what in (("w1", 0, "weight"), ("b1", 0, "bias"), ("w2", 2, "weight"), ("b2", 2, "bias"), ("w3", 4, "weight"), ("b3", 4, "bias")):
        t = getattr(val, k)
        assert t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and torch.equal(t, getattr(seq[m], what).detach()), k
    # the same network as the six tensors spelled out, bit for bit, and close to the float32 module (whose sums are not the normative ones)
    by_hand = DeepValueFunction(seq[4].weight, seq[4].bias, seq[2].weight, seq[2].bias, seq[0].weight, seq[0].bias)
    x = torch.randn(7, 11, generator=torch.Generator().manual_seed(3))
    assert torch.equal(val(x), by_hand(x)) and val(x).dtype == torch.float32 and tuple(val(x).shape) == (7,)
    assert torch.allclose(val(x), seq(x)[:, 0].detach(), rtol=1e-5, atol=1e-5)
    assert val.to("cpu") is val and val.bind(_engine("HopperRunning", 11, 3)) is val
    s = val.struct()
    assert (s.struct_size, s.hidden1, s.hidden2, s.reserved, s.w1, s.b3) == (72, 9, 2, 0, val.w1.data_ptr(), val.b3.data_ptr())


def test_from_module_refuses_other_shapes():
    from emei_amd.policy import DeepValueFunction

    lin, relu, tanh = torch.nn.Linear, torch.nn.ReLU, torch.nn.Tanh
    for bad in ([lin(4, 1)], [lin(4, 8), relu(), lin(8, 1)], [lin(4, 8), tanh(), lin(8, 8), relu(), lin(8, 1)],
                [lin(4, 8), relu(), lin(8, 8), relu(), lin(8, 1), tanh()], [lin(4, 8), relu(), lin(8, 8), relu(), lin(8, 1), relu()], []):
        with pytest.raises(ValueError, match="from_module"):
            DeepValueFunction.from_module(torch.nn.Sequential(*bad))
    with pytest.raises(ValueError, match="bias"):
        DeepValueFunction.from_module(torch.nn.Sequential(lin(4, 3), relu(), lin(3, 2, bias=False), relu(), lin(2, 1)))
    with pytest.raises(ValueError, match="one output"):
        DeepValueFunction.from_module(_critic(4, 3, 2, n_out=2))
    with pytest.raises(ValueError, match="hidden1=257"):
        DeepValueFunction.from_module(_critic(4, 257, 2))
    with pytest.raises(TypeError):
        DeepValueFunction.from_module(lin(4, 1))  # not a sequence of modules


def test_value_is_a_keyword_of_every_open_loop_call():
    from emei_amd.engine import Engine
    from emei_amd.envs.base import HipEnv

    for fn in (Engine.evaluate_sequences, Engine.plan_shooting, Engine.plan_mppi, Engine.plan_cem, HipEnv.evaluate_action_sequences,
               HipEnv.plan_random_shooting, HipEnv.plan_mppi, HipEnv.plan_cem):
        p = inspect.signature(fn).parameters
        assert p["value"].default is None and list(p)[-1] == "value", fn  # appended: the positional order is what it was
    # the fused controllers take no value
    for fn in (Engine.mpc_mppi, Engine.mpc_cem):
        assert "value" not in inspect.signature(fn).parameters, fn


def test_engine_methods_reject_anything_but_a_deep_value_function():
    from emei_amd.engine import Engine
    from emei_amd.policy import DeepMLPPolicy, DeepValueFunction

    hopper = _engine("HopperRunning", 11, 3)
    val = DeepValueFunction.from_module(_critic(11, 9, 2))
    assert Engine._plan_value(hopper, None, "plan_mppi") is None
    s = Engine._plan_value(hopper, val, "plan_mppi")
    assert isinstance(s, _lib.EmeiPolicyDeep) and (s.hidden1, s.hidden2, s.w3) == (9, 2, val.w3.data_ptr())
    with pytest.raises(ValueError, match="obs_dim=4"):  # bound as plan_policy binds it: the shapes against the env
        Engine._plan_value(_engine("CartPoleBalancing", 4, 0), val, "plan_mppi")
    seq = _critic(11, 9, 2)
    actor = DeepMLPPolicy(seq[4].weight, seq[4].bias, seq[2].weight, seq[2].bias, seq[0].weight, seq[0].bias)
    acts = torch.zeros((2, 3, 4, 3))
    calls = {"evaluate_sequences": lambda v: Engine.evaluate_sequences.__wrapped__(hopper, acts, value=v),
             "plan_shooting": lambda v: Engine.plan_shooting.__wrapped__(hopper, 2, 4, 0, value=v),
             "plan_mppi": lambda v: Engine.plan_mppi.__wrapped__(hopper, 2, 4, 0, 1.0, value=v),
             "plan_cem": lambda v: Engine.plan_cem.__wrapped__(hopper, 2, 4, 2, 0, value=v)}
    for name, call in calls.items():
        for bad in (seq, actor, lambda o: o, 1.0, (val,)):
            with pytest.raises(TypeError, match=f"{name} takes an emei_amd.DeepValueFunction"):
                call(bad)
