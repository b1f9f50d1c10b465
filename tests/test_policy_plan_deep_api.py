"""emei_plan_policy_deep on the host: declared (additive under ABI 8), exported and bound; the header carries the history line and a
normative comment of its own, the terminal-value clause included; every refusal that needs no device comes back EMEI_ERR_INVALID with
a message that starts with `emei_plan_policy_deep:` and names the argument, for a NULL handle and before any HIP call (no GPU
needed), in the header's order: horizon, n_candidates, discount, the temperature where an output needs it, the policy struct, the
noise struct, the value struct, then the handle.  And the host logic of the Python layer on CPU tensors: the checker of the deep
route, the refusal of value= with a one-layer policy, and DeepValueFunction.__call__ against a Python-loop restatement of the value
clause, bit for bit."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "emei_plan_policy_deep"


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    proto = re.search(r"EMEI_API\s+int\s+emei_plan_policy_deep\s*\(([^;]*)\)\s*;", hdr)
    assert proto
    args = [a.strip() for a in " ".join(proto.group(1).split()).split(",")]
    assert args == ["emei_env* h", "int32_t horizon", "int32_t n_candidates", "const emei_policy_deep* policy",
                    "const emei_policy_noise* noise", "const emei_policy_deep* value", "double discount", "double temperature",
                    "const double* start_state", "void* workspace", "void* best_action_out", "int action_dtype", "float* mean_action_out",
                    "double* best_return_out", "int32_t* best_index_out", "int32_t* best_length_out", "double* return_out",
                    "double* ess_out", "void* stream"]
    sym = _lib.SYMBOLS[FN]
    assert sym[0] is C.c_int and len(sym[1]) == len(args) == 19
    assert sym[1][3]._type_ is _lib.EmeiPolicyDeep and sym[1][4]._type_ is _lib.EmeiPolicyNoise and sym[1][5]._type_ is _lib.EmeiPolicyDeep
    assert sym[1][6] is C.c_double and sym[1][7] is C.c_double
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    history = hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    assert FN in history and "terminal value" in history
    # the prototype and its comment stand after emei_evaluate_policies_deep's prototype: nothing new in front of the deep struct
    assert FN not in hdr[hdr.index("#define EMEI_ABI_VERSION"):hdr.index("#define EMEI_POLICY_DEEP_MAX_HIDDEN")]
    after = hdr[hdr.index("EMEI_API int emei_evaluate_policies_deep("):]
    comment = after[:after.index("EMEI_API int emei_plan_policy_deep(")]
    for word in ("emei_plan_policy's text clause for clause", "Start and observe", "Step and score", "Select", "Weights",
                 "emei_rollout_policy_deep", "float64 ascending sums", "rounded to float32", "NaN gives 0", "added last",
                 "ws [n_out, hidden2]", "epsilon-greedy", "philox4x32_10", "key = seed + t (mod 2^64)", "(g lo, g hi, k, m >> 2)",
                 "Candidate 0 takes NO noise", "-0.0", "non-finite std", "never explores",
                 "3b. Terminal value", "n_out = 1", "w3 [1, hidden2]", "b3 [1]", "widths are its own", "out_mode is ignored",
                 "ret = ret + g_H * (double)v", "after `horizon` multiplications", "v = (float)y_0", "x_H", "step horizon - 1 emits",
                 "no output", "NaN y_0 stays NaN", "planner's order puts it last", "rounded to float64", "no fused multiply-add",
                 "terminated gets nothing", "the last one included", "L(i, k) is unchanged", "bootstrapped returns",
                 "`value` NULL: no bootstrap", "emei_evaluate_policies_deep with n_policies = 1", "emei_evaluate_sequences",
                 "pend_policy_plan_deep_kernel", "body_policy_plan_deep_kernel", "ONE-WAVE", "dynamic LDS", "64 KiB",
                 "plan_policy_finish_kernel", "emei_plan_policy_workspace_bytes", "DEVICE pointers", "EMEI_ERR_INVALID",
                 "value.struct_size", "value.hidden1", "value.hidden2", "value.reserved", "NULL workspace", "2^31 - 1", "EMEI_ERR_STATE"):
        assert word in comment, word
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert FN in exported and hasattr(lib, FN)
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def test_no_kernel_id_and_no_struct_change():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    enum = hdr[hdr.index("enum emei_kernel_id {"):]
    enum = enum[:enum.index("};")]
    ids = [int(v) for v in re.findall(r"EMEI_KERNEL_\w+\s*=\s*(\d+)", enum)]
    assert ids == list(range(24)) and "plan_policy" not in enum and "POLICY_PLAN" not in enum
    assert C.sizeof(_lib.EmeiPolicy) == 48 and C.sizeof(_lib.EmeiPolicyDeep) == 72 and C.sizeof(_lib.EmeiPolicyNoise) == 64
    assert C.sizeof(_lib.EmeiConfig) == 408
    # no workspace function of its own
    assert "emei_plan_policy_deep_workspace_bytes" not in hdr and "emei_plan_policy_deep_workspace_bytes" not in _lib.SYMBOLS


def _caller():
    lib = _lib.lib()
    names = ("w1", "b1", "w2", "b2", "w3", "b3", "std", "ws", "bs", "work", "act", "mean", "ret", "idx", "len", "rets", "ess", "start")
    buf = {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in names}
    psize, nsize = C.sizeof(_lib.EmeiPolicyDeep), C.sizeof(_lib.EmeiPolicyNoise)
    W = ("w1", "b1", "w2", "b2", "w3", "b3")

    def call(horizon=3, n_candidates=5, policy=True, p_size=psize, hidden1=4, hidden2=3, out_mode=0, p_reserved=0, p_null=None, noise=True,
             struct_size=nsize, mode=0, seed=7, sigma=0.5, std=None, ws=None, bs=None, lmin=-20.0, lmax=2.0, reserved=0,
             value=False, v_size=psize, v_hidden1=9, v_hidden2=2, v_out_mode=0, v_reserved=0, v_null=None, discount=1.0, temperature=1.0,
             start=None, work=buf["work"], act=buf["act"], dtype=_lib.ACT_F32, mean=buf["mean"], ess=buf["ess"]):
        pw = [None if k == p_null else buf[k] for k in W]
        vw = [None if k == v_null else buf[k] for k in W]
        pol = _lib.EmeiPolicyDeep(p_size, hidden1, hidden2, out_mode, *pw, p_reserved)
        val = _lib.EmeiPolicyDeep(v_size, v_hidden1, v_hidden2, v_out_mode, *vw, v_reserved)
        nz = _lib.EmeiPolicyNoise(struct_size, mode, seed, sigma, std, ws, bs, lmin, lmax, reserved)
        rc = lib.emei_plan_policy_deep(None, horizon, n_candidates, C.byref(pol) if policy else None, C.byref(nz) if noise else None,
                                       C.byref(val) if value else None, discount, temperature, start, work, act, dtype, mean, buf["ret"],
                                       buf["idx"], buf["len"], buf["rets"], ess, None)
        return rc, lib.emei_last_error().decode()

    return call, buf, nsize, psize


def test_refusals_with_a_null_handle():
    call, buf, nsize, psize = _caller()
    nan, inf = float("nan"), float("inf")
    HEAD, EPS = _lib.POLICY_NOISE_GAUSS_HEAD, _lib.POLICY_NOISE_EPS_GREEDY
    head = dict(mode=HEAD, ws=buf["ws"], bs=buf["bs"])
    for kw in ({}, {"value": True}):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and "null handle" in msg, msg
    V = {"value": True}
    cases = (({"horizon": 0}, "horizon"), ({"horizon": -5}, "horizon"), ({"n_candidates": 0}, "n_candidates"), ({"n_candidates": -1}, "n_candidates"),
             ({"discount": 0.0}, "discount"), ({"discount": -0.5}, "discount"), ({"discount": 1.0000001}, "discount"), ({"discount": nan}, "discount"),
             ({"temperature": 0.0}, "temperature"), ({"temperature": -1.0}, "temperature"), ({"temperature": nan}, "temperature"),
             ({"temperature": inf}, "temperature"), ({"temperature": 0.0, "mean": None}, "temperature"), ({"temperature": 0.0, "ess": None}, "temperature"),
             ({"policy": False}, "null policy"), ({"p_size": 8}, "policy.struct_size"), ({"p_size": psize + 8}, "policy.struct_size"),
             ({"hidden1": 0}, "policy.hidden1"), ({"hidden1": 257}, "policy.hidden1"), ({"hidden2": 0}, "policy.hidden2"),
             ({"hidden2": 257}, "policy.hidden2"), ({"out_mode": 2}, "policy.out_mode"), ({"p_reserved": 1}, "policy.reserved"),
             ({"noise": False}, "null noise"),
             ({"struct_size": 0}, "noise.struct_size"), ({"struct_size": nsize - 8}, "noise.struct_size"), ({"struct_size": nsize + 8}, "noise.struct_size"),
             ({"mode": 3}, "noise.mode"), ({"mode": -1}, "noise.mode"), ({"reserved": 1}, "noise.reserved"), ({"reserved": -7}, "noise.reserved"),
             ({"sigma": -0.5}, "noise.sigma"), ({"sigma": nan}, "noise.sigma"), ({"sigma": inf}, "noise.sigma"),
             ({"mode": EPS, "sigma": -0.01}, "noise.sigma"), ({"mode": EPS, "sigma": 1.0000001}, "noise.sigma"), ({"mode": EPS, "sigma": nan}, "noise.sigma"),
             (dict(head, lmin=2.5), "noise.log_std_min"), (dict(head, lmin=nan), "noise.log_std_min"), (dict(head, lmax=nan), "noise.log_std_m"),
             (dict(head, ws=None), "null noise.ws"), (dict(head, bs=None), "null noise.bs"),
             (dict(V, v_size=8), "value.struct_size"), (dict(V, v_size=psize + 8), "value.struct_size"), (dict(V, v_hidden1=0), "value.hidden1"),
             (dict(V, v_hidden1=257), "value.hidden1"), (dict(V, v_hidden2=0), "value.hidden2"), (dict(V, v_hidden2=257), "value.hidden2"),
             (dict(V, v_reserved=1), "value.reserved"))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and word in msg, (kw, rc, msg)
    # the edges pass the checks that need no handle: the handle is what is named.  Without mean_action_out and ess_out the temperature
    # is neither consulted nor checked; the value's out_mode is ignored; a NULL value is checked for nothing
    for kw in ({"horizon": 1}, {"horizon": 2 ** 31 - 1}, {"n_candidates": 1}, {"n_candidates": 2 ** 31 - 1}, {"discount": 5e-324},
               {"hidden1": 1}, {"hidden1": 256}, {"hidden2": 1}, {"hidden2": 256}, {"out_mode": 1}, {"sigma": 0.0}, {"mode": EPS, "sigma": 1.0},
               dict(head, lmin=2.0, lmax=2.0), {"sigma": nan, "std": buf["std"]}, {"seed": 2 ** 64 - 1}, {"start": buf["start"]},
               {"temperature": 5e-324}, {"temperature": nan, "mean": None, "ess": None}, {"temperature": -1.0, "mean": None, "ess": None},
               dict(V, v_hidden1=1, v_hidden2=1), dict(V, v_hidden1=256, v_hidden2=256), dict(V, v_out_mode=2), dict(V, v_out_mode=-9),
               {"v_size": 8, "v_hidden1": 0, "v_reserved": 5}):
        assert "null handle" in call(**kw)[1], kw
    # in the order of the header
    bad = {"horizon": 0, "n_candidates": 0, "discount": 2.0, "temperature": 0.0, "policy": False, "noise": False, "value": True, "v_size": 1}
    for key, word in (("horizon", "horizon"), ("n_candidates", "n_candidates"), ("discount", "discount"), ("temperature", "temperature"),
                      ("policy", "null policy"), ("noise", "null noise"), ("v_size", "value.struct_size")):
        msg = call(**bad)[1]
        assert word in msg and msg.startswith(FN + ":"), (key, msg)
        del bad[key]
    bad = {"p_size": 1, "hidden1": 0, "hidden2": 0, "out_mode": 9, "p_reserved": 3, "struct_size": 1, "mode": 9, "reserved": 3, "sigma": -1.0,
           "value": True, "v_size": 1, "v_hidden1": 0, "v_hidden2": 0, "v_reserved": 3}
    for key, word in (("p_size", "policy.struct_size"), ("hidden1", "policy.hidden1"), ("hidden2", "policy.hidden2"),
                      ("out_mode", "policy.out_mode"), ("p_reserved", "policy.reserved"), ("struct_size", "noise.struct_size"),
                      ("mode", "noise.mode"), ("reserved", "noise.reserved"), ("sigma", "noise.sigma"), ("v_size", "value.struct_size"),
                      ("v_hidden1", "value.hidden1"), ("v_hidden2", "value.hidden2"), ("v_reserved", "value.reserved")):
        msg = call(**bad)[1]
        assert word in msg, (key, msg)
        del bad[key]
    assert "null handle" in call(**bad)[1]
    # what comes after the handle (the weights of the policy and of the value, the lanes, the dtype, the workspace, best_action_out, the
    # mode against the env kind) does not win over it
    assert "null handle" in call(p_null="w1", value=True, v_null="b3", dtype=77, work=None, act=None, n_candidates=2 ** 31 - 1)[1]
    assert "value.reserved" in call(value=True, v_reserved=1, p_null="w3", v_null="w1", dtype=77, work=None, act=None)[1]
    with pytest.raises(ValueError, match="n_candidates"):
        _lib.check(call(n_candidates=0)[0])


# ---------------------------------------------------------------------------------------------- the Python layer, on CPU tensors
torch = pytest.importorskip("torch")


def _engine(name, obs_dim, act_dim, n=3):
    return type("E", (), dict(env_name=name, obs_dim=obs_dim, act_dim=act_dim, n_envs=n, device=torch.device("cpu")))()


def _deep(obs_dim, h1, h2, n_out, out="clip", seed=0):
    from emei_amd.policy import DeepMLPPolicy

    g = torch.Generator().manual_seed(1000 * seed + 100 * h1 + 10 * h2 + obs_dim)
    r = lambda *s: torch.randn(*s, generator=g)
    return DeepMLPPolicy(r(n_out, h2), r(n_out), r(h2, h1), r(h2), r(h1, obs_dim), r(h1), out=out)


def _value(obs_dim, h1, h2, seed=0):
    from emei_amd.policy import DeepValueFunction

    g = torch.Generator().manual_seed(7000 + 1000 * seed + 100 * h1 + 10 * h2 + obs_dim)
    r = lambda *s: torch.randn(*s, generator=g)
    return DeepValueFunction(r(1, h2), r(1), r(h2, h1), r(h2), r(h1, obs_dim), r(h1))


def test_the_deep_route_has_a_checker_of_its_own():
    import emei_amd
    from emei_amd.engine import Engine
    from emei_amd.envs.base import HipEnv
    from emei_amd.policy import DeepValueFunction, PolicyNoise

    assert emei_amd.DeepValueFunction is DeepValueFunction
    for fn in (Engine.plan_policy, HipEnv.plan_policy):
        p = inspect.signature(fn).parameters
        assert p["value"].default is None and list(p)[-1] == "value", fn  # appended: the positional order is what it was
    check = Engine._plan_policy_deep_args
    hopper, cart = _engine("HopperRunning", 11, 3), _engine("CartPoleBalancing", 4, 0)
    pol, noise, val = _deep(11, 5, 3, 3), PolicyNoise(3, std=0.2), _value(11, 9, 2)
    H, K, ps, ns, vs, discount, temperature = check(hopper, 12, 70, pol, noise, None, 0.99, None)
    assert (H, K, vs, discount, temperature) == (12, 70, None, 0.99, None)
    assert isinstance(ps, _lib.EmeiPolicyDeep) and (ps.struct_size, ps.hidden1, ps.hidden2, ps.w3) == (72, 5, 3, pol.w3.data_ptr())
    assert (ns.struct_size, ns.mode, ns.seed, ns.sigma) == (64, 0, 3, 0.2)
    vs = check(hopper, 1, 1, pol, noise, val, 1.0, 0.5)[4]
    assert isinstance(vs, _lib.EmeiPolicyDeep) and (vs.struct_size, vs.hidden1, vs.hidden2, vs.reserved) == (72, 9, 2, 0)
    assert (vs.w1, vs.b3) == (val.w1.data_ptr(), val.b3.data_ptr())
    assert check(hopper, 1, 1, pol, noise, val, 1.0, 0.5)[6] == 0.5
    for kw, word in ((dict(H=0), "horizon"), (dict(K=0), "n_candidates"), (dict(discount=0.0), "discount"), (dict(discount=1.5), "discount"),
                     (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
                     (dict(temperature=float("inf")), "temperature")):
        a = dict(H=3, K=4, discount=1.0, temperature=None)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            check(hopper, a["H"], a["K"], pol, noise, val, a["discount"], a["temperature"])
    # shapes against the env, the noise mode against the env kind, the head against hidden2
    with pytest.raises(ValueError, match="obs_dim=11"):
        check(hopper, 3, 4, _deep(4, 5, 3, 3), noise, None, 1.0, None)
    with pytest.raises(ValueError, match="3 policy output"):
        check(hopper, 3, 4, _deep(11, 5, 3, 1), noise, None, 1.0, None)
    with pytest.raises(ValueError, match="obs_dim=11"):
        check(hopper, 3, 4, pol, noise, _value(4, 9, 2), 1.0, None)
    with pytest.raises(ValueError, match="continuous"):
        check(hopper, 3, 4, pol, PolicyNoise(3, epsilon=0.1), None, 1.0, None)
    with pytest.raises(ValueError, match="discrete"):
        check(cart, 3, 4, _deep(4, 5, 3, 1), PolicyNoise(3, std=0.1), None, 1.0, None)
    with pytest.raises(ValueError, match="3 policy output"):
        check(hopper, 3, 4, pol, PolicyNoise(3, std=[0.1, 0.2]), None, 1.0, None)
    with pytest.raises(ValueError, match="like the policy's w2"):  # a head of hidden1 = 5 columns: the head reads h2 (3 columns)
        check(hopper, 3, 4, pol, PolicyNoise(3, log_std_head=(torch.zeros(3, 5), torch.zeros(3))), None, 1.0, None)
    ns = check(hopper, 3, 4, pol, PolicyNoise(3, log_std_head=(torch.zeros(3, 3), torch.zeros(3))), None, 1.0, None)[3]
    assert ns.mode == _lib.POLICY_NOISE_GAUSS_HEAD
    assert check(cart, 3, 4, _deep(4, 5, 3, 1), PolicyNoise(3, epsilon=0.1), _value(4, 3, 4), 1.0, None)[3].mode == _lib.POLICY_NOISE_EPS_GREEDY
    with pytest.raises(TypeError, match="DeepMLPPolicy"):
        check(hopper, 3, 4, lambda o: o, noise, None, 1.0, None)
    with pytest.raises(TypeError, match="PolicyNoise"):
        check(hopper, 3, 4, pol, None, None, 1.0, None)
    with pytest.raises(TypeError, match="DeepValueFunction"):
        check(hopper, 3, 4, pol, noise, pol, 1.0, None)
    # the value network's own shape checks
    z = torch.zeros
    with pytest.raises(ValueError, match="one output"):
        DeepValueFunction(z(2, 3), z(2), z(3, 5), z(3), z(5, 11), z(5))
    with pytest.raises(ValueError, match="hidden1=257"):
        DeepValueFunction(z(1, 3), z(1), z(3, 257), z(3), z(257, 11), z(257))
    with pytest.raises(ValueError, match="hidden2"):
        DeepValueFunction(z(1, 4), z(1), z(3, 5), z(3), z(5, 11), z(5))


def test_value_with_a_one_layer_policy_is_refused_and_the_old_checker_is_what_it_was():
    from emei_amd.engine import Engine
    from emei_amd.policy import MLPPolicy, PolicyNoise

    hopper = _engine("HopperRunning", 11, 3)
    hopper._h = None  # never reached
    hopper._device_index = None
    noise, val = PolicyNoise(3, std=0.2), _value(11, 9, 2)
    one = MLPPolicy(torch.zeros(3, 5), torch.zeros(3), torch.zeros(5, 11), torch.zeros(5))
    plan = inspect.unwrap(Engine.plan_policy)
    with pytest.raises(ValueError, match="terminal value.* comes with the two-hidden-layer call"):
        plan(hopper, 3, 4, one, noise, value=val)
    # Engine._plan_policy_args stays the one-layer call's checker, its refusal of a DeepMLPPolicy included
    with pytest.raises(ValueError, match="two-hidden-layer network .* is not served by this call yet"):
        Engine._plan_policy_args(hopper, 3, 4, _deep(11, 5, 3, 3), noise, 1.0, None)
    assert list(inspect.signature(Engine._plan_policy_args).parameters) == ["self", "H", "K", "policy", "noise", "discount", "temperature"]


def _value_by_loops(v, obs):
    """the value clause of emei_plan_policy_deep restated with Python loops over numpy float64 scalars, every sum ascending"""
    f32, f64 = np.float32, np.float64
    w1, b1, w2, b2, w3, b3 = (getattr(v, k).numpy() for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    out = np.empty(len(obs), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for n, x in enumerate(np.asarray(obs, f32)):
            h1 = []
            for j in range(v.hidden1):
                z = f64(b1[j])
                for k in range(v.obs_dim):
                    z = z + f64(w1[j, k]) * f64(x[k])
                hj = f32(z)
                h1.append(hj if hj > 0 else f32(0))  # NaN gives 0
            h2 = []
            for i in range(v.hidden2):
                z = f64(b2[i])
                for j in range(v.hidden1):
                    z = z + f64(w2[i, j]) * f64(h1[j])
                hi = f32(z)
                h2.append(hi if hi > 0 else f32(0))
            y = f64(b3[0])
            for i in range(v.hidden2):
                y = y + f64(w3[0, i]) * f64(h2[i])
            out[n] = f32(y)  # no output clause
    return out


@pytest.mark.parametrize("h1,h2", [(5, 3), (9, 2)])
def test_value_function_call_is_the_value_clause_bit_for_bit(h1, h2):
    obs_dim = 11
    v = _value(obs_dim, h1, h2, seed=3)
    g = torch.Generator().manual_seed(h1 * h2)
    obs = (3.0 * torch.randn(40, obs_dim, generator=g)).to(torch.float32)
    obs[7, 2] = float("nan")  # a NaN input: every pre-activation it reaches is NaN, which the ReLU sends to 0
    got = v(obs)
    assert got.dtype == torch.float32 and tuple(got.shape) == (40,)
    want = _value_by_loops(v, obs.numpy())
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    # the cases the clause names are among the rows: a negative pre-activation (cut to 0) and a NaN one
    x = obs.to(torch.float64)
    z1 = v.b1.to(torch.float64)[None, :] + x @ v.w1.to(torch.float64).T
    assert bool((z1[torch.isfinite(z1).all(1)] < 0).any()) and bool(torch.isnan(z1[7]).any())
    assert np.isfinite(want[7])  # every unit of h1 saw the NaN: h1 = 0, the value is what the biases give
    # no output clause: a NaN bias of the last layer comes out as NaN
    v.b3[0] = float("nan")
    assert bool(torch.isnan(v(obs)).all())
