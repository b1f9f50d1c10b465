"""emei_plan_policy on the host: declared (additive under ABI 8), exported and bound; the header carries the history line and a
normative comment of its own; every refusal that needs no device comes back EMEI_ERR_INVALID with a message that starts with
`emei_plan_policy:` and names the argument, for a NULL handle and before any HIP call (no GPU needed), in the header's order: horizon,
n_candidates, discount, the temperature where an output needs it, the policy struct, the noise struct, then the handle.  The workspace
function and its negative cases.  And the host logic of Engine.plan_policy's argument checks and of the `candidate` argument of the
per-step twin, on CPU tensors."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "emei_plan_policy"
WS = "emei_plan_policy_workspace_bytes"


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    proto = re.search(r"EMEI_API\s+int\s+emei_plan_policy\s*\(([^;]*)\)\s*;", hdr)
    assert proto
    args = [a.strip() for a in " ".join(proto.group(1).split()).split(",")]
    assert args == ["emei_env* h", "int32_t horizon", "int32_t n_candidates", "const emei_policy* policy", "const emei_policy_noise* noise",
                    "double discount", "double temperature", "const double* start_state", "void* workspace", "void* best_action_out",
                    "int action_dtype", "float* mean_action_out", "double* best_return_out", "int32_t* best_index_out",
                    "int32_t* best_length_out", "double* return_out", "double* ess_out", "void* stream"]
    assert len(_lib.SYMBOLS[FN][1]) == len(args)
    ws = re.search(r"EMEI_API\s+int64_t\s+emei_plan_policy_workspace_bytes\s*\(([^;]*)\)\s*;", hdr)
    assert ws and [a.strip() for a in ws.group(1).split(",")] == ["int64_t n_envs", "int32_t n_candidates"]
    assert _lib.SYMBOLS[WS] == (C.c_int64, [C.c_int64, C.c_int32])
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    history = hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    assert FN in history and WS in history
    # a normative comment of its own, between emei_evaluate_policies' prototype and this one
    after = hdr[hdr.index("EMEI_API int emei_evaluate_policies("):]
    comment = after[:after.index("EMEI_API int emei_plan_policy(")]
    for word in ("Start and observe", "Policy", "Step and score", "Select", "Weights", "philox4x32_10", "key = seed + t (mod 2^64)",
                 "(g lo, g hi, k, m >> 2)", "Candidate 0 takes NO noise", "-0.0", "never explores", "never worse", "GAUSS_HEAD", "EPS_GREEDY",
                 "emei_evaluate_policies", "emei_rollout_policy_noisy", "emei_plan_mppi", "ties go to the lower k", "NaN comes last",
                 "k = l, l + 64", "d = 1, 2, .., 32", "best_action_out", "mean_action_out", "weighted share of action 1", "best_length_out",
                 "[n_envs, n_candidates]", "Z^2 / sum_k w_k^2", "neither consulted nor checked", "depend on g, not on the shard",
                 "capturable", "n_policies = 1", "n_candidates = 1 is legal", "emei_get_solver_cap_hits", "untouched",
                 "emei_last_rollout_kernel", "pend_policy_plan_kernel", "body_policy_plan_kernel", "plan_policy_finish_kernel", "scalar loads",
                 "STORES every candidate's action of step 0", "24 bytes per candidate", "16-byte aligned", "DEVICE pointers",
                 "EMEI_ERR_INVALID", "EMEI_ERR_STATE", "NULL workspace", "2^31 - 1"):
        assert word in comment, word
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    for name in (FN, WS):
        assert name in _lib.SYMBOLS and name in exported and hasattr(lib, name)
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def test_no_kernel_id_and_no_struct_change():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    enum = hdr[hdr.index("enum emei_kernel_id {"):]
    enum = enum[:enum.index("};")]
    ids = [int(v) for v in re.findall(r"EMEI_KERNEL_\w+\s*=\s*(\d+)", enum)]
    assert ids == list(range(24)) and "plan_policy" not in enum and "POLICY_PLAN" not in enum
    assert len(_lib.KERNEL_NAMES) == 15 and sorted(_lib.POLICY_KERNEL_NAMES) == [15, 16, 17]
    assert sorted(_lib.POLICY_NOISY_KERNEL_NAMES) == [18, 19, 20] and sorted(_lib.POLICY_DEEP_KERNEL_NAMES) == [21, 22, 23]
    assert C.sizeof(_lib.EmeiPolicy) == 48 and C.sizeof(_lib.EmeiPolicyNoise) == 64 and C.sizeof(_lib.EmeiConfig) == 408


def _caller():
    lib = _lib.lib()
    buf = {k: C.cast((C.c_double * 64)(), C.c_void_p)
           for k in ("w1", "b1", "w2", "b2", "std", "ws", "bs", "work", "act", "mean", "ret", "idx", "len", "rets", "ess", "start")}
    psize, nsize = C.sizeof(_lib.EmeiPolicy), C.sizeof(_lib.EmeiPolicyNoise)

    def call(horizon=3, n_candidates=5, policy=True, p_size=psize, hidden=4, out_mode=0, p_reserved=0, w2=buf["w2"], noise=True,
             struct_size=nsize, mode=0, seed=7, sigma=0.5, std=None, ws=None, bs=None, lmin=-20.0, lmax=2.0, reserved=0, discount=1.0,
             temperature=1.0, start=None, work=buf["work"], act=buf["act"], dtype=_lib.ACT_F32, mean=buf["mean"], ess=buf["ess"]):
        pol = _lib.EmeiPolicy(p_size, hidden, out_mode, p_reserved, buf["w1"], buf["b1"], w2, buf["b2"])
        nz = _lib.EmeiPolicyNoise(struct_size, mode, seed, sigma, std, ws, bs, lmin, lmax, reserved)
        rc = lib.emei_plan_policy(None, horizon, n_candidates, C.byref(pol) if policy else None, C.byref(nz) if noise else None, discount,
                                  temperature, start, work, act, dtype, mean, buf["ret"], buf["idx"], buf["len"], buf["rets"], ess, None)
        return rc, lib.emei_last_error().decode()

    return call, buf, nsize, psize


def test_refusals_with_a_null_handle():
    call, buf, nsize, psize = _caller()
    nan, inf = float("nan"), float("inf")
    HEAD, EPS = _lib.POLICY_NOISE_GAUSS_HEAD, _lib.POLICY_NOISE_EPS_GREEDY
    head = dict(mode=HEAD, ws=buf["ws"], bs=buf["bs"])
    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and "null handle" in msg, msg
    cases = (({"horizon": 0}, "horizon"), ({"horizon": -5}, "horizon"), ({"n_candidates": 0}, "n_candidates"), ({"n_candidates": -1}, "n_candidates"),
             ({"discount": 0.0}, "discount"), ({"discount": -0.5}, "discount"), ({"discount": 1.0000001}, "discount"), ({"discount": nan}, "discount"),
             ({"temperature": 0.0}, "temperature"), ({"temperature": -1.0}, "temperature"), ({"temperature": nan}, "temperature"),
             ({"temperature": inf}, "temperature"), ({"temperature": 0.0, "mean": None}, "temperature"), ({"temperature": 0.0, "ess": None}, "temperature"),
             ({"policy": False}, "null policy"), ({"p_size": 8}, "policy.struct_size"), ({"p_size": psize + 8}, "policy.struct_size"),
             ({"hidden": -1}, "policy.hidden"), ({"hidden": 1025}, "policy.hidden"), ({"out_mode": 2}, "policy.out_mode"),
             ({"p_reserved": 1}, "policy.reserved"),
             ({"noise": False}, "null noise"),
             ({"struct_size": 0}, "noise.struct_size"), ({"struct_size": nsize - 8}, "noise.struct_size"), ({"struct_size": nsize + 8}, "noise.struct_size"),
             ({"mode": 3}, "noise.mode"), ({"mode": -1}, "noise.mode"), ({"reserved": 1}, "noise.reserved"), ({"reserved": -7}, "noise.reserved"),
             ({"sigma": -0.5}, "noise.sigma"), ({"sigma": nan}, "noise.sigma"), ({"sigma": inf}, "noise.sigma"),
             ({"mode": EPS, "sigma": -0.01}, "noise.sigma"), ({"mode": EPS, "sigma": 1.0000001}, "noise.sigma"), ({"mode": EPS, "sigma": nan}, "noise.sigma"),
             (dict(head, lmin=2.5), "noise.log_std_min"), (dict(head, lmin=nan), "noise.log_std_min"), (dict(head, lmax=nan), "noise.log_std_m"),
             (dict(head, ws=None), "null noise.ws"), (dict(head, bs=None), "null noise.bs"))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and word in msg, (kw, rc, msg)
    # the edges pass the checks that need no handle: the handle is what is named.  Without mean_action_out and ess_out the temperature
    # is neither consulted nor checked
    for kw in ({"horizon": 1}, {"horizon": 2 ** 31 - 1}, {"n_candidates": 1}, {"n_candidates": 2 ** 31 - 1}, {"discount": 5e-324}, {"hidden": 0},
               {"hidden": 1024}, {"out_mode": 1}, {"sigma": 0.0}, {"mode": EPS, "sigma": 1.0}, dict(head, lmin=2.0, lmax=2.0),
               {"sigma": nan, "std": buf["std"]}, {"seed": 2 ** 64 - 1}, {"start": buf["start"]}, {"temperature": 5e-324},
               {"temperature": nan, "mean": None, "ess": None}, {"temperature": -1.0, "mean": None, "ess": None}):
        assert "null handle" in call(**kw)[1], kw
    # in the order of the header
    bad = {"horizon": 0, "n_candidates": 0, "discount": 2.0, "temperature": 0.0, "policy": False, "noise": False}
    for key, word in (("horizon", "horizon"), ("n_candidates", "n_candidates"), ("discount", "discount"), ("temperature", "temperature"),
                      ("policy", "null policy"), ("noise", "null noise")):
        msg = call(**bad)[1]
        assert word in msg and msg.startswith(FN + ":"), (key, msg)
        del bad[key]
    bad = {"p_size": 1, "hidden": -1, "out_mode": 9, "p_reserved": 3, "struct_size": 1, "mode": 9, "reserved": 3, "sigma": -1.0}
    for key, word in (("p_size", "policy.struct_size"), ("hidden", "policy.hidden"), ("out_mode", "policy.out_mode"),
                      ("p_reserved", "policy.reserved"), ("struct_size", "noise.struct_size"), ("mode", "noise.mode"), ("reserved", "noise.reserved")):
        msg = call(**bad)[1]
        assert word in msg, (key, msg)
        del bad[key]
    assert "noise.sigma" in call(**bad)[1]
    # what comes after the handle (the weights, the lanes, the dtype, the workspace, best_action_out, the mode against the env kind)
    # does not win over it
    assert "null handle" in call(w2=None, dtype=77, work=None, act=None, n_candidates=2 ** 31 - 1)[1]
    assert "noise.reserved" in call(reserved=1, w2=None, dtype=77, work=None, act=None)[1]
    with pytest.raises(ValueError, match="n_candidates"):
        _lib.check(call(n_candidates=0)[0])


def test_the_shared_checks_keep_their_messages():
    lib = _lib.lib()
    pol = _lib.EmeiPolicy(C.sizeof(_lib.EmeiPolicy), -1, 0, 0, None, None, None, None)
    assert lib.emei_rollout_policy(None, 3, C.byref(pol), None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_rollout_policy: policy.hidden=-1 is outside [0, EMEI_POLICY_MAX_HIDDEN=1024]"
    assert lib.emei_rollout_policy_noisy(None, 3, None, None, None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_rollout_policy_noisy: null policy"
    assert lib.emei_plan_mppi(None, 3, 2, 0, None, 0.0, 1.0, 0.0, None, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_plan_mppi: temperature=0 must be finite and > 0"


def test_workspace_bytes():
    lib = _lib.lib()
    f, mppi = lib.emei_plan_policy_workspace_bytes, lib.emei_plan_mppi_workspace_bytes
    for n, k in ((1, 1), (3, 70), (67, 5), (256, 64), (4096, 1000), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1)):
        # emei_plan_mppi's workspace plus six float32 slots per candidate for the stored actions of step 0
        assert f(n, k) == mppi(n, k) + 24 * n * k and f(n, k) % 8 == 0, (n, k)
    for n, k in ((0, 1), (-1, 1), (1, 0), (1, -1), (2 ** 31, 1), (2 ** 16, 2 ** 15), (2 ** 40, 1)):
        assert f(n, k) == _lib.ERR_INVALID, (n, k)
        assert lib.emei_last_error().decode().startswith(WS + ":")


# ---------------------------------------------------------------------------------------------- the Python layer, on CPU tensors
torch = pytest.importorskip("torch")


def _engine(name, obs_dim, act_dim, n=3):
    return type("E", (), dict(env_name=name, obs_dim=obs_dim, act_dim=act_dim, n_envs=n, device=torch.device("cpu")))()


def _policy(obs_dim, hidden, n_out, out="clip"):
    from emei_amd.policy import MLPPolicy

    g = torch.Generator().manual_seed(obs_dim + hidden)
    r = lambda *s: torch.randn(*s, generator=g)
    if hidden == 0:
        return MLPPolicy(r(n_out, obs_dim), r(n_out), out=out)
    return MLPPolicy(r(n_out, hidden), r(n_out), r(hidden, obs_dim), r(hidden), out=out)


def test_plan_policy_argument_checks():
    from emei_amd.engine import Engine
    from emei_amd.envs.base import HipEnv
    from emei_amd.policy import DeepMLPPolicy, PolicyNoise

    assert callable(Engine.plan_policy) and callable(HipEnv.plan_policy)
    sig = inspect.signature(Engine.plan_policy)
    assert list(sig.parameters)[1:5] == ["H", "K", "policy", "noise"]
    assert {k: sig.parameters[k].default for k in ("discount", "temperature", "start_state", "returns", "length", "ess")} == \
        dict(discount=1.0, temperature=None, start_state=None, returns=False, length=False, ess=False)
    check = Engine._plan_policy_args
    hopper, cart = _engine("HopperRunning", 11, 3), _engine("CartPoleBalancing", 4, 0)
    pol, noise = _policy(11, 5, 3), PolicyNoise(3, std=0.2)
    H, K, ps, ns, discount, temperature = check(hopper, 12, 70, pol, noise, 0.99, None)
    assert (H, K, discount, temperature) == (12, 70, 0.99, None)
    assert (ps.struct_size, ps.hidden, ps.w2) == (48, 5, pol.w2.data_ptr()) and (ns.struct_size, ns.mode, ns.seed, ns.sigma) == (64, 0, 3, 0.2)
    assert check(hopper, 1, 1, pol, noise, 1.0, 0.5)[5] == 0.5
    for kw, word in ((dict(H=0), "horizon"), (dict(K=0), "n_candidates"), (dict(discount=0.0), "discount"), (dict(discount=1.5), "discount"),
                     (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
                     (dict(temperature=float("inf")), "temperature")):
        a = dict(H=3, K=4, discount=1.0, temperature=None)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            check(hopper, a["H"], a["K"], pol, noise, a["discount"], a["temperature"])
    # shapes against the env, the noise mode against the env kind
    with pytest.raises(ValueError, match="obs_dim=11"):
        check(hopper, 3, 4, _policy(4, 5, 3), noise, 1.0, None)
    with pytest.raises(ValueError, match="3 policy output"):
        check(hopper, 3, 4, _policy(11, 5, 1), noise, 1.0, None)
    with pytest.raises(ValueError, match="continuous"):
        check(hopper, 3, 4, pol, PolicyNoise(3, epsilon=0.1), 1.0, None)
    with pytest.raises(ValueError, match="discrete"):
        check(cart, 3, 4, _policy(4, 0, 1), PolicyNoise(3, std=0.1), 1.0, None)
    with pytest.raises(ValueError, match="3 policy output"):
        check(hopper, 3, 4, pol, PolicyNoise(3, std=[0.1, 0.2]), 1.0, None)
    with pytest.raises(ValueError, match="like the policy's w2"):
        check(hopper, 3, 4, pol, PolicyNoise(3, log_std_head=(torch.zeros(3, 4), torch.zeros(3))), 1.0, None)
    assert check(cart, 3, 4, _policy(4, 0, 1), PolicyNoise(3, epsilon=0.1), 1.0, None)[3].mode == _lib.POLICY_NOISE_EPS_GREEDY
    with pytest.raises(TypeError, match="MLPPolicy"):
        check(hopper, 3, 4, lambda o: o, noise, 1.0, None)
    with pytest.raises(TypeError, match="PolicyNoise"):
        check(hopper, 3, 4, pol, None, 1.0, None)
    # the two-hidden-layer network is a follow-up
    deep = DeepMLPPolicy(torch.zeros(3, 6), torch.zeros(3), torch.zeros(6, 5), torch.zeros(6), torch.zeros(5, 11), torch.zeros(5))
    with pytest.raises(ValueError, match="two-hidden-layer network .* is not served by this call yet"):
        check(hopper, 3, 4, deep, noise, 1.0, None)


def test_candidate_zero_is_the_default_of_the_twin():
    from emei_amd.policy import DeepMLPPolicy, MLPPolicy, PolicyNoise

    for fn in (PolicyNoise.draws, MLPPolicy.__call__, DeepMLPPolicy.__call__):
        p = inspect.signature(fn).parameters
        assert p["candidate"].default == 0 and list(p)[-1] == "candidate", fn
    assert list(inspect.signature(PolicyNoise.draws).parameters) == ["self", "engine", "t", "candidate"]
    assert list(inspect.signature(MLPPolicy.__call__).parameters) == ["self", "obs", "noise", "t", "candidate"]

    # draws(engine, t, candidate=k) asks the engine for candidates 0 .. k of the key seed + t and takes the k-th: the default is the
    # one-candidate request it always made
    class Eng:
        n_envs, device, _act_tail = 3, torch.device("cpu"), (2,)

        def __init__(self, act_dim):
            self.act_dim, self.calls = act_dim, []

        def sample_candidates(self, H, K, seed, nominal=None, sigma=None):
            self.calls.append((H, K, seed, sigma))
            tail = self._act_tail if self.act_dim else ()
            k = torch.arange(K, dtype=torch.float32).reshape((1, 1, K) + (1,) * len(tail))
            return (k + torch.zeros((H, self.n_envs, K) + tail)).to(torch.float32 if self.act_dim else torch.int64)

    eng, noise = Eng(2), PolicyNoise(10, std=0.5)
    z = noise.draws(eng, 4)
    assert eng.calls == [(1, 1, 14, 0.125)] and tuple(z.shape) == (3, 2) and (z == 0).all()
    z = noise.draws(eng, 4, candidate=6)
    assert eng.calls[-1] == (1, 7, 14, 0.125) and (z == 48.0).all()  # 8 * candidate 6's value
    eng, noise = Eng(0), PolicyNoise(10, epsilon=0.5)
    explore, coin = noise.draws(eng, 1)
    assert eng.calls == [(2, 1, 11, None)] and (explore == 0).all()
    explore, coin = noise.draws(eng, 1, 2)
    assert eng.calls[-1] == (2, 3, 11, None) and (explore == 2).all() and (coin == 2).all()
    with pytest.raises(ValueError, match="candidate"):
        noise.draws(eng, 1, -1)
