"""emei_mpc_policy_workspace_bytes / emei_mpc_policy on the host: declared (additive under ABI 8), exported and bound; the header
carries the history line and a normative comment of its own; the two kernel ids live in an enum of their own behind
emei_last_rollout_kernel, the first enum and every struct size are what they were; every refusal that needs no device comes back
EMEI_ERR_INVALID with a message that starts with `emei_mpc_policy:` and names the argument, for a NULL handle and before any HIP call
(no GPU needed), in the header's order: n_steps, horizon, n_candidates, discount, act_mode, the temperature where the call needs it,
the policy struct, the noise struct, then the handle.  The workspace function and its negative cases, and the host logic of the
Python layer's argument checks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "emei_mpc_policy"
WS = "emei_mpc_policy_workspace_bytes"


def _header():
    return open(os.path.join(ROOT, "include", "emei_hip.h")).read()


def test_declared_exported_and_bound():
    hdr = _header()
    proto = re.search(r"EMEI_API\s+int\s+emei_mpc_policy\s*\(([^;]*)\)\s*;", hdr)
    assert proto
    args = [a.strip() for a in " ".join(proto.group(1).split()).split(",")]
    assert args == ["emei_env* h", "int32_t n_steps", "int32_t horizon", "int32_t n_candidates", "const emei_policy* policy",
                    "const emei_policy_noise* noise", "uint64_t seed_stride", "int32_t act_mode", "double discount", "double temperature",
                    "void* workspace", "void* actions_out", "int action_dtype", "float* obs_out", "float* reward_out", "uint8_t* done_out",
                    "double* plan_return_out", "int32_t* plan_index_out", "double* ess_out", "uint32_t flags", "void* stream"]
    assert len(_lib.SYMBOLS[FN][1]) == len(args) and _lib.SYMBOLS[FN][0] is C.c_int
    assert _lib.SYMBOLS[FN][1][6] is C.c_uint64 and _lib.SYMBOLS[FN][1][7] is C.c_int32  # seed_stride, act_mode
    ws = re.search(r"EMEI_API\s+int64_t\s+emei_mpc_policy_workspace_bytes\s*\(([^;]*)\)\s*;", hdr)
    assert ws and [a.strip() for a in ws.group(1).split(",")] == ["int64_t n_envs", "int32_t n_candidates"]
    assert _lib.SYMBOLS[WS] == (C.c_int64, [C.c_int64, C.c_int32])
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    history = hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    assert FN in history and WS in history
    # a normative comment of its own, between emei_plan_policy_deep's prototype and the new ones, all in front of the
    # emei_last_rollout_kernel comment
    after = hdr[hdr.index("EMEI_API int emei_plan_policy_deep("):]
    comment = after[:after.index("EMEI_API int64_t emei_mpc_policy_workspace_bytes(")]
    for word in ("Plan", "Act", "Step", "noise.seed + t * seed_stride", "key = noise.seed + t * seed_stride + h (mod 2^64)",
                 "(g lo, g hi, k, m >> 2)", "Candidate 0 takes NO noise", "k = l, l + 64", "d = 1 .. 32", "plan_return_out[t, i] = r*",
                 "plan_index_out[t, i] = k*", "ess_out[t, i]", "EMEI_MPC_POLICY_ACT_BEST", "EMEI_MPC_POLICY_ACT_MEAN", "best_action_out",
                 "mean_action_out", "(mean >= 0.5f) ? 1 : 0", "Clause 4 of emei_mpc_mppi", "EMEI_FLAG_AUTO_RESET", "[n_steps, n_envs, 6]",
                 "Chunking", "(b, noise.seed + a * seed_stride)", "Replay", "emei_rollout", "Sharding", "capturable",
                 "n_candidates = 1 is the deterministic policy", "Seed stride", "no horizon cap", "one-layer struct emei_policy only",
                 "12 * n_envs * n_candidates", "8-byte aligned", "DEVICE pointers", "pend_mpc_policy_kernel", "body_mpc_policy_kernel",
                 "unknown act_mode", "unknown flags", "NULL workspace, then NULL actions_out", "a NULL handle", "2^31 - 1",
                 "EMEI_ERR_INVALID", "EMEI_ERR_STATE", "EMEI_ERR_UNSUPPORTED", "emei_compact_done"):
        assert word in comment, word
    # the refusal order, as the header states it
    order = ["n_steps < 1", "horizon < 1", "n_candidates < 1", "discount outside", "unknown act_mode", "temperature not finite",
             "policy.reserved", "NULL noise", "a NULL handle", "NULL w2 or", "n_envs * n_candidates > 2^31 - 1", "a wrong action_dtype",
             "unknown flags", "NULL workspace", "a GAUSS mode on a discrete env"]
    tail = " ".join(comment[comment.index("EMEI_ERR_INVALID before any HIP call"):].replace("\n *", " ").split())
    at = [tail.index(w) for w in order]
    assert at == sorted(at), list(zip(order, at))
    assert after.index(WS + "(") < after.index("EMEI_API int emei_mpc_policy(") < after.index("/* Which kernel the LAST emei_step")
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    for name in (FN, WS):
        assert name in _lib.SYMBOLS and name in exported and hasattr(lib, name)
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def test_kernel_ids_in_an_enum_of_their_own_and_no_struct_change():
    hdr = _header()
    enum = hdr[hdr.index("enum emei_kernel_id {"):]
    enum = enum[:enum.index("};")]
    ids = [int(v) for v in re.findall(r"EMEI_KERNEL_\w+\s*=\s*(\d+)", enum)]
    assert ids == list(range(24)) and "MPC_POLICY" not in enum  # the first enum is the list it was
    behind = hdr[hdr.index("EMEI_API int emei_last_rollout_kernel("):]
    second = behind[behind.index("enum emei_kernel_id_mpc_policy {"):]
    second = second[:second.index("};")]
    assert re.findall(r"(EMEI_KERNEL_\w+)\s*=\s*(\d+)", second) == [("EMEI_KERNEL_PEND_MPC_POLICY", "24"), ("EMEI_KERNEL_BODY_MPC_POLICY", "25")]
    assert "closed list" in behind[:behind.index("enum emei_kernel_id_mpc_policy {")]  # its comment says why it stands apart
    assert (_lib.KERNEL_PEND_MPC_POLICY, _lib.KERNEL_BODY_MPC_POLICY) == (24, 25)
    assert sorted(_lib.MPC_POLICY_KERNEL_NAMES) == [24, 25] and _lib.kernel_name(24) == "pend_mpc_policy_kernel"
    assert _lib.kernel_name(25) == "body_mpc_policy_kernel" and _lib.kernel_name(11) == _lib.KERNEL_NAMES[11]
    assert re.search(r"enum\s+emei_mpc_policy_act\s*\{\s*EMEI_MPC_POLICY_ACT_BEST\s*=\s*0\s*,\s*EMEI_MPC_POLICY_ACT_MEAN\s*=\s*1\s*\}", hdr)
    assert (_lib.MPC_POLICY_ACT_BEST, _lib.MPC_POLICY_ACT_MEAN) == (0, 1)
    assert len(_lib.KERNEL_NAMES) == 15 and sorted(_lib.POLICY_DEEP_KERNEL_NAMES) == [21, 22, 23]
    assert C.sizeof(_lib.EmeiPolicy) == 48 and C.sizeof(_lib.EmeiPolicyDeep) == 72 and C.sizeof(_lib.EmeiPolicyNoise) == 64
    assert C.sizeof(_lib.EmeiConfig) == 408


def test_workspace_bytes():
    lib = _lib.lib()
    f, mppi = lib.emei_mpc_policy_workspace_bytes, lib.emei_plan_mppi_workspace_bytes
    for n, k in ((1, 1), (3, 5), (3, 70), (67, 5), (256, 64), (4096, 1000), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1)):
        # a float64 return and a float32 first action per candidate, rounded up to the 8-byte records of the done-mask launch
        assert f(n, k) == (12 * n * k + 7) // 8 * 8 and f(n, k) % 8 == 0, (n, k)
    assert f(1, 1) == 16 and f(3, 5) == 184 and f(256, 64) == 12 * 256 * 64
    for n, k in ((0, 1), (-1, 1), (1, 0), (1, -1), (2 ** 31, 1), (2 ** 16, 2 ** 15), (2 ** 40, 1)):
        assert mppi(n, k) == _lib.ERR_INVALID, (n, k)  # negative where emei_plan_mppi_workspace_bytes is
        assert f(n, k) == _lib.ERR_INVALID, (n, k)
        assert lib.emei_last_error().decode().startswith(WS + ":")


def _caller():
    lib = _lib.lib()
    buf = {k: C.cast((C.c_double * 64)(), C.c_void_p)
           for k in ("w1", "b1", "w2", "b2", "std", "ws", "bs", "work", "act", "obs", "rew", "done", "ret", "idx", "ess")}
    psize, nsize = C.sizeof(_lib.EmeiPolicy), C.sizeof(_lib.EmeiPolicyNoise)

    def call(n_steps=2, horizon=3, n_candidates=5, policy=True, p_size=psize, hidden=4, out_mode=0, p_reserved=0, w2=buf["w2"], noise=True,
             struct_size=nsize, mode=0, seed=7, sigma=0.5, std=None, ws=None, bs=None, lmin=-20.0, lmax=2.0, reserved=0, stride=3,
             act_mode=_lib.MPC_POLICY_ACT_MEAN, discount=1.0, temperature=1.0, work=buf["work"], act=buf["act"], dtype=_lib.ACT_F32,
             ess=buf["ess"], flags=0):
        pol = _lib.EmeiPolicy(p_size, hidden, out_mode, p_reserved, buf["w1"], buf["b1"], w2, buf["b2"])
        nz = _lib.EmeiPolicyNoise(struct_size, mode, seed, sigma, std, ws, bs, lmin, lmax, reserved)
        rc = lib.emei_mpc_policy(None, n_steps, horizon, n_candidates, C.byref(pol) if policy else None, C.byref(nz) if noise else None,
                                 stride, act_mode, discount, temperature, work, act, dtype, buf["obs"], buf["rew"], buf["done"], buf["ret"],
                                 buf["idx"], ess, flags, None)
        return rc, lib.emei_last_error().decode()

    return call, buf, nsize, psize


def test_refusals_with_a_null_handle():
    call, buf, nsize, psize = _caller()
    nan, inf = float("nan"), float("inf")
    BEST, MEAN = _lib.MPC_POLICY_ACT_BEST, _lib.MPC_POLICY_ACT_MEAN
    HEAD, EPS = _lib.POLICY_NOISE_GAUSS_HEAD, _lib.POLICY_NOISE_EPS_GREEDY
    head = dict(mode=HEAD, ws=buf["ws"], bs=buf["bs"])
    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and "null handle" in msg, msg
    cases = (({"n_steps": 0}, "n_steps"), ({"n_steps": -3}, "n_steps"), ({"horizon": 0}, "horizon"), ({"horizon": -5}, "horizon"),
             ({"n_candidates": 0}, "n_candidates"), ({"n_candidates": -1}, "n_candidates"),
             ({"discount": 0.0}, "discount"), ({"discount": -0.5}, "discount"), ({"discount": 1.0000001}, "discount"), ({"discount": nan}, "discount"),
             ({"act_mode": 2}, "act_mode"), ({"act_mode": -1}, "act_mode"),
             ({"temperature": 0.0}, "temperature"), ({"temperature": -1.0}, "temperature"), ({"temperature": nan}, "temperature"),
             ({"temperature": inf}, "temperature"), ({"temperature": 0.0, "ess": None}, "temperature"),
             ({"temperature": 0.0, "act_mode": BEST}, "temperature"),  # ACT_BEST with an ess_out still weighs
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
    # the edges pass the checks that need no handle: the handle is what is named.  With ACT_BEST and no ess_out the temperature is
    # neither consulted nor checked; any seed stride is legal and there is no horizon cap
    for kw in ({"n_steps": 1}, {"n_steps": 2 ** 31 - 1}, {"horizon": 1}, {"horizon": 2 ** 31 - 1}, {"n_candidates": 1},
               {"n_candidates": 2 ** 31 - 1}, {"discount": 5e-324}, {"hidden": 0}, {"hidden": 1024}, {"out_mode": 1}, {"sigma": 0.0},
               {"mode": EPS, "sigma": 1.0}, dict(head, lmin=2.0, lmax=2.0), {"sigma": nan, "std": buf["std"]}, {"seed": 2 ** 64 - 1},
               {"stride": 0}, {"stride": 1}, {"stride": 2 ** 64 - 1}, {"temperature": 5e-324}, {"act_mode": BEST},
               {"temperature": nan, "act_mode": BEST, "ess": None}, {"temperature": -1.0, "act_mode": BEST, "ess": None}):
        assert "null handle" in call(**kw)[1], kw
    # in the order of the header: two (and more) violated at once, the earlier one is reported
    bad = {"n_steps": 0, "horizon": 0, "n_candidates": 0, "discount": 2.0, "act_mode": 7, "temperature": 0.0, "policy": False, "noise": False}
    for key, word in (("n_steps", "n_steps"), ("horizon", "horizon"), ("n_candidates", "n_candidates"), ("discount", "discount"),
                      ("act_mode", "act_mode"), ("temperature", "temperature"), ("policy", "null policy"), ("noise", "null noise")):
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
    for pair, word in ((dict(n_steps=0, horizon=0), "n_steps"), (dict(horizon=0, discount=0.0), "horizon"), (dict(discount=0.0, act_mode=5), "discount"),
                       (dict(act_mode=5, temperature=0.0), "act_mode"), (dict(temperature=0.0, policy=False), "temperature"),
                       (dict(p_reserved=1, noise=False), "policy.reserved"), (dict(noise=False, w2=None), "null noise")):
        assert word in call(**pair)[1], pair
    # what comes after the handle (the weights, the lanes, the dtype, the flags, the workspace, actions_out, the mode against the env
    # kind) does not win over it
    assert "null handle" in call(w2=None, dtype=77, flags=6, work=None, act=None, n_candidates=2 ** 31 - 1)[1]
    assert "noise.reserved" in call(reserved=1, w2=None, dtype=77, flags=6, work=None, act=None)[1]
    with pytest.raises(ValueError, match="n_steps"):
        _lib.check(call(n_steps=0)[0])


# ---------------------------------------------------------------------------------------------- the Python layer, on CPU tensors
torch = pytest.importorskip("torch")


def test_python_layer_signatures_and_host_checks():
    from emei_amd import datasets
    from emei_amd.engine import Engine
    from emei_amd.envs.base import HipEnv
    from emei_amd.policy import DeepMLPPolicy, MLPPolicy, PolicyNoise

    sig = inspect.signature(Engine.mpc_policy)
    assert list(sig.parameters)[1:6] == ["T", "H", "K", "policy", "noise"]
    assert {k: sig.parameters[k].default for k in ("act", "temperature", "seed_stride", "discount", "auto_reset", "out", "diagnostics")} == \
        dict(act="best", temperature=None, seed_stride=None, discount=1.0, auto_reset=False, out=None, diagnostics=False)
    hsig = inspect.signature(HipEnv.mpc_policy)
    assert list(hsig.parameters)[1:6] == ["n_steps", "horizon", "n_candidates", "policy", "noise"] and hsig.parameters["auto_reset"].default is None
    eng = type("E", (), dict(env_name="CartPoleSwingUp", obs_dim=4, act_dim=0, n_envs=3, device=torch.device("cpu"),
                             _plan_policy_args=Engine._plan_policy_args))()
    eng.device = type("D", (), dict(index=0))()  # never reached: the refusals below come first
    pol, noise = MLPPolicy(torch.zeros(1, 4), torch.zeros(1)), PolicyNoise(3, epsilon=0.1)
    raw = Engine.mpc_policy.__wrapped__
    with pytest.raises(ValueError, match="n_steps"):
        raw(eng, 0, 3, 4, pol, noise)
    deep = DeepMLPPolicy(torch.zeros(1, 6), torch.zeros(1), torch.zeros(6, 5), torch.zeros(6), torch.zeros(5, 4), torch.zeros(5))
    with pytest.raises(NotImplementedError, match="plan_policy"):
        raw(eng, 2, 3, 4, deep, noise)
    with pytest.raises(ValueError, match="act="):
        raw(eng, 2, 3, 4, pol, noise, act="first")
    with pytest.raises(ValueError, match="needs a temperature"):
        raw(eng, 2, 3, 4, pol, noise, act="mean")
    # collect: the unknown planner's message names all three
    env = type("Env", (), dict(engine=type("E2", (), dict(n_envs=1, obs_dim=4, act_dim=0, device=torch.device("cpu"),
                                                             get_counters=lambda self: (None, None)))(),
                               reset=lambda self, seed=0, options=None: (torch.zeros(1, 4), {})))()
    with pytest.raises(ValueError, match="'mppi', 'cem' or 'policy'"):
        datasets.collect(env, 2, mpc=dict(planner="ilqr", horizon=3, n_candidates=4))
