"""emei_rollout_policy_deep / emei_evaluate_policies_deep on the host: declared (additive under ABI 8), exported and bound; the header
carries the history line, the normative comment, the struct and the kernel ids; struct emei_policy is what it was; every refusal that
precedes the handle comes back EMEI_ERR_INVALID with a message that starts with the function's name and names the argument, for a NULL
handle and before any HIP call (no GPU needed), in the header's order."""
import ctypes as C
import os
import re
import subprocess

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLL, EVAL = "emei_rollout_policy_deep", "emei_evaluate_policies_deep"
FIELDS = ["struct_size", "hidden1", "hidden2", "out_mode", "w1", "b1", "w2", "b2", "w3", "b3", "reserved"]


def _hdr():
    return open(os.path.join(ROOT, "include", "emei_hip.h")).read()


def _struct_fields(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n.strip().lstrip("*") for decl in re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*([\w\s,\*]+);", body, re.M) for n in decl.split(",")]


def test_declared_exported_and_bound():
    hdr = _hdr()
    args = lambda fn: [a.strip() for a in " ".join(re.search(r"EMEI_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % fn, hdr).group(1).split()).split(",")]
    assert args(ROLL) == ["emei_env* h", "int32_t n_steps", "const emei_policy_deep* policy", "const emei_policy_noise* noise",
                          "void* actions_out", "int action_dtype", "float* obs_out", "float* reward_out", "uint8_t* done_out",
                          "uint32_t flags", "void* stream"]
    assert args(EVAL) == ["emei_env* h", "int32_t horizon", "int32_t n_policies", "const emei_policy_deep* stacked", "double discount",
                          "const double* start_state", "double* return_out", "int32_t* length_out", "float* final_obs_out", "void* stream"]
    assert len(_lib.SYMBOLS[ROLL][1]) == 11 and len(_lib.SYMBOLS[EVAL][1]) == 10
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert re.search(r"#define\s+EMEI_POLICY_DEEP_MAX_HIDDEN\s+256\b", hdr) and _lib.POLICY_DEEP_MAX_HIDDEN == 256
    for name, val, py in (("EMEI_KERNEL_PEND_POLICY_DEEP", 21, _lib.KERNEL_PEND_POLICY_DEEP),
                          ("EMEI_KERNEL_BODY_POLICY_DEEP", 22, _lib.KERNEL_BODY_POLICY_DEEP),
                          ("EMEI_KERNEL_BODY_POLICY_DEEP_RK4", 23, _lib.KERNEL_BODY_POLICY_DEEP_RK4)):
        assert re.search(name + r"\s*=\s*%d\b" % val, hdr) and py == val and "deep" in _lib.kernel_name(val), name
    # the older tables keep their ids; one lookup serves all four
    assert sorted(_lib.POLICY_DEEP_KERNEL_NAMES) == [21, 22, 23] and sorted(_lib.POLICY_NOISY_KERNEL_NAMES) == [18, 19, 20]
    assert sorted(_lib.POLICY_KERNEL_NAMES) == [15, 16, 17] and len(_lib.KERNEL_NAMES) == 15
    assert _lib.kernel_name(16) == _lib.POLICY_KERNEL_NAMES[16] and _lib.kernel_name(19) == _lib.POLICY_NOISY_KERNEL_NAMES[19]
    # the history line and the normative comment
    assert ROLL in hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    assert EVAL in hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    after = hdr[hdr.index("EMEI_API int emei_evaluate_policies("):]
    comment = after[:after.index("#define EMEI_POLICY_DEEP_MAX_HIDDEN")]
    for word in ("ascending index order", "h1_j = (float)z", "h2_i = (float)z", "NaN gives 0", "(double)w3[q,i] * (double)h2_i",
                 "ws [n_out, hidden2]", "added last", "epsilon-greedy", "(seed + t, g)", "neither allocate nor synchronise", "ONE-WAVE",
                 "dynamic LDS", "pend_policy_rollout_deep_kernel", "body_policy_rollout_deep_kernel", "pend_policy_eval_deep_kernel",
                 "body_policy_eval_deep_kernel", "EMEI_ERR_INVALID", "EMEI_ERR_STATE", "EMEI_ERR_UNSUPPORTED", "DEVICE pointers"):
        assert word in comment, word
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    for fn in (ROLL, EVAL):
        assert fn in _lib.SYMBOLS and fn in exported and hasattr(lib, fn)
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def test_struct_layout_and_the_old_struct_is_untouched():
    hdr = _hdr()
    assert _struct_fields(hdr, "emei_policy_deep") == FIELDS
    D = _lib.EmeiPolicyDeep
    assert [f[0] for f in D._fields_] == FIELDS
    assert C.sizeof(D) == 72
    assert [getattr(D, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert D.reserved.size == 8 and D.hidden1.size == 4
    # struct emei_policy: its eight fields, 48 bytes, in the header and in the binding
    old = ["struct_size", "hidden", "out_mode", "reserved", "w1", "b1", "w2", "b2"]
    assert _struct_fields(hdr, "emei_policy") == old
    assert [f[0] for f in _lib.EmeiPolicy._fields_] == old and C.sizeof(_lib.EmeiPolicy) == 48
    assert _lib.SYMBOLS["emei_rollout_policy"][1][2]._type_ is _lib.EmeiPolicy
    assert _lib.SYMBOLS[ROLL][1][2]._type_ is D and _lib.SYMBOLS[EVAL][1][3]._type_ is D
    assert _lib.SYMBOLS[ROLL][1][3]._type_ is _lib.EmeiPolicyNoise


def _callers():
    lib = _lib.lib()
    names = ("w1", "b1", "w2", "b2", "w3", "b3", "std", "ws", "bs", "act", "obs", "rew", "done", "ret")
    buf = {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in names}
    psize, nsize = C.sizeof(_lib.EmeiPolicyDeep), C.sizeof(_lib.EmeiPolicyNoise)

    def policy(kw):
        w = {k: kw.pop(k, buf[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
        return _lib.EmeiPolicyDeep(kw.pop("p_size", psize), kw.pop("hidden1", 4), kw.pop("hidden2", 3), kw.pop("out_mode", 0), w["w1"], w["b1"],
                                   w["w2"], w["b2"], w["w3"], w["b3"], kw.pop("p_reserved", 0))

    def roll(**kw):
        pol = policy(kw) if kw.pop("policy", True) else None
        nz = None
        if kw.pop("noise", False):
            nz = _lib.EmeiPolicyNoise(kw.pop("struct_size", nsize), kw.pop("mode", 0), 7, kw.pop("sigma", 0.5), kw.pop("std", None),
                                      kw.pop("ws", None), kw.pop("bs", None), kw.pop("lmin", -20.0), kw.pop("lmax", 2.0), kw.pop("reserved", 0))
        rc = lib.emei_rollout_policy_deep(None, kw.pop("n_steps", 3), None if pol is None else C.byref(pol), None if nz is None else C.byref(nz),
                                          buf["act"], kw.pop("dtype", _lib.ACT_U8), buf["obs"], buf["rew"], buf["done"], kw.pop("flags", 0), None)
        assert not kw, kw
        return rc, lib.emei_last_error().decode()

    def evaluate(**kw):
        pol = policy(kw) if kw.pop("policy", True) else None
        rc = lib.emei_evaluate_policies_deep(None, kw.pop("horizon", 3), kw.pop("n_policies", 2), None if pol is None else C.byref(pol),
                                             kw.pop("discount", 0.99), None, kw.pop("ret", buf["ret"]), None, None, None)
        assert not kw, kw
        return rc, lib.emei_last_error().decode()

    return roll, evaluate, buf, psize, nsize


def test_sizeof_matches_the_binding():
    roll, evaluate, _, psize, _ = _callers()
    for call, fn in ((roll, ROLL), (evaluate, EVAL)):
        rc, msg = call(p_size=0)
        assert rc == _lib.ERR_INVALID and msg.startswith(fn + ":")
        assert int(re.search(r"sizeof\(emei_policy_deep\)=(\d+)", msg).group(1)) == psize == 72


def test_refusals_of_the_rollout_with_a_null_handle():
    roll, _, buf, psize, nsize = _callers()
    rc, msg = roll()
    assert rc == _lib.ERR_INVALID and msg.startswith(ROLL + ":") and "null handle" in msg, msg
    assert "null handle" in roll(noise=True)[1]
    head = dict(noise=True, mode=_lib.POLICY_NOISE_GAUSS_HEAD, ws=buf["ws"], bs=buf["bs"])
    nan = float("nan")
    cases = (({"n_steps": 0}, "n_steps"), ({"policy": False}, "null policy"), ({"p_size": 8}, "policy.struct_size"),
             ({"p_size": psize - 8}, "policy.struct_size"), ({"p_size": psize + 8}, "policy.struct_size"), ({"p_size": 48}, "policy.struct_size"),
             ({"hidden1": 0}, "policy.hidden1"), ({"hidden1": -1}, "policy.hidden1"), ({"hidden1": 257}, "policy.hidden1"),
             ({"hidden2": 0}, "policy.hidden2"), ({"hidden2": 257}, "policy.hidden2"), ({"hidden2": 1024}, "policy.hidden2"),
             ({"out_mode": 2}, "policy.out_mode"), ({"out_mode": -1}, "policy.out_mode"),
             ({"p_reserved": 1}, "policy.reserved"), ({"p_reserved": -(2 ** 40)}, "policy.reserved"), ({"p_reserved": 2 ** 32}, "policy.reserved"),
             (dict(noise=True, struct_size=0), "noise.struct_size"), (dict(noise=True, struct_size=nsize + 8), "noise.struct_size"),
             (dict(noise=True, mode=3), "noise.mode"), (dict(noise=True, reserved=1), "noise.reserved"),
             (dict(noise=True, sigma=-0.5), "noise.sigma"), (dict(noise=True, sigma=nan), "noise.sigma"),
             (dict(noise=True, mode=_lib.POLICY_NOISE_EPS_GREEDY, sigma=1.5), "noise.sigma"),
             (dict(head, lmin=2.5), "noise.log_std_min"), (dict(head, ws=None), "null noise.ws"), (dict(head, bs=None), "null noise.bs"))
    for kw, word in cases:
        rc, msg = roll(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith(ROLL + ":") and word in msg, (kw, rc, msg)
    # the edges pass: the handle is what is named
    for kw in ({"hidden1": 1, "hidden2": 1}, {"hidden1": 256, "hidden2": 256}, {"out_mode": 1}, dict(noise=True, sigma=0.0), head):
        assert "null handle" in roll(**kw)[1], kw
    # the header's order: scalars, NULL policy, struct_size, hidden1, hidden2, out_mode, reserved, the noise, the handle
    bad = dict(n_steps=0, p_size=1, hidden1=0, hidden2=0, out_mode=9, p_reserved=3, noise=True, struct_size=1, mode=9, reserved=3, sigma=-1.0)
    order = (("n_steps", "n_steps"), ("p_size", "policy.struct_size"), ("hidden1", "policy.hidden1"), ("hidden2", "policy.hidden2"),
             ("out_mode", "policy.out_mode"), ("p_reserved", "policy.reserved"), ("struct_size", "noise.struct_size"), ("mode", "noise.mode"),
             ("reserved", "noise.reserved"), ("sigma", "noise.sigma"))
    for key, word in order:
        msg = roll(**bad)[1]
        assert word in msg and msg.startswith(ROLL + ":"), (key, msg)
        del bad[key]
    assert "null handle" in roll(**bad)[1]
    assert "n_steps" in roll(n_steps=0, policy=False)[1] and "null policy" in roll(policy=False, noise=True, mode=9)[1]
    # what comes after the handle (the weights, the dtype, the flags, the mode against the env kind) does not win over it
    assert "null handle" in roll(w1=None, b3=None, dtype=77, flags=0xF0)[1]
    assert "policy.reserved" in roll(p_reserved=1, w1=None, dtype=77, flags=0xF0)[1]


def test_refusals_of_the_population_call_with_a_null_handle():
    _, evaluate, _, psize, _ = _callers()
    rc, msg = evaluate()
    assert rc == _lib.ERR_INVALID and msg.startswith(EVAL + ":") and "null handle" in msg, msg
    cases = (({"horizon": 0}, "horizon"), ({"n_policies": 0}, "n_policies"), ({"discount": 0.0}, "discount"), ({"discount": 1.5}, "discount"),
             ({"discount": float("nan")}, "discount"), ({"policy": False}, "null stacked"), ({"p_size": psize - 8}, "stacked.struct_size"),
             ({"p_size": psize + 8}, "stacked.struct_size"), ({"hidden1": 0}, "stacked.hidden1"), ({"hidden1": 257}, "stacked.hidden1"),
             ({"hidden2": 0}, "stacked.hidden2"), ({"hidden2": 257}, "stacked.hidden2"), ({"out_mode": 2}, "stacked.out_mode"),
             ({"p_reserved": 1}, "stacked.reserved"))
    for kw, word in cases:
        rc, msg = evaluate(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith(EVAL + ":") and word in msg, (kw, rc, msg)
    bad = dict(horizon=0, n_policies=0, discount=2.0, p_size=1, hidden1=0, hidden2=0, out_mode=9, p_reserved=3)
    order = (("horizon", "horizon"), ("n_policies", "n_policies"), ("discount", "discount"), ("p_size", "stacked.struct_size"),
             ("hidden1", "stacked.hidden1"), ("hidden2", "stacked.hidden2"), ("out_mode", "stacked.out_mode"), ("p_reserved", "stacked.reserved"))
    for key, word in order:
        msg = evaluate(**bad)[1]
        assert word in msg and msg.startswith(EVAL + ":"), (key, msg)
        del bad[key]
    assert "null handle" in evaluate(**bad)[1]
    assert "null handle" in evaluate(w2=None, ret=None)[1]  # the weights and return_out come after the handle


def test_the_messages_of_the_one_layer_calls_stay():
    lib = _lib.lib()
    pol = _lib.EmeiPolicy(C.sizeof(_lib.EmeiPolicy), -1, 0, 0, None, None, None, None)
    assert lib.emei_rollout_policy(None, 3, C.byref(pol), None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_rollout_policy: policy.hidden=-1 is outside [0, EMEI_POLICY_MAX_HIDDEN=1024]"
    for size in (40, 56):  # struct emei_policy did not grow
        pol = _lib.EmeiPolicy(size, 4, 0, 0, None, None, None, None)
        assert lib.emei_evaluate_policies(None, 3, 2, C.byref(pol), 1.0, None, None, None, None, None) == _lib.ERR_INVALID
        assert "stacked.struct_size" in lib.emei_last_error().decode()
    pol = _lib.EmeiPolicy(48, 4, 0, 7, None, None, None, None)  # ... and `reserved` is still reserved
    assert lib.emei_rollout_policy(None, 3, C.byref(pol), None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert "policy.reserved" in lib.emei_last_error().decode()
