"""emei_rollout_policy on the host: declared (additive under ABI 8), exported and bound; the header carries the history line, the
normative comment and the kernel ids; every refusal that needs no device comes back EMEI_ERR_INVALID with a message that starts
with `emei_rollout_policy:` and names the argument, for a NULL handle and before any HIP call (no GPU needed), in the header's order:
n_steps, the policy pointer, struct_size, hidden, out_mode, reserved, then the handle."""
import ctypes as C
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "emei_rollout_policy"


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    assert re.search(r"EMEI_API\s+int\s+emei_rollout_policy\s*\(", hdr)
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert re.search(r"#define\s+EMEI_POLICY_MAX_HIDDEN\s+1024\b", hdr) and _lib.POLICY_MAX_HIDDEN == 1024
    assert re.search(r"enum\s+emei_policy_out\s*\{\s*EMEI_POLICY_OUT_CLIP\s*=\s*0\s*,\s*EMEI_POLICY_OUT_TANH\s*=\s*1\s*\}", hdr)
    assert (_lib.POLICY_OUT_CLIP, _lib.POLICY_OUT_TANH) == (0, 1)
    for name, val, py in (("EMEI_KERNEL_PEND_POLICY", 15, _lib.KERNEL_PEND_POLICY), ("EMEI_KERNEL_BODY_POLICY", 16, _lib.KERNEL_BODY_POLICY),
                          ("EMEI_KERNEL_BODY_POLICY_RK4", 17, _lib.KERNEL_BODY_POLICY_RK4)):
        assert re.search(name + r"\s*=\s*%d\b" % val, hdr) and py == val and "policy" in _lib.kernel_name(val), name
    assert sorted(_lib.POLICY_KERNEL_NAMES) == [15, 16, 17] and not set(_lib.POLICY_KERNEL_NAMES) & set(_lib.KERNEL_NAMES)
    assert _lib.kernel_name(5) == _lib.KERNEL_NAMES[5]  # one lookup for every id
    # the struct: field for field, and the binding's layout is the C layout (32 + 4 pointers)
    body = hdr[hdr.index("typedef struct emei_policy {"):hdr.index("} emei_policy;")]
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\s*\*?\s*(\w+);", body, re.M)
    assert [f[1] for f in fields] == ["struct_size", "hidden", "out_mode", "reserved", "w1", "b1", "w2", "b2"]
    assert [f[0] for f in _lib.EmeiPolicy._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.EmeiPolicy) == 16 + 4 * C.sizeof(C.c_void_p) and _lib.EmeiPolicy.w1.offset == 16
    # the history line, and a normative comment of its own in front of the prototype
    assert FN in hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    after = hdr[hdr.index("EMEI_API int emei_mpc_cem("):]
    comment = after[:after.index("enum emei_policy_out")]
    for word in ("Observe", "Policy", "Step", "ascending", "float64", "emei_get_obs", "emei_episode_init_obs", "fminf(fmaxf(", "tanh", "NaN gives lo",
                 "NaN gives 0", "Replay", "Chunking", "Sharding", "capturable", "work-queue", "EMEI_ERR_STATE", "EMEI_ERR_UNSUPPORTED",
                 "pend_policy_rollout_kernel", "body_policy_rollout_kernel", "DEVICE pointers"):
        assert word in comment, word
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert FN in _lib.SYMBOLS and FN in exported and hasattr(lib, FN)
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def test_refusals_with_a_null_handle():
    lib = _lib.lib()
    buf = {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in ("w1", "b1", "w2", "b2", "act", "obs", "rew", "done")}
    size = C.sizeof(_lib.EmeiPolicy)

    def call(n_steps=3, policy=True, struct_size=size, hidden=4, out_mode=0, reserved=0, w1=buf["w1"], b1=buf["b1"], w2=buf["w2"],
             b2=buf["b2"], dtype=_lib.ACT_U8, flags=0):
        pol = _lib.EmeiPolicy(struct_size, hidden, out_mode, reserved, w1, b1, w2, b2)
        rc = lib.emei_rollout_policy(None, n_steps, C.byref(pol) if policy else None, buf["act"], dtype, buf["obs"], buf["rew"],
                                     buf["done"], flags, None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and "null handle" in msg, msg
    cases = (({"n_steps": 0}, "n_steps"), ({"n_steps": -5}, "n_steps"), ({"policy": False}, "null policy"),
             ({"struct_size": 0}, "struct_size"), ({"struct_size": size - 8}, "struct_size"), ({"struct_size": size + 8}, "struct_size"),
             ({"hidden": -1}, "hidden"), ({"hidden": 1025}, "hidden"), ({"hidden": 2**31 - 1}, "hidden"),
             ({"out_mode": 2}, "out_mode"), ({"out_mode": -1}, "out_mode"), ({"reserved": 1}, "reserved"), ({"reserved": -7}, "reserved"))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and word in msg, (kw, rc, msg)
    # the edges pass the checks that need no handle: the handle is what is named
    for kw in ({"hidden": 0}, {"hidden": 1024}, {"out_mode": 1}, {"n_steps": 1}, {"n_steps": 2**31 - 1}):
        assert "null handle" in call(**kw)[1], kw
    # in the order of the header
    bad = {"n_steps": 0, "policy": False}
    assert "n_steps" in call(**bad)[1]
    del bad["n_steps"]
    assert "null policy" in call(**bad)[1]
    bad = {"struct_size": 1, "hidden": -1, "out_mode": 9, "reserved": 3}
    for key in ("struct_size", "hidden", "out_mode", "reserved"):
        msg = call(**bad)[1]
        assert key in msg and msg.startswith(FN + ":"), (key, msg)
        del bad[key]
    # what comes after the handle (the weights, the dtype, the flags) does not win over it
    assert "null handle" in call(w1=None, b1=None, w2=None, b2=None, dtype=77, flags=0xF0)[1]
    assert "reserved" in call(reserved=1, w2=None, dtype=77, flags=0xF0)[1]
    with pytest.raises(ValueError, match="n_steps"):
        _lib.check(call(n_steps=0)[0])
