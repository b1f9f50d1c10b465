"""emei_plan_shooting_workspace_bytes / emei_sample_candidates / emei_plan_shooting on the host: declared (additive under ABI 8),
exported and bound; every argument refusal comes back EMEI_ERR_INVALID with a message, for a NULL handle and before any HIP call
(no GPU needed); the workspace size is a pure host function."""
import ctypes as C
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("emei_plan_shooting_workspace_bytes", "emei_sample_candidates", "emei_plan_shooting")


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    assert re.search(r"EMEI_API\s+int64_t\s+emei_plan_shooting_workspace_bytes\s*\(", hdr)
    assert re.search(r"EMEI_API\s+int\s+emei_sample_candidates\s*\(", hdr)
    assert re.search(r"EMEI_API\s+int\s+emei_plan_shooting\s*\(", hdr)
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert "core.py:18-37,190-193" in hdr[hdr.index("Random-shooting planning"):hdr.index("emei_plan_shooting_workspace_bytes(")]
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    for name in NAMES:
        assert name in _lib.SYMBOLS and name in exported and hasattr(lib, name), name
    assert lib.emei_abi_version() == 8


def _buffers():
    return {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in ("ws", "act", "seq", "ret", "idx", "len", "nom")}


def test_plan_shooting_refusals_with_a_null_handle():
    lib = _lib.lib()
    b = _buffers()

    def call(horizon=4, k=8, discount=1.0, nominal=None, sigma=0.0, ws=b["ws"], act=b["act"], ret=b["ret"], idx=b["idx"]):
        rc = lib.emei_plan_shooting(None, horizon, k, 1234, nominal, sigma, discount, None, ws, act, _lib.ACT_U8, b["seq"], ret, idx,
                                    b["len"], None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and "emei_plan_shooting" in msg and "null handle" in msg, msg
    # the scalars are checked first: each refusal names its own argument
    for kw, word in (({"horizon": 0}, "horizon"), ({"horizon": -2}, "horizon"), ({"k": 0}, "n_candidates"), ({"k": -1}, "n_candidates"),
                     ({"discount": 0.0}, "discount"), ({"discount": 1.0000001}, "discount"), ({"discount": -1.0}, "discount"),
                     ({"discount": float("nan")}, "discount"), ({"discount": float("inf")}, "discount")):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and word in msg, (kw, rc, msg)
    # what needs the handle (is the env continuous?  how many envs?) and the pointers: refused, with a message, not dereferenced
    for kw in ({"nominal": b["nom"], "sigma": 0.0}, {"nominal": b["nom"], "sigma": -1.0}, {"nominal": b["nom"], "sigma": float("nan")},
               {"nominal": b["nom"], "sigma": float("inf")}, {"k": 2**31 - 1}, {"ws": None}, {"act": None}, {"ret": None}, {"idx": None}):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_plan_shooting"), (kw, rc, msg)
    with pytest.raises(ValueError, match="discount"):
        _lib.check(call(discount=2.0)[0])


def test_sample_candidates_refusals_with_a_null_handle():
    lib = _lib.lib()
    b = _buffers()

    def call(horizon=4, k=8, nominal=None, sigma=0.0, out=b["act"]):
        rc = lib.emei_sample_candidates(None, horizon, k, 1, nominal, sigma, out, _lib.ACT_U8, None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and "emei_sample_candidates" in msg and "null handle" in msg, msg
    for kw, word in (({"horizon": 0}, "horizon"), ({"k": 0}, "n_candidates")):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and word in msg, (kw, rc, msg)
    for kw in ({"nominal": b["nom"], "sigma": -1.0}, {"out": None}):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_sample_candidates"), (kw, rc, msg)


def test_workspace_bytes():
    f = _lib.lib().emei_plan_shooting_workspace_bytes
    assert f(1, 1) > 0
    ns, ks = (1, 3, 64, 65, 257, 4096, 100000), (1, 13, 63, 64, 65, 300, 4096)
    for a in range(len(ns)):
        for c in range(len(ks)):
            v = f(ns[a], ks[c])
            assert v > 0
            # one 16-byte record per (wave, env) segment: at most waves + envs of them
            assert v >= 16 * (-(-ns[a] * ks[c] // 64) + ns[a] - 1)
            if a:
                assert v >= f(ns[a - 1], ks[c])
            if c:
                assert v >= f(ns[a], ks[c - 1])
    assert f(1, 2**31 - 1) > 0 and f(2**31 - 1, 1) > 0  # the largest shapes the plan call takes
    for bad in ((0, 4), (-1, 4), (4, 0), (4, -7), (2, 2**30), (2**31, 1), (2**40, 1), (2**16, 2**15)):
        assert f(*bad) == _lib.ERR_INVALID, bad
        assert b"emei_plan_shooting_workspace_bytes" in _lib.lib().emei_last_error()
