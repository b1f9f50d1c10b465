"""emei_plan_mppi_workspace_bytes / emei_plan_mppi on the host: declared (additive under ABI 8), exported and bound; every argument
refusal comes back EMEI_ERR_INVALID with a message that names the argument, for a NULL handle and before any HIP call (no GPU
needed), the scalars first; the workspace size is a pure host function."""
import ctypes as C
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("emei_plan_mppi_workspace_bytes", "emei_plan_mppi")


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    assert re.search(r"EMEI_API\s+int64_t\s+emei_plan_mppi_workspace_bytes\s*\(", hdr)
    assert re.search(r"EMEI_API\s+int\s+emei_plan_mppi\s*\(", hdr)
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    # after emei_plan_shooting's prototype, with a normative comment of its own that cites the reference interface
    after = hdr[hdr.index("EMEI_API int emei_plan_shooting("):]
    comment = after[:after.index("emei_plan_mppi_workspace_bytes(")]
    assert "core.py:18-37,190-193" in comment and "temperature" in comment and "ess_out" in comment
    assert "emei_plan_mppi" in hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    for name in NAMES:
        assert name in _lib.SYMBOLS and name in exported and hasattr(lib, name), name
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def _buffers():
    return {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in ("ws", "out", "ret", "idx", "ess", "nom")}


def test_plan_mppi_refusals_with_a_null_handle():
    lib = _lib.lib()
    b = _buffers()

    def call(horizon=4, k=8, discount=1.0, temperature=1.0, nominal=None, sigma=0.0, ws=b["ws"], out=b["out"], ret=b["ret"],
             idx=b["idx"], ess=b["ess"]):
        rc = lib.emei_plan_mppi(None, horizon, k, 1234, nominal, sigma, discount, temperature, None, ws, out, ret, idx, ess, None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith("emei_plan_mppi") and "null handle" in msg, msg
    # the scalars are checked first: each refusal names its own argument
    for kw, word in (({"horizon": 0}, "horizon"), ({"horizon": -2}, "horizon"), ({"k": 0}, "n_candidates"), ({"k": -1}, "n_candidates"),
                     ({"discount": 0.0}, "discount"), ({"discount": 1.0000001}, "discount"), ({"discount": -1.0}, "discount"),
                     ({"discount": float("nan")}, "discount"), ({"discount": float("inf")}, "discount"),
                     ({"temperature": 0.0}, "temperature"), ({"temperature": -1.0}, "temperature"),
                     ({"temperature": float("nan")}, "temperature"), ({"temperature": float("inf")}, "temperature")):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_plan_mppi:") and word in msg, (kw, rc, msg)
    # in the order of the list: horizon before n_candidates before discount before temperature
    assert "horizon" in call(horizon=0, k=0, discount=0.0, temperature=0.0)[1]
    assert "n_candidates" in call(k=0, discount=0.0, temperature=0.0)[1]
    assert "discount" in call(discount=0.0, temperature=0.0)[1]
    # a bad scalar wins over the NULL handle and the NULL pointers; without one the handle is what is named
    assert "temperature" in call(temperature=0.0, ws=None, out=None)[1]
    assert "null handle" in call(ws=None, out=None)[1]
    # what needs the handle and the pointers: refused, with a message, nothing dereferenced
    for kw in ({"nominal": b["nom"], "sigma": 0.0}, {"nominal": b["nom"], "sigma": float("nan")}, {"k": 2**31 - 1}, {"ws": None},
               {"out": None}):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_plan_mppi:"), (kw, rc, msg)
    with pytest.raises(ValueError, match="temperature"):
        _lib.check(call(temperature=-3.0)[0])


def test_workspace_bytes():
    f, g = _lib.lib().emei_plan_mppi_workspace_bytes, _lib.lib().emei_plan_shooting_workspace_bytes
    assert f(1, 1) >= g(1, 1) + 8
    ns, ks = (1, 3, 64, 65, 257, 4096, 100000), (1, 13, 63, 64, 65, 300, 4096)
    for a in range(len(ns)):
        for c in range(len(ks)):
            v = f(ns[a], ks[c])
            # the shooting partials plus 8 bytes per candidate
            assert v >= g(ns[a], ks[c]) + 8 * ns[a] * ks[c]
            assert v % 8 == 0
            if a:
                assert v >= f(ns[a - 1], ks[c])
            if c:
                assert v >= f(ns[a], ks[c - 1])
    assert f(1, 2**31 - 1) >= g(1, 2**31 - 1) + 8 * (2**31 - 1) and f(2**31 - 1, 1) > 0  # the largest shapes the plan call takes
    for bad in ((0, 4), (-1, 4), (4, 0), (4, -7), (2, 2**30), (2**31, 1), (2**40, 1), (2**16, 2**15)):
        assert g(*bad) == _lib.ERR_INVALID, bad  # refused where the shooting size is
        assert f(*bad) == _lib.ERR_INVALID, bad
        assert b"emei_plan_mppi_workspace_bytes" in _lib.lib().emei_last_error()
