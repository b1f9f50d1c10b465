"""emei_mpc_cem_workspace_bytes / emei_mpc_cem on the host: declared (additive under ABI 8), exported and bound; every scalar
refusal comes back EMEI_ERR_INVALID with a message that starts with `emei_mpc_cem:` and names the argument, for a NULL handle and
before any HIP call (no GPU needed), in the order the header gives; the workspace size is the pure host function 8 * n * k."""
import ctypes as C
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("emei_mpc_cem_workspace_bytes", "emei_mpc_cem")
INF = float("inf")
NAN = float("nan")


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    assert re.search(r"EMEI_API\s+int64_t\s+emei_mpc_cem_workspace_bytes\s*\(", hdr)
    assert re.search(r"EMEI_API\s+int\s+emei_mpc_cem\s*\(", hdr)
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert re.search(r"EMEI_KERNEL_PEND_MPC_CEM\s*=\s*12\b", hdr) and _lib.KERNEL_PEND_MPC_CEM == 12 and 12 in _lib.KERNEL_NAMES
    # the history line, and a normative comment of its own between emei_mpc_mppi's prototype and the new ones
    assert "emei_mpc_cem" in hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    after = hdr[hdr.index("EMEI_API int emei_mpc_mppi("):]
    comment = after[:after.index("EMEI_API int64_t emei_mpc_cem_workspace_bytes(")]
    for word in ("Iterate", "Clamp", "Refit", "Act", "Step", "Warm start", "Chunking", "seed + t*iterations + j", "capturable",
                 "EMEI_ERR_UNSUPPORTED"):
        assert word in comment, word
    assert after.index("emei_mpc_cem_workspace_bytes(") < after.index("EMEI_API int emei_mpc_cem(") < after.index("enum emei_kernel_id")
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    for name in NAMES:
        assert name in _lib.SYMBOLS and name in exported and hasattr(lib, name), name
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def _buffers():
    return {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in ("nom", "ws", "act", "obs", "rew", "done", "ret", "elite")}


def test_mpc_cem_refusals_with_a_null_handle():
    lib = _lib.lib()
    b = _buffers()

    def call(n_steps=3, horizon=4, k=8, n_elites=2, iterations=3, sigma=0.5, sigma_min=0.05, discount=1.0, refill=0.5, lo=0.05, hi=0.95,
             nom=b["nom"], ws=b["ws"], act=b["act"]):
        rc = lib.emei_mpc_cem(None, n_steps, horizon, k, n_elites, iterations, 1234, nom, sigma, sigma_min, discount, refill, lo, hi, ws,
                              act, _lib.ACT_U8, b["obs"], b["rew"], b["done"], b["ret"], b["elite"], 0, None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith("emei_mpc_cem:") and "null handle" in msg, msg
    # the scalars are checked first: each refusal names its own argument
    cases = (({"n_steps": 0}, "n_steps"), ({"n_steps": -3}, "n_steps"), ({"horizon": 0}, "horizon"), ({"horizon": -2}, "horizon"),
             ({"k": 0}, "n_candidates"), ({"k": -1}, "n_candidates"),
             ({"n_elites": 0}, "n_elites"), ({"n_elites": -1}, "n_elites"), ({"n_elites": 9}, "n_elites"),
             ({"discount": 0.0}, "discount"), ({"discount": 1.0000001}, "discount"), ({"discount": -1.0}, "discount"),
             ({"discount": NAN}, "discount"), ({"discount": INF}, "discount"),
             ({"iterations": 0}, "iterations"), ({"iterations": -2}, "iterations"),
             ({"refill": NAN}, "refill"), ({"refill": INF}, "refill"), ({"refill": -INF}, "refill"),
             ({"lo": 0.9, "hi": 0.1}, "nominal_lo"), ({"lo": NAN}, "nominal_lo"), ({"hi": NAN}, "nominal_hi"),
             ({"sigma_min": -0.1}, "sigma_min"), ({"sigma_min": NAN}, "sigma_min"), ({"sigma_min": INF}, "sigma_min"),
             ({"horizon": 257}, "EMEI_MPC_MAX_HORIZON"), ({"horizon": 2**31 - 1}, "EMEI_MPC_MAX_HORIZON"))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_mpc_cem:") and word in msg, (kw, rc, msg)
    # no clamp (-inf, +inf), equal bounds, no floor, every candidate an elite and the largest horizon pass the scalar checks
    for kw in ({"lo": -INF, "hi": INF}, {"lo": 0.5, "hi": 0.5}, {"sigma_min": 0.0}, {"n_elites": 8}, {"n_elites": 1}, {"horizon": 256},
               {"iterations": 1}):
        assert "null handle" in call(**kw)[1], kw
    # in the order of the header: n_steps, horizon, n_candidates, n_elites, discount, iterations, refill, the clamp, sigma_min, the
    # horizon's cap, the handle
    bad = {"n_steps": 0, "horizon": 0, "k": 0, "n_elites": 0, "discount": 0.0, "iterations": 0, "refill": NAN, "lo": 1.0, "hi": 0.0,
           "sigma_min": -1.0}
    for key, word in (("n_steps", "n_steps"), ("horizon", "horizon"), ("k", "n_candidates"), ("n_elites", "n_elites"),
                      ("discount", "discount"), ("iterations", "iterations"), ("refill", "refill"), ("lo", "nominal_lo"),
                      ("sigma_min", "sigma_min")):
        msg = call(**bad)[1]
        assert word in msg and msg.startswith("emei_mpc_cem:"), (key, msg)
        del bad[key]
        if key == "horizon":
            bad["horizon"] = 300  # valid as a horizon, beyond the cap: the LAST scalar check
        if key == "lo":
            del bad["hi"]
    assert bad == {"horizon": 300} and "EMEI_MPC_MAX_HORIZON" in call(**bad)[1]
    # a bad scalar wins over the NULL handle and the NULL pointers; without one the handle is what is named
    assert "sigma_min" in call(sigma_min=-1.0, nom=None, ws=None, act=None)[1]
    assert "iterations" in call(iterations=0, nom=None, ws=None, act=None)[1]
    assert "null handle" in call(nom=None, ws=None, act=None)[1]
    with pytest.raises(ValueError, match="n_steps"):
        _lib.check(call(n_steps=0)[0])


def test_workspace_bytes():
    f, g = _lib.lib().emei_mpc_cem_workspace_bytes, _lib.lib().emei_plan_mppi_workspace_bytes
    for n in (1, 3, 64, 65, 257, 4096, 100000):
        for k in (1, 13, 63, 64, 65, 300, 4096):
            assert f(n, k) == 8 * n * k, (n, k)
    assert f(1, 2**31 - 1) == 8 * (2**31 - 1) and f(2**31 - 1, 1) == 8 * (2**31 - 1)  # the largest shapes the call takes
    for bad in ((0, 4), (-1, 4), (4, 0), (4, -7), (2, 2**30), (2**31, 1), (2**40, 1), (2**16, 2**15)):
        assert g(*bad) == _lib.ERR_INVALID, bad  # negative where emei_plan_mppi_workspace_bytes is
        assert f(*bad) == _lib.ERR_INVALID, bad
        assert b"emei_mpc_cem_workspace_bytes" in _lib.lib().emei_last_error()
