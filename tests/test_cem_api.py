"""emei_sample_candidates_sigma / emei_plan_cem_workspace_bytes / emei_plan_cem on the host: declared (additive under ABI 8), exported
and bound; every argument refusal that does not need a live handle comes back EMEI_ERR_INVALID with a message that names the
argument, for a NULL handle and before any HIP call (no GPU needed), the scalars first; the workspace size is a pure host function.
(The refusals that read the handle — a sigma_map on a discrete env, NULL workspace — are in tests/test_gpu_cem.py.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("emei_sample_candidates_sigma", "emei_plan_cem_workspace_bytes", "emei_plan_cem")


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    assert re.search(r"EMEI_API\s+int\s+emei_sample_candidates_sigma\s*\(", hdr)
    assert re.search(r"EMEI_API\s+int64_t\s+emei_plan_cem_workspace_bytes\s*\(", hdr)
    assert re.search(r"EMEI_API\s+int\s+emei_plan_cem\s*\(", hdr)
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    # after emei_plan_mppi's prototype, with a normative comment of its own: the order, the moments, the in-place clause
    after = hdr[hdr.index("EMEI_API int emei_plan_mppi("):]
    comment = after[:after.index("emei_plan_cem_workspace_bytes(")]
    for word in ("core.py:18-37,190-193", "n_elites", "elite_return_out", "sigma_map", "lower k", "NaN", "S2", "in place"):
        assert word in comment, word
    # the candidate specification carries the sigma_map clause
    spec = hdr[hdr.index("The candidates (normative)"):hdr.index("emei_sample_candidates writes them out")]
    assert "sigma_map[t, i, a]" in spec and "entry of 0" in spec
    history = hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    assert "emei_plan_cem" in history and "emei_sample_candidates_sigma" in history
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    for name in NAMES:
        assert name in _lib.SYMBOLS and name in exported and hasattr(lib, name), name
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def _buffers():
    return {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in ("ws", "mean", "std", "ret", "idx", "er", "nom", "smap", "out")}


def test_plan_cem_refusals_with_a_null_handle():
    lib = _lib.lib()
    b = _buffers()

    def call(horizon=4, k=8, m=2, discount=1.0, nominal=None, sigma=0.0, smap=None, ws=b["ws"], mean=b["mean"], std=b["std"],
             ret=b["ret"], idx=b["idx"], er=b["er"]):
        rc = lib.emei_plan_cem(None, horizon, k, m, 1234, nominal, sigma, smap, discount, None, ws, mean, std, ret, idx, er, None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith("emei_plan_cem") and "null handle" in msg, msg
    # the scalars are checked first: each refusal names its own argument
    for kw, word in (({"horizon": 0}, "horizon"), ({"horizon": -2}, "horizon"), ({"k": 0}, "n_candidates"), ({"k": -1}, "n_candidates"),
                     ({"m": 0}, "n_elites"), ({"m": -3}, "n_elites"), ({"m": 9}, "n_elites"), ({"k": 1, "m": 2}, "n_elites"),
                     ({"discount": 0.0}, "discount"), ({"discount": 1.0000001}, "discount"), ({"discount": -1.0}, "discount"),
                     ({"discount": float("nan")}, "discount"), ({"discount": float("inf")}, "discount")):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_plan_cem:") and word in msg, (kw, rc, msg)
    assert "null handle" in call(m=8)[1] and "null handle" in call(m=1)[1]  # n_elites = n_candidates and = 1 are legal
    # in the order of the list: horizon before n_candidates before n_elites before discount
    assert "horizon" in call(horizon=0, k=0, m=0, discount=0.0)[1]
    assert "n_candidates" in call(k=0, m=0, discount=0.0)[1]
    assert "n_elites" in call(m=0, discount=0.0)[1]
    # a bad scalar wins over the NULL handle and the NULL pointers; without one the handle is what is named
    assert "n_elites" in call(m=0, ws=None, mean=None)[1]
    assert "discount" in call(discount=0.0, ws=None, mean=None)[1]
    assert "null handle" in call(ws=None, mean=None)[1]
    # what needs the handle and the pointers: refused, with a message, nothing dereferenced
    for kw in ({"nominal": b["nom"], "sigma": 0.0}, {"nominal": b["nom"], "sigma": float("nan")}, {"smap": b["smap"]},
               {"nominal": b["nom"], "smap": b["smap"]}, {"k": 2**31 - 1}, {"ws": None}, {"mean": None}):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_plan_cem:"), (kw, rc, msg)
    with pytest.raises(ValueError, match="n_elites"):
        _lib.check(call(m=0)[0])


def test_sample_candidates_sigma_refusals_with_a_null_handle():
    lib = _lib.lib()
    b = _buffers()

    def call(horizon=4, k=8, nominal=b["nom"], smap=b["smap"], out=b["out"], dtype=3):  # EMEI_ACT_F32
        rc = lib.emei_sample_candidates_sigma(None, horizon, k, 1234, nominal, smap, out, dtype, None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith("emei_sample_candidates_sigma") and "null handle" in msg, msg
    for kw, word in (({"horizon": 0}, "horizon"), ({"k": 0}, "n_candidates")):  # emei_sample_candidates' scalar checks, first
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_sample_candidates_sigma:") and word in msg, (kw, rc, msg)
    for kw in ({"nominal": None}, {"smap": None}, {"out": None}):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith("emei_sample_candidates_sigma:"), (kw, rc, msg)


def test_workspace_bytes():
    f, g = _lib.lib().emei_plan_cem_workspace_bytes, _lib.lib().emei_plan_mppi_workspace_bytes
    ns, ks = (1, 3, 64, 65, 257, 4096, 100000), (1, 13, 63, 64, 65, 300, 4096)
    for a in range(len(ns)):
        for c in range(len(ks)):
            v = f(ns[a], ks[c])
            assert v >= g(ns[a], ks[c]) > 0  # at least MPPI's: its partials plus 8 bytes per candidate
            assert v % 8 == 0
            if a:
                assert v >= f(ns[a - 1], ks[c])
            if c:
                assert v >= f(ns[a], ks[c - 1])
    assert f(1, 2**31 - 1) >= g(1, 2**31 - 1) and f(2**31 - 1, 1) >= g(2**31 - 1, 1) > 0  # the largest shapes the plan call takes
    for bad in ((0, 4), (-1, 4), (4, 0), (4, -7), (2, 2**30), (2**31, 1), (2**40, 1), (2**16, 2**15)):
        assert g(*bad) == _lib.ERR_INVALID, bad  # negative where MPPI's size is
        assert f(*bad) == _lib.ERR_INVALID, bad
        assert b"emei_plan_cem_workspace_bytes" in _lib.lib().emei_last_error()
