"""emei_evaluate_sequences (ABI 8) on the host: declared, exported and bound; its scalar arguments are refused before any HIP
call (no GPU needed); and the prototype is C (tests/host/plan_abi.c compiles and links with gcc -std=c99 -Werror)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "emei_amd")
SRC = os.path.join(ROOT, "tests", "host", "plan_abi.c")


def test_header_declares_it_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    assert re.search(r"EMEI_API\s+int\s+emei_evaluate_sequences\s*\(", hdr)
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)
    assert _lib.ABI_VERSION == 8
    assert "emei_evaluate_sequences" in _lib.SYMBOLS
    lib = _lib.lib()
    assert lib.emei_abi_version() == 8
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert any(l.split()[-1] == "emei_evaluate_sequences" and " T " in l for l in nm.splitlines())


def test_bad_arguments_are_refused_before_touching_a_device():
    """Each case with a null handle: the scalar arguments are checked first, so every refusal names its own argument."""
    lib = _lib.lib()
    acts = (C.c_uint8 * 8)()
    ret = (C.c_double * 4)()
    ln = (C.c_int32 * 4)()

    def call(h=None, horizon=2, k=2, discount=1.0):
        rc = lib.emei_evaluate_sequences(h, horizon, k, C.cast(acts, C.c_void_p), _lib.ACT_U8, discount, None,
                                         C.cast(ret, C.c_void_p), C.cast(ln, C.c_void_p), None, None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and "null handle" in msg, msg
    for kw, word in (({"horizon": 0}, "horizon"), ({"horizon": -3}, "horizon"), ({"k": 0}, "n_candidates"),
                     ({"discount": 0.0}, "discount"), ({"discount": 1.5}, "discount"), ({"discount": -0.5}, "discount"),
                     ({"discount": float("nan")}, "discount")):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and word in msg, (kw, rc, msg)
    with pytest.raises(ValueError, match="discount"):
        _lib.check(call(discount=1.5)[0])


def test_c_program_calling_the_prototype_compiles_and_links(tmp_path):
    if not os.path.exists(os.path.join(LIBDIR, "libemei_hip.so")):
        pytest.skip("libemei_hip.so not built")
    exe = str(tmp_path / "plan_abi")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
           "-I", "/opt/rocm/include", SRC, "-o", exe, "-L", LIBDIR, "-lemei_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    assert os.path.exists(exe)
