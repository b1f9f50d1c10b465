"""The InvertedDoublePendulum's fused controllers on the host: the two kernel ids are declared (additive under ABI 8) and bound with
names, and the header says which handles emei_mpc_mppi / emei_mpc_cem serve.  The refusal order and the workspace sizes of the two
calls are unchanged (tests/test_mpc_api.py, tests/test_mpc_cem_api.py)."""
import os
import re

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "emei_hip.h")).read()


def test_kernel_ids_are_declared_and_bound():
    assert re.search(r"EMEI_KERNEL_BODY_MPC_MPPI\s*=\s*13\b", HDR) and re.search(r"EMEI_KERNEL_BODY_MPC_CEM\s*=\s*14\b", HDR)
    assert _lib.KERNEL_BODY_MPC_MPPI == 13 and _lib.KERNEL_BODY_MPC_CEM == 14
    assert _lib.KERNEL_NAMES[13] == "body_mpc_mppi_kernel" and _lib.KERNEL_NAMES[14] == "body_mpc_cem_kernel"
    assert sorted(_lib.KERNEL_NAMES) == list(range(15))  # the enum has no holes
    # the earlier ids keep their values
    assert re.search(r"EMEI_KERNEL_PEND_MPC_MPPI\s*=\s*11\b", HDR) and re.search(r"EMEI_KERNEL_PEND_MPC_CEM\s*=\s*12\b", HDR)


def test_the_abi_version_stays():
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", HDR) and _lib.ABI_VERSION == 8
    assert _lib.lib().emei_abi_version() == 8


def test_the_header_names_the_inverted_double_pendulum():
    history = HDR[HDR.index("ABI history"):HDR.index("#define EMEI_ABI_VERSION")]
    assert "InvertedDoublePendulum" in history and "EMEI_KERNEL_BODY_MPC_MPPI" in history and "EMEI_KERNEL_BODY_MPC_CEM" in history
    after = HDR[HDR.index("EMEI_API int emei_plan_cem("):]
    mppi = after[:after.index("EMEI_API int64_t emei_mpc_mppi_workspace_bytes(")]
    after = HDR[HDR.index("EMEI_API int emei_mpc_mppi("):]
    cem = after[:after.index("EMEI_API int64_t emei_mpc_cem_workspace_bytes(")]
    for comment in (mppi, cem):
        assert "InvertedDoublePendulum" in comment and "six floats" in comment and "observation noise" in comment
        assert "EMEI_ERR_UNSUPPORTED" in comment
