"""The LDS budget of the deep policy PLAN kernels (emei_plan_policy_deep), from the metadata of the shipped gfx950 code objects (no
GPU, no instructions read), as test_policy_deep_lds.py reads it for the other deep kernels.  Both are launched as ONE-WAVE blocks
whose dynamic LDS is the wave's h1 tile, sized by the wider first layer of the policy and the value network: at
EMEI_POLICY_DEEP_MAX_HIDDEN the 64 KiB tile and the kernel's static LDS (the trig table, the body's solver scratch at stride 64)
together must fit the 160 KiB a gfx950 CU has.  The static part must be a multiple of 16 bytes: the tile follows it unpadded and is
read and written 16 bytes per lane."""
import os
import re
import shutil
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "emei_amd", "libemei_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
PLAN_DEEP = ("pend_policy_plan_deep_kernel", "body_policy_plan_deep_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: its metadata entry} over every gfx950 code object bundled in the library"""
    d = tmp_path_factory.mktemp("notes")
    lib = shutil.copy(LIB, d)
    subprocess.check_call([OBJDUMP, "--offloading", lib], stdout=subprocess.DEVNULL, cwd=d)
    readelf = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
    seen = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f:
            continue
        txt = subprocess.check_output([readelf, "--notes", os.path.join(d, f)], text=True)
        for blk in txt.split("- .agpr_count:")[1:]:
            g = dict(re.findall(r"\.(\w+):\s+(\S+)", ".agpr_count:" + blk))
            if "name" in g:
                seen[g["name"]] = g
    return seen


def test_every_plan_deep_kernel_is_there(kernels):
    count = {k: sum(k in name for name in kernels) for k in PLAN_DEEP}
    # 16 translation units of the 4-state family, one Env each; 24 of the bodies, each with the RK4 and the Euler instantiation
    assert count == {"pend_policy_plan_deep_kernel": 16, "body_policy_plan_deep_kernel": 48}, count


def test_the_tile_fits_beside_the_static_lds_at_the_cap(kernels):
    tile = 256 * _lib.POLICY_DEEP_MAX_HIDDEN
    assert tile == 64 * 1024
    checked = 0
    for name, g in kernels.items():
        if not any(k in name for k in PLAN_DEEP):
            continue
        static = int(g["group_segment_fixed_size"])
        assert static + tile <= 160 * 1024, (name, static)
        assert static % 16 == 0, (name, static)  # the tile starts where the static arrays end
        assert int(g["max_flat_workgroup_size"]) == 64, (name, g["max_flat_workgroup_size"])
        assert int(g["vgpr_count"]) <= 512, (name, g["vgpr_count"])
        checked += 1
    assert checked == 64
