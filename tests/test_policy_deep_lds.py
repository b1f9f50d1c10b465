"""The LDS budget of the deep policy kernels, from the metadata of the shipped gfx950 code objects (no GPU, no instructions read).
Every deep kernel is launched as a ONE-WAVE block whose dynamic LDS is the wave's h1 tile, 256 bytes per unit of the first hidden
layer (emei_device.h:policy_deep_tile_bytes): at EMEI_POLICY_DEEP_MAX_HIDDEN the tile and the kernel's static LDS together must fit
the 160 KiB a gfx950 CU has, or the launch at widths of 256 fails on the GPU.  The static part must also be a multiple of 16 bytes:
the dynamic region follows it unpadded and the tile is read and written 16 bytes per lane."""
import os
import re
import shutil
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "emei_amd", "libemei_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
WAVES_PER_BLOCK = 1  # pendulum_kernels.h / body_kernels.h: dim3(kWave) at every deep launch
DEEP = ("pend_policy_rollout_deep_kernel", "body_policy_rollout_deep_kernel", "pend_policy_eval_deep_kernel", "body_policy_eval_deep_kernel")


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


def test_every_deep_kernel_is_there(kernels):
    count = {k: sum(k in name for name in kernels) for k in DEEP}
    # 16 translation units of the 4-state family, one Env each; 24 of the bodies, each with the RK4 and the Euler instantiation
    assert count["pend_policy_rollout_deep_kernel"] == 16 and count["pend_policy_eval_deep_kernel"] == 16, count
    assert count["body_policy_rollout_deep_kernel"] == 48 and count["body_policy_eval_deep_kernel"] == 48, count


def test_the_tile_fits_beside_the_static_lds_at_the_cap(kernels):
    tile = 256 * _lib.POLICY_DEEP_MAX_HIDDEN
    assert tile == 64 * 1024
    checked = 0
    for name, g in kernels.items():
        if not any(k in name for k in DEEP):
            continue
        static = int(g["group_segment_fixed_size"])
        assert static + WAVES_PER_BLOCK * tile <= 160 * 1024, (name, static)
        assert static % 16 == 0, (name, static)  # the tile starts where the static arrays end
        assert int(g["max_flat_workgroup_size"]) == 64 * WAVES_PER_BLOCK, (name, g["max_flat_workgroup_size"])
        assert int(g["vgpr_count"]) <= 512, (name, g["vgpr_count"])
        checked += 1
    assert checked == 128
