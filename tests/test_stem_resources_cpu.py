"""The stem kernels' registers, as the build compiles them: csrc/stem_pool.hip cross-compiled for gfx950 (device code only, the
flags of build.py) with -Rpass-analysis=kernel-resource-usage. Every instantiation must keep the occupancy it had before the frame
descriptor's formats were added and use no scratch: stem_tile_kernel<*,32> sits at 126 / 128 VGPRs, right below the step from 4 to 3
waves per SIMD, and stem_conv_kernel keeps its 6 / 5 waves only with the layout its comments describe. A compiler that allocates
differently fails here, not silently on the GPU. No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# waves per SIMD of (kernel, output channels) in the parent of the frame descriptor
OCCUPANCY = {("stem_tile_kernel", 32): 4, ("stem_tile_kernel", 64): 2, ("stem_conv_kernel", 32): 6, ("stem_conv_kernel", 64): 5}


@pytest.fixture(scope="module")
def usage(pkg, tmp_path_factory):
    from unina_yolo_dla_amd import build
    d = tmp_path_factory.mktemp("stem_resources")
    cmd = [build.hipcc(), *build.COMMON, *build.UNITS["stem_pool.hip"], "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(build.CSRC, "stem_pool.hip"), "-o", str(d / "stem_pool.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def test_every_stem_instantiation_keeps_its_occupancy_and_uses_no_scratch(usage):
    seen = 0
    for name, u in usage.items():
        m = re.search(r"(stem_tile_kernel|stem_conv_kernel)I.*Li(32|64)E", name)
        if not m:
            continue
        seen += 1
        want = OCCUPANCY[(m.group(1), int(m.group(2)))]
        print(name, u)
        assert u["Occupancy [waves/SIMD]"] >= want, (name, u)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (name, u)
    assert seen == 12                                                       # f16, f32, s16 x 32, 64 channels x two kernels
