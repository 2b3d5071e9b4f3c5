"""The stand-alone stride-2 3x3 convs in front of the two-bottleneck blocks (backbone.stage2_conv, backbone.stage3_conv) under
every stride-2 register-queue configuration, bit for bit against the im2col kernel (conv_glds, configuration 0) on the same
buffers, fp16 and int8. The stride-2 tiles keep an LDS image of their own (csrc/regq_s2.h: even patch columns in front of the odd
ones); the frame sizes put one tile larger than the image (32x32), partial tiles on both edges with odd tile counts (48x80) and
several full tiles (96x160), so the image border falls on even and on odd patch rows and columns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPS = ("backbone.stage2_conv", "backbone.stage3_conv")
SIZES = ((32, 32), (48, 80), (96, 160))
WANT = {"backbone.stage2_conv": 2, "backbone.stage3_conv": 3}      # stride-2 rows of the table for Cin 64 and for Cin 128


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", ["fp16", "int8"])
def test_stride2_regq_configurations_equal_conv_glds(pkg, sd7, torch_cuda, precision, size):
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine, calibrate_amax
    g = pkg.graph.Graph(in_h=size[0], in_w=size[1])
    if precision == "int8":
        amax = calibrate_amax(sd7, g, [pkg.rng.frame(5000 + i, *size) for i in range(2)])
        e = Engine.from_state_dict(sd7, g, precision=export.INT8, amax=amax)
    else:
        e = Engine.from_state_dict(sd7, g)
    try:
        assert e.set_fusion(False) == 0
        xd = torch_cuda.from_numpy(pkg.rng.frame(1234, *size)).cuda()
        infos = e.op_infos()
        names = e.conv_configs()
        assert names[0].startswith("conv_glds")
        index = {n: [i for i, o in enumerate(infos) if o["kind"] == 1 and o["name"] == n] for n in OPS}
        for n in OPS:
            assert len(index[n]) == 1, (n, [o["name"] for o in infos])
            assert e.set_op_config(index[n][0], 0)
        e.forward(xd)
        want = {n: e.read_buffer(n).copy() for n in OPS}
        assert all(np.isfinite(v).all() and v.any() for v in want.values())
        tried = {n: 0 for n in OPS}
        for cfg, cname in enumerate(names):
            if not (cname.startswith("conv3x3_regq") and cname.endswith("s2>")):
                continue
            applied = [n for n in OPS if e.set_op_config(index[n][0], cfg)]
            if not applied:
                continue
            e.forward(xd)
            for n in applied:
                got = e.read_buffer(n)
                diff = int((got != want[n]).sum())
                print(f"stage s2 conv: {precision} {size[0]}x{size[1]} {n} {cname}: {got.size} elements, {diff} differ from conv_glds")
                assert diff == 0, (n, cname, diff)
                tried[n] += 1
                assert e.set_op_config(index[n][0], 0)
        assert all(tried[n] >= WANT[n] for n in OPS), tried
    finally:
        e.close()
