"""The block kernels' prologue (c3k2_fused_body, conv_pair_kernel, head_fused_body; csrc/block_kernels.h, conv_pair.hip) requests
the input patch, the per-channel constants and then the weight queue, and waits with a COUNTED s_waitcnt for the first two only
(csrc/request_schedule.h): the weights stay in flight across the barrier. Nothing in the arithmetic moves, so

  * every block output of the fused frame equals the per-op table bit for bit (fp16, int8), and stays inside the STRICT mode's
    fused-vs-per-op bound (tests/test_gpu_strict.py) -- three frames per size, at the smallest sizes with edge tiles;
  * a wrong count would show as a RACE (a step reading a patch or constants that have not landed): 200 replays of three frames
    on one handle, and two handles alternating on two streams, must give each frame's first bytes every time (the criterion of
    tools/soak.py at test size).

(The tile form of the P2 head, head_fused_body, runs only under UNINA_HEAD_ALT=0: tests/test_gpu_pipeline.py compares it with the
default row-streaming head byte for byte in child processes.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = 3
REPLAYS = 200

# a down-sampling conv fused into its PAN block keeps its output in LDS, and the SPPF's pooled maps are formed in LDS by the pair
# kernel: those channels of the concat buffers are not written by the fused frame (tests/test_gpu_parity.py WRITTEN_WHEN_FUSED)
WRITTEN_WHEN_FUSED = {"neck.cat_pan1": (64, None), "neck.cat_pan2": (128, None), "backbone.sppf.cat": (0, 128)}
FP16_BUFFERS = ("neck.cat_fpn2", "neck.cat_fpn1", "neck.cat_pan2", "neck.cat_pan1", "p2_fused", "p3_out", "p4_out", "backbone.sppf.cat")
INT8_BUFFERS = ("neck.cat_fpn1", "neck.cat_pan1", "neck.cat_pan2", "p3_out", "p4_out", "backbone.sppf.cat", "neck.cat_fpn2", "p2_fused",
                "p2_fused.q8")
STRICT_BUFFERS = ("p2_fused", "p3_out", "p4_out", "backbone.sppf", "neck.cat_fpn1", "neck.cat_fpn2")


def written(bname, arr):
    a, b = WRITTEN_WHEN_FUSED.get(bname, (0, None))
    return arr[a:b]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def frames(pkg, torch, size):
    return [torch.from_numpy(pkg.rng.frame(1234 + i, size, size)).cuda() for i in range(FRAMES)]


def make_engine(pkg, sd7, precision, size, path=None):
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine, calibrate_amax
    g = pkg.graph.Graph(in_h=size, in_w=size)
    if precision == "int8":
        amax = calibrate_amax(sd7, g, [pkg.rng.frame(5000 + i, size, size) for i in range(2)])
        return Engine.from_state_dict(sd7, g, path=path, precision=export.INT8, amax=amax)
    if precision == "strict":
        return Engine.from_state_dict(sd7, g, path=path, precision=export.STRICT)
    return Engine.from_state_dict(sd7, g, path=path)


def assert_block_kernels_ran(e, precision):
    """The kernels whose prologue this file is about are in the frame as launched."""
    kernels = [o["kernel"] for o in e.op_infos()]
    tag = {"fp16": "", "int8": "i8", "strict": "s16"}[precision]
    blocks = [k for k in kernels if "c3k2_fused<" in k or k.startswith("block_dual")]
    pairs = [k for k in kernels if k.startswith("conv_pair<")]
    assert len(blocks) >= 5 and len(pairs) == 1, kernels
    if tag:
        assert any(("c3k2_fused<" + tag) in k or ("c3k2" + tag) in k for k in blocks), kernels
        assert ("conv_pair<" + tag) in pairs[0], kernels
    return kernels


@pytest.mark.parametrize("precision,size", [("fp16", 64), ("fp16", 96), ("int8", 96), ("int8", 128)])
def test_fused_frame_equals_the_per_op_table_bit_for_bit(pkg, sd7, torch_cuda, precision, size):
    e = make_engine(pkg, sd7, precision, size)
    try:
        assert e.L.unina_fusion_groups(e.h) == 9
        kernels = assert_block_kernels_ran(e, precision)
        if precision == "fp16":
            assert sum("head_fused" in k or "block_dual" in k for k in kernels) == 1, kernels     # the P2 head as one launch
        names = FP16_BUFFERS if precision == "fp16" else INT8_BUFFERS
        for x in frames(pkg, torch_cuda, size):
            assert e.set_fusion(True) == 9
            fused = {k: v.copy() for k, v in e.forward(x).items()}
            fbuf = {b: e.read_buffer(b) for b in names}
            assert e.set_fusion(False) == 0
            plain = e.forward(x)
            for b in names:
                assert np.array_equal(written(b, fbuf[b]), written(b, e.read_buffer(b))), b
            for k in plain:
                if precision == "int8" or k.startswith("p2_"):
                    assert np.array_equal(fused[k], plain[k]), k
                else:   # fp16 P3 / P4 heads: the fused frame runs them on the chunk-major pair kernel (test_gpu_parity.py same_head)
                    np.testing.assert_allclose(fused[k], plain[k], atol=5e-3, rtol=0, err_msg=k)
    finally:
        e.close()


@pytest.mark.parametrize("size", [64, 96])
def test_strict_fused_frame_stays_inside_the_per_op_bound(pkg, sd7, torch_cuda, size, tmp_path):
    e = make_engine(pkg, sd7, "strict", size, path=str(tmp_path / "s.une"))
    try:
        assert e.set_fusion(True) >= 8
        assert_block_kernels_ran(e, "strict")
        for x in frames(pkg, torch_cuda, size):
            e.set_fusion(True)
            fused = {k: v.copy() for k, v in e.forward(x).items()}
            fbuf = {b: e.read_buffer(b) for b in STRICT_BUFFERS}
            e.set_fusion(False)
            plain = e.forward(x)
            for name in pkg.graph.OUTPUT_NAMES:      # the bounds of test_strict_fused_equals_per_op_within_fp32_noise
                np.testing.assert_allclose(fused[name], plain[name], atol=5e-5, rtol=0, err_msg=name)
            for b in STRICT_BUFFERS:
                want = e.read_buffer(b)
                np.testing.assert_allclose(fbuf[b], want, atol=2e-5 * max(1.0, float(np.abs(want).max())), rtol=0, err_msg=b)
    finally:
        e.close()


def head_bytes(torch, e):
    """All six head tensors of the handle's last enqueue, as one device tensor."""
    return torch.cat([e.outputs[n].reshape(-1) for n in sorted(e.outputs)]).clone()


@pytest.mark.parametrize("precision,size", [("fp16", 64), ("fp16", 96), ("int8", 96), ("int8", 128), ("strict", 64), ("strict", 96)])
def test_replays_give_the_same_bytes(pkg, sd7, torch_cuda, precision, size, tmp_path):
    """One handle replaying, then two handles on two streams alternating: a prologue that let a step start before its patch or
    constants had landed would give different bytes now and then."""
    from unina_yolo_dla_amd.engine import Engine
    torch = torch_cuda
    path = str(tmp_path / "e.une")
    e1 = make_engine(pkg, sd7, precision, size, path=path)
    e2 = Engine(path)
    try:
        assert_block_kernels_ran(e1, precision)
        xs = frames(pkg, torch, size)
        ref = []
        for x in xs:
            e1.bind_images(x)
            e1.enqueue()
            torch.cuda.synchronize()
            ref.append(head_bytes(torch, e1))
        assert not torch.equal(ref[0], ref[1])                      # (the frames differ, so a stale result would show)
        bad = 0
        for i in range(REPLAYS * FRAMES):
            e1.bind_images(xs[i % FRAMES])
            e1.enqueue()
            torch.cuda.synchronize()
            bad += not torch.equal(head_bytes(torch, e1).view(torch.int32), ref[i % FRAMES].view(torch.int32))
        assert bad == 0, f"{bad} of {REPLAYS * FRAMES} replays differ from their frame's first result"
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for i in range(REPLAYS * FRAMES):
            a, b = i % FRAMES, (i + 1) % FRAMES
            e1.bind_images(xs[a])
            e2.bind_images(xs[b])
            e1.enqueue(s1)
            e2.enqueue(s2)
            torch.cuda.synchronize()
            bad += not torch.equal(head_bytes(torch, e1).view(torch.int32), ref[a].view(torch.int32))
            bad += not torch.equal(head_bytes(torch, e2).view(torch.int32), ref[b].view(torch.int32))
        assert bad == 0, f"{bad} of {2 * REPLAYS * FRAMES} two-stream results differ from their frame's first result"
    finally:
        e2.close()
        e1.close()

