"""The P3 / P4 head path of the frame AS LAUNCHED, held to float64 and to bytes.

tests/test_gpu_per_op.py holds every op to its rounding bound with fusion OFF, and test_frame_as_launched_equals_per_op_table
carries that bound over to the fused block kernels and the P2 head by bit-identity. It does not carry over to the P3 / P4
heads: with fusion on their 3x3 layers run as dual launches (conv_dual_head3x3_ws and its _i8 / _s16 / _small forms; plan_duals
returns early with fusion off, and a forced tile configuration takes an op out of its pair), and unina_infer computes their 1x1
output convs inside post_decode_kernel. same_head allows those launches 5e-3 on a logit. Here:
  1. the launched frame's own buffers against float64, op by op, for every op whose slices all reach memory in that frame;
  2. the pair kernels against the single configurations whose bodies they instantiate: bytes;
  3. both at the smallest frame that selects the half-height pair;
  4. the folded decode with every cell observed (conf_thr 0, iou_thr 1: nothing is dropped, nothing suppressed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emulate as E
import launched_heads_child as LH

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "launched_heads_child.py")
IDS = LH.IDS


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _child(args, env, timeout):
    r = subprocess.run([sys.executable, CHILD, *args], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    sys.stdout.write("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("per-op bound")))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


# ---- 1. the launched frame against float64, teacher-forced on its own buffers ----
@pytest.mark.parametrize("size", LH.SIZES, ids=IDS)
@pytest.mark.parametrize("precision", ["fp16", "strict", "int8"])
def test_launched_frame_within_the_bound(pkg, sd7, torch_cuda, tmp_path, precision, size):
    """One forward with fusion on; every op whose source, shortcut and destination slices the frame writes (emulate.launched_ops,
    from op_infos()) against its float64 evaluation on the frame's own buffers, bound of check_slice. The four 3x3 head layers
    must run as the weights-stationary pair (not its stamped twin), all six head ops of P3 and of P4 must be among the checked
    ops, and every checked slice must change with the frame (it is written, not left over). At 80x112 the fused groups the
    engine reports are those of launched_heads_child.GROUPS_A, which the CPU test works from."""
    LH.hold_launched_frame(pkg, sd7, torch_cuda, tmp_path, precision, size, LH.DUAL[precision][0], check_groups=size == (80, 112))


@pytest.mark.parametrize("precision", ["fp16", "strict", "int8"])
def test_launched_frame_within_the_bound_register_queue_pairs(precision):
    """UNINA_DUAL_WS=0 (read once per process: a child of its own, with its own time limit): the same check with the head layers
    on the register-queue pairs conv_dual_head3x3 / _i8 / _s16, every size."""
    _child(["bound", precision, *map(IDS, LH.SIZES)], {"UNINA_DUAL_WS": "0"}, timeout=240)


# ---- 2. exact twin ----
@pytest.mark.parametrize("size", LH.SIZES, ids=IDS)
@pytest.mark.parametrize("precision", ["fp16", "int8"])
def test_pair_kernels_equal_their_single_configurations(pkg, sd7, torch_cuda, tmp_path, precision, size):
    """Fusion off, the four 3x3 head ops forced to the single configurations whose bodies the pair kernel instantiates; then the
    frame as launched. The hidden buffers behind layer 0 and layer 1 and the four P3 / P4 planes: the same bytes.
    Not STRICT in this form: with fusion off a STRICT engine's 3x3 convs INSIDE the C3k2 blocks run on the chunked
    weights-stationary kernels (conv_plan takes them first for kS16; conv3x3_wsc_body sums chunk-major: chunk, ky, kx, cb) while
    the block kernels sum (ky, kx, cb), so p3_out / p4_out -- the heads' INPUTS -- already differ in their last bits between the two
    runs (measured: every one of the eight buffers and both inputs differ; test_frame_as_launched_equals_per_op_table allows that
    2e-5). That is the blocks' order, not the pair's: the next test gives both runs the same inputs and holds STRICT to bytes."""
    same = LH.exact_twin(pkg, sd7, torch_cuda, tmp_path, precision, size)
    print(f"exact twin: {precision} {IDS(size)}: {same}")
    assert all(same.values()), same


@pytest.mark.parametrize("size", LH.SIZES, ids=IDS)
@pytest.mark.parametrize("precision", ["fp16", "strict", "int8"])
def test_pair_kernels_equal_their_single_configurations_behind_the_block_kernels(pkg, sd7, torch_cuda, tmp_path, precision, size):
    """The same with fusion on in both runs (a forced configuration alone takes an op out of its pair): the heads read the block
    kernels' p3_out / p4_out both times, so the only difference between the runs is the pair launch itself. All three precisions."""
    same = LH.exact_twin(pkg, sd7, torch_cuda, tmp_path, precision, size, fused_upstream=True)
    print(f"exact twin behind the block kernels: {precision} {IDS(size)}: {same}")
    assert all(same.values()), same


# ---- 3. the half-height pair ----
def test_half_height_pair_at_the_smallest_frame_that_selects_it(pkg, sd7, torch_cuda, tmp_path):
    """conv_dual_match takes conv_dual_head3x3_ws_small when the grids of the full-height pair together exceed 256 workgroups.
    conv_grid gives ceil(Ho / th) * ceil(Wo / tw) M tiles times sum(ceil(n_pad / 64)) N tiles: for P3 (Ho, Wo) = (H / 8, W / 8),
    16 x 16 tiles and two slices of 128 channels, 4 * ceil(H / 128) * ceil(W / 128); for P4 (H / 16, W / 16), 8 x 16 tiles and two
    slices of 256, 8 * ceil(H / 128) * ceil(W / 256). A wide frame of the smallest legal height, 16, needs 4 * ceil(W / 128) +
    8 * ceil(W / 256) > 256: W = 4112 (132 + 136). A TALL frame of the smallest legal width, 16, needs 12 * ceil(H / 128) > 256:
    22 tile rows, H = 2704 (88 + 176 = 264; H = 2688 gives 252) -- fewer pixels, because P4's tiles are 8 rows high but 16 columns
    wide. Maps of 676 x 4, 338 x 2 and 169 x 1: every float64 evaluation stays small. Sections 1 and 2 there, fp16."""
    h, w, ga, gb = LH.smallest_half_height_size()
    assert (h, w, ga, gb) == (2704, 16, 88, 176)
    prefix = LH.DUAL["fp16-small"][0]
    LH.hold_launched_frame(pkg, sd7, torch_cuda, tmp_path, "fp16", (h, w), prefix)
    same = LH.exact_twin(pkg, sd7, torch_cuda, tmp_path, "fp16", (h, w), key="fp16-small")
    print(f"exact twin: fp16 {h}x{w} half-height pair: {same}")
    assert all(same.values()), same


# ---- 4. the folded decode, every cell observed ----
def _per_op_heads(pkg, sd7, torch, tmp_path, precision, size):
    """The per-op planes: every op of the head path a launch of its own, the four 3x3 head ops on the configurations of the
    pair's bodies (section 2: the launched frame's bytes; the heuristic's im2col kernels sum in another order, same_head).
    fp16: fusion off, the whole per-op table. STRICT: fusion stays on for the C3k2 blocks, whose per-op form sums in another order
    than the block kernels (section 2) -- the heads' ops, P2's included, are single launches there all the same (no split-fp16 head
    kernel, a forced configuration unpairs, forward() folds nothing)."""
    from test_gpu_per_op import _make
    b, e, _ = _make(pkg, sd7, pkg.graph.Graph(in_h=size[0], in_w=size[1]), precision, tmp_path)
    try:
        if precision == "strict":
            assert e.set_fusion(True) > 0
        else:
            assert e.set_fusion(False) == 0
        LH.force_twins(e, b, LH.DUAL[precision][1])
        infos = e.op_infos()
        for oi in (oi for lv in E.head_ops(b, ("p2", "p3", "p4")).values() for oi in lv):
            if precision == "strict" or "p2" not in b.ops[oi].name:
                assert not infos[oi]["kernel"].startswith(("(", "conv_dual", "head")), (b.ops[oi].name, infos[oi]["kernel"])
        return {k: v.copy() for k, v in e.forward(torch.from_numpy(pkg.rng.frame(1234, *size)).cuda()).items()}
    finally:
        e.close()


@pytest.mark.parametrize("precision", ["fp16", "strict"])
def test_folded_decode_every_cell(pkg, sd7, oracle_mod, torch_cuda, tmp_path, precision):
    """infer(x, conf_thr 0, iou_thr 1, q) through the full-frame graph with the P3 / P4 output convs folded into the decode launch
    (STRICT: P2's too, its head is not a fused launch), against the oracle's post-process of the per-op planes: as many records
    as cells (21, 63, 735 <= MAX_DETECTIONS), boxes and classes bit for bit, confidences within 2e-7 (GPU expf against glibc's).
    Every cell's arg-max logit and its four regression values are thereby observed, the tail subtiles' cells (pix clamped to
    ncell - 1) included, for heads read from planes (256 cells per workgroup) and folded ones (64). Then UNINA_POST_FOLD=0 in a
    child: the same bytes. fp16: the fold issues the MFMAs of conv_glds in its order. STRICT: both sides are mfma_split (lo*hi,
    hi*lo, hi*hi into one accumulator) per k block in ascending order from zero, then acc + bias -- the split fold reproduces the
    per-op S16 output conv bit for bit as well, so bytes are asserted for both."""
    from test_gpu_class_counts import check_same_records
    from unina_yolo_dla_amd.engine import MAX_DETECTIONS
    got = LH.decode_records(pkg, sd7, torch_cuda, precision, LH.DECODE_SIZES)
    for size in LH.DECODE_SIZES:
        folded = [bool(v) for v in got[f"{IDS(size)}_folded"]]
        assert folded == [precision == "strict", True, True], (size, folded)          # not folded is a failure, not a skip
        heads = _per_op_heads(pkg, sd7, torch_cuda, tmp_path, precision, size)
        ncell = LH.n_cells(size)
        assert ncell <= MAX_DETECTIONS
        for q in LH.DECODE_QS:
            want, ncand = oracle_mod.postprocess([heads[n] for n in pkg.graph.OUTPUT_NAMES], 0.0, 1.0, q)
            assert len(want) == ncand == ncell, (size, q, len(want), ncand, ncell)
            check_same_records(got[f"{IDS(size)}_{q}"], want, 4, ordered=False)
    out = str(tmp_path / "unfolded.npz")
    _child(["decode", precision, out, *map(IDS, LH.DECODE_SIZES)], {"UNINA_POST_FOLD": "0"}, timeout=240)
    plain = np.load(out)
    for size in LH.DECODE_SIZES:
        assert not plain[f"{IDS(size)}_folded"].any()
        for q in LH.DECODE_QS:
            assert plain[f"{IDS(size)}_{q}"].tobytes() == got[f"{IDS(size)}_{q}"].tobytes(), (size, q)
