"""The post-process at its structural edges (-m gpu): the constructed frames of tests/post_cases.py through csrc/postprocess.hip,
against the oracle, record for record and IN ORDER -- the cases are built so that the order is decidable (confidence ladder,
exact ties, binned confidences), so there is no set comparison and no allowance for unmatched records.

Which branch a case drives (the regimes are proved on the CPU by tests/test_post_cases_cpu.py):
    n=...           nw = ceil(n / 64), ntiles = nw (nw + 1) / 2 and the tile -> (c, w) decode; dummy rows / columns past n; the last
                    arriver's second candidate (tid + kTN) from 513; total <= kMaxDet against the overflow branch at 1025
    chain-...       the greedy scan: "a suppressed row suppresses nothing", groups of 16 in blocks of 64, lists keyed by class & 3
                    (960 rows in one list; classes 1 and 5 in one list), word_of
    pair-/special-  strict IoU > thr, strict confidence, class -1 through pack_ce / ce_class beside the dummies, NaN, +-inf
    cut-...         the histogram bin T, cnt against kMemCap, the `khi - klo` split loop (0 to 3 levels), esh / ebin, want = 1 .. cnt
Every case runs on the split form (post_decode_kernel + post_nms_kernel) and on the one-launch form (postprocess_kernel); cases
with at most 1024 candidates also through the seven step-wise gpu_postprocess.h symbols."""
import ctypes as C
import functools

import numpy as np
import pytest

import post_cases as pc

pytestmark = pytest.mark.gpu

FORMS = ("split", "one")
SIZES = {"s4": (96, 160, 4), "s8": (96, 160, 8), "l4": (640, 640, 4)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engines(pkg, sd7, torch_cuda):
    """(engine key, form) -> Engine, created on first use from the seed-7 synthetic weights (only the output tensors are used).
    The one-launch form is a second engine created with UNINA_POST_SPLIT=0 (read once, when the engine is loaded)."""
    from unina_yolo_dla_amd.engine import Engine
    made = {}

    def get(key, form):
        if (key, form) not in made:
            h, w, nc = SIZES[key]
            g = pkg.graph.Graph(num_classes=nc, in_h=h, in_w=w)
            sd = sd7 if nc == 4 else pkg.synth.make_state_dict(7, g)
            with pytest.MonkeyPatch.context() as mp:
                if form == "one":
                    mp.setenv("UNINA_POST_SPLIT", "0")
                made[key, form] = Engine.from_state_dict(sd, g)
        return made[key, form]

    yield get
    for e in made.values():
        e.close()


@functools.lru_cache(maxsize=None)
def case(name, key=None):
    """(heads, conf, iou, q, expect, oracle records, oracle candidate count): built and solved once, shared by every test"""
    from oracle import oracle
    grids, nc = pc.ENGINES[key or pc.engine_of(name)]
    heads, conf, iou, q, ex = pc.build(name, grids, nc)
    want, ncand = oracle.postprocess(heads, conf, iou, q)
    assert ncand == ex["total"]
    for h in heads:
        h.setflags(write=False)
    want.setflags(write=False)
    return heads, conf, iou, q, ex, want, ncand


def run_engine(pkg, torch, eng, heads, conf, iou, q):
    for n, h in zip(pkg.graph.OUTPUT_NAMES, heads):
        eng.outputs[n].copy_(torch.from_numpy(np.array(h))[None])
    return eng.postprocess(conf, iou, q)


def check(got, want, label=""):
    print(f"{label}: {len(got)} records (oracle {len(want)})"
          + (f", max |dconf| {np.abs(got['confidence'] - want['confidence']).max():.3g}" if len(got) == len(want) and len(got) else ""))
    assert len(got) == len(want), (len(got), len(want))
    for f in ("x1", "y1", "x2", "y2", "class_id"):
        assert np.array_equal(got[f], want[f]), (f, int(np.flatnonzero(got[f] != want[f])[0]))
    np.testing.assert_allclose(got["confidence"], want["confidence"], atol=2e-7, rtol=0)
    assert np.all(np.diff(got["confidence"]) <= 0)
    assert np.all(got["valid"] == 1) and np.all(got["_pad"] == 0)


def ids(names):
    return [f"{n}-{f}" for n in names for f in FORMS]


def params(names):
    return [(n, f) for n in names for f in FORMS]


@pytest.mark.parametrize("name,form", params(pc.COUNT_NAMES), ids=ids(pc.COUNT_NAMES))
def test_count_sweep(pkg, engines, torch_cuda, name, form):
    heads, conf, iou, q, ex, want, _ = case(name)
    check(run_engine(pkg, torch_cuda, engines(pc.engine_of(name), form), heads, conf, iou, q), want, name)


@pytest.mark.parametrize("name,form", params(pc.CHAIN_NAMES), ids=ids(pc.CHAIN_NAMES))
def test_chains(pkg, engines, torch_cuda, name, form):
    heads, conf, iou, q, ex, want, _ = case(name)
    assert len(want) == len(ex["kept_e"]) < ex["total"]
    check(run_engine(pkg, torch_cuda, engines(pc.engine_of(name), form), heads, conf, iou, q), want, name)


@pytest.mark.parametrize("name,form", params(pc.PAIR_NAMES), ids=ids(pc.PAIR_NAMES))
def test_pair_edges(pkg, engines, torch_cuda, name, form):
    heads, conf, iou, q, ex, want, _ = case(name)
    check(run_engine(pkg, torch_cuda, engines(pc.engine_of(name), form), heads, conf, iou, q), want, name)


@pytest.mark.parametrize("name,form", params(pc.CUT_NAMES), ids=ids(pc.CUT_NAMES))
def test_cut_regimes(pkg, engines, torch_cuda, name, form):
    heads, conf, iou, q, ex, want, ncand = case(name)
    assert ncand > pc.MAX_DET
    check(run_engine(pkg, torch_cuda, engines("l4", form), heads, conf, iou, q), want, name)


# exact ties scattered over all three levels and many launch-1 workgroups, one per way the cut can fall among them
TIED = ["cut-bin2048-cnt=1025-want=1-1key", "cut-bin2048-cnt=1025-want=1024-2keys", "cut-bin2048-cnt=5000-want=2-1key",
        "cut-bin0-all-2keys", "cut-bin1-2keys", "cut-bin4095-2keys-and-ones", "special-all_m200", "special-m200_bg_ladder",
        "special-inf"]


@pytest.mark.parametrize("name,form", params(TIED), ids=ids(TIED))
def test_scattered_ties_are_identical_run_to_run(pkg, engines, torch_cuda, name, form):
    """Launch 1 builds the candidate list in arrival order; every later decision rests on (confidence, enumeration index)
    alone, so five runs of a frame full of exact ties return the same bytes."""
    heads, conf, iou, q, ex, want, _ = case(name)
    assert ex.get("tied")
    eng = engines(pc.engine_of(name), form)
    runs = [run_engine(pkg, torch_cuda, eng, heads, conf, iou, q).tobytes() for _ in range(5)]
    assert all(r == runs[0] for r in runs[1:])
    check(np.frombuffer(runs[0], dtype=want.dtype), want, name)


@pytest.mark.parametrize("form", FORMS)
def test_sequence_of_wildly_different_counts_on_one_engine(pkg, engines, torch_cuda, form):
    """ws_rank, ws_rownz, ws_hist, ws_total and ticket2 are zero at rest: the last arriver resets them over the nw * 64 entries
    of ITS frame. 33 600 candidates, then 1, 0, 1025, 64, ... on one engine, every call against the oracle; then backwards."""
    eng = engines("l4", form)
    for name in pc.SEQUENCE + pc.SEQUENCE[::-1]:
        heads, conf, iou, q, ex, want, _ = case(name, "l4")
        check(run_engine(pkg, torch_cuda, eng, heads, conf, iou, q), want, f"sequence {name}")


@pytest.fixture(scope="module")
def stepwise(engines, torch_cuda):
    L = engines("s4", "split").L
    assert L.init_postprocess_resources() == 0
    yield L
    L.cleanup_postprocess_resources()


STEP_NAMES = [n for n in pc.COUNT_NAMES + pc.CHAIN_NAMES + pc.PAIR_NAMES
              if not any(n.startswith(f"n={k}-") for k in (1025, 1260)) and "m200" not in n]


@pytest.mark.parametrize("name", STEP_NAMES)
def test_stepwise_api(pkg, stepwise, torch_cuda, name):
    """reset_detection_counter, 3 x decode_yolo_head, get_detection_count, run_gpu_nms, copy_valid_detections_to_host
    (the call sequence of test_stepwise_reference_api) on every case of at most 1024 candidates. (Above 1024 that API caps by
    enumeration order, by design.)"""
    from unina_yolo_dla_amd.engine import DET_DTYPE
    L, torch = stepwise, torch_cuda
    heads, conf, iou, q, ex, want, ncand = case(name)
    assert ncand <= pc.MAX_DET
    dev = [torch.from_numpy(np.array(h)).cuda() for h in heads]
    dets = torch.zeros(1024 * 8, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert L.reset_detection_counter(stream) == 0
    for i, s in enumerate(pc.STRIDES):
        c, r = dev[2 * i], dev[2 * i + 1]
        assert L.decode_yolo_head(c.data_ptr(), r.data_ptr(), dets.data_ptr(), c.shape[2], c.shape[1], s, c.shape[0],
                                  conf, q, stream) == 0
    n = C.c_int(-1)
    assert L.get_detection_count(C.byref(n), stream) == 0
    torch.cuda.synchronize()
    assert n.value == ncand
    assert L.run_gpu_nms(dets.data_ptr(), n.value, iou, stream) == 0
    host = np.zeros(1024, dtype=DET_DTYPE)
    valid = C.c_int(-1)
    assert L.copy_valid_detections_to_host(dets.data_ptr(), host.ctypes.data, n.value, C.byref(valid), stream) == 0
    check(host[:valid.value], want, name)
