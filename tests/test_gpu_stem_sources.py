"""Camera frames in the stem at partial tiles and on non-square networks (the cases of tests/stem_source_cases.py; what they are
and why the thresholds keep a record on every compared tensor: tests/test_stem_sources_cpu.py). For every case, in the three stem
instantiations (FP16, FP32, STRICT) and, for the tap and letterbox cases, in INT8:

  * the stem buffer a camera call leaves, against a float64 evaluation of the stem on the numpy twin's tensor, element by element
    under the bound of DESIGN.md 6.4 (emulate.per_op_bounds / check_per_op: no failing element, worst error / bound <= 1.0) -- a
    reference that is no GPU kernel. A tiled call is run once per tile with that tile last (the stem buffer holds the last tile);
  * the in-stem call against the two-step form: unina_preprocess_frame / _letterbox_frame into a NaN-filled tensor equals the twin
    byte for byte, and unina_infer on it leaves the same bytes in EVERY buffer (fusion off: all are written; the head planes a
    frame graph folds into its decode launch stay NaN in both and are not counted) and returns the same records, synchronous and
    asynchronous; letterboxed records with map_boxes = 1 equal camera.unmap_boxes of them; a tiled call equals twin tensor per tile
    -> unina_infer_async -> slicing.map_records -> the oracle's sort + NMS, and slicing.merge_numpy;
  * the stem op is stem_tile_kernel in these engines; a third of the cases once more through stem_conv_kernel (UNINA_STEM_V1=1, one
    fresh child: tests/stem_sources_child.py);
  * one engine, many sources in a row -- with and without the frame graph -- against a fresh engine per call;
  * the 64-channel stem (Graph(base_channels=64) at 32 x 80): buffers only, its seed-7 weights keep no record at any sensible
    threshold (stem_source_cases.B64_SIZE).

Every destination is filled with NaN (tensors) or -1 (record buffers) before the call that writes it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emulate as E
import stem_source_cases as S
from frame_child import NAMES, NV12
from nv12_child import ROOT
from test_tiled_cpu import oracle_sort_nms

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp16", "fp32", "strict")
KERNEL_TYPE = {"fp16": "f16", "fp32": "f32", "strict": "s16"}
# (INT8: the tap and letterbox cases)
RUNS = [(p, s, g) for p in PRECISIONS for s in S.SIZES for g in S.GEOMETRIES] + \
       [("int8", s, g) for s in S.SIZES for g in ("tap", "letterbox")]
RUN_IDS = [f"{p}-{S.SIZE_ID(s)}-{g}" for p, s, g in RUNS]


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import camera as twin, engine, export, slicing
    return torch, engine, twin, slicing, export


@pytest.fixture(scope="module")
def engines(env, pkg, sd7, tmp_path_factory):
    """get(size, precision, base_channels=32) -> (builder, engine loaded from the file the builder wrote): built on first use,
    shared by every test of this module."""
    torch, engine, twin, slicing, export = env
    made = {}
    d = tmp_path_factory.mktemp("stem_sources")

    def get(size, precision, base_channels=32):
        key = (size, precision, base_channels)
        if key not in made:
            g = pkg.graph.Graph(base_channels=base_channels, in_h=size[0], in_w=size[1])
            sd = sd7 if base_channels == 32 else pkg.synth.make_state_dict(7, g)
            amax = None
            if precision == "int8":
                amax = engine.calibrate_amax(sd, g, [pkg.rng.frame(5000 + i, *size) for i in range(2)])
            p = {"fp16": export.FP16, "fp32": export.FP32, "strict": export.STRICT, "int8": export.INT8}[precision]
            b = export.EngineBuilder(sd, g, p, amax)
            path = str(d / f"{S.SIZE_ID(size)}_{precision}_{base_channels}.une")
            b.save(path)
            made[key] = (b, engine.Engine(path))
        return made[key]

    yield get
    for _b, e in made.values():
        e.close()


@pytest.fixture(scope="module")
def frames(env):
    """get(case) -> the case's frame on the device (frame_child.make_frame) with f["x"] = its reference tensors; made once."""
    torch, engine, twin, _s, _x = env
    made = {}

    def get(c):
        if c not in made:
            f = S.device_frame(torch, engine, twin, c)
            want = S.planes(twin, c)                                  # the bytes the CPU tests chose the thresholds on
            for a, b in zip(f["planes"] if c.fmt == NV12 else [f["planes"]], want if c.fmt == NV12 else [want]):
                assert np.array_equal(a, b), S.case_id(c)
            f["x"] = S.reference_tensors(twin, c, f["planes"])
            made[c] = f
        return made[c]

    return get


def stem_index(env, b):
    (i,) = [i for i, op in enumerate(b.ops) if op.kind == env[4].OP_STEM]
    return i


def assert_tiled_stem(env, b, e, precision, co=32):
    kernel = e.op_infos()[stem_index(env, b)]["kernel"]
    if precision == "int8":                                           # (whichever type the stem's destination has there)
        assert kernel.startswith("stem_tile_kernel<") and kernel.endswith(f",{co}>"), kernel
    else:
        assert kernel == f"stem_tile_kernel<{KERNEL_TYPE[precision]},{co}>", kernel


def nan_heads(e):
    for t in e.outputs.values():
        t.fill_(float("nan"))


_nan_images = {}


def bind_nan_images(torch, e, size):
    """The engine's `images` tensor is all NaN during a camera call: a stem that read it would show."""
    if size not in _nan_images:
        _nan_images[size] = torch.full((1, 3) + tuple(size), float("nan"), dtype=torch.float32, device="cuda")
    e.bind_images(_nan_images[size])


def hold_stem(env, b, x, teacher):
    """(failures, worst error / bound) of the stem op's output in `teacher` against float64 on the tensor x [3, H, W]."""
    recs = E.per_op_bounds(b, x[None], teacher, only_op=[stem_index(env, b)])
    assert len(recs) == 1 and recs[0]["buf"] == "backbone.stem"
    fails, worst, _ties = E.check_per_op(recs, teacher)
    return fails, worst


def record_buffer(torch):
    return torch.full((S.MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")


def rotations(tiles):
    """[(tile list with tile k last, k)]: the stem buffer holds the last tile of a tiled call."""
    return [(tuple(tiles[k + 1:]) + tuple(tiles[:k + 1]), k) for k in range(len(tiles))]


# ------------------------------------------------------------------------------------ 1. against float64

def check_against_float64(env, b, e, frames, cases, label):
    torch = env[0]
    assert e.set_fusion(False) == 0
    n = 0
    worst_cam = 0.0
    for c in cases:
        f = frames(c)
        for tiles, t in (rotations(c.tiles) if c.geometry == "tiled" else [(None, 0)]):
            bind_nan_images(torch, e, c.size)
            S.call(e, c, f, tiles=tiles)
            teacher = E.engine_buffers(b, e.read_buffer)
            fails, worst = hold_stem(env, b, f["x"][t], teacher)
            which = f" tile {t} {c.tiles[t]} last" if tiles else ""
            print(f"stem sources: {label} {S.case_id(c)}{which}: worst error/bound {worst:.3f}")
            assert not fails, (S.case_id(c), which, fails[:4])
            assert worst <= 1.0, (S.case_id(c), which, worst)
            worst_cam = max(worst_cam, worst)
            n += 1
    return n, worst_cam


@pytest.mark.parametrize("precision,size,geometry", RUNS, ids=RUN_IDS)
def test_stem_from_camera_bytes_within_the_float64_bound(env, pkg, engines, frames, precision, size, geometry):
    torch = env[0]
    b, e = engines(size, precision)
    assert_tiled_stem(env, b, e, precision)
    label = f"{precision} {S.SIZE_ID(size)}"
    n, worst_cam = check_against_float64(env, b, e, frames, S.cases(size, geometry), label)
    assert n == len(S.cases(size, geometry)) * (3 if geometry == "tiled" else 1)
    x = pkg.rng.frame(1234, *size)                                  # the same engine's stem fed from a tensor (tests/test_gpu_per_op.py)
    e.forward(torch.from_numpy(x).cuda())
    fails, worst_tensor = hold_stem(env, b, x[0], E.engine_buffers(b, e.read_buffer))
    assert not fails and worst_tensor <= 1.0
    print(f"stem sources: {label} {geometry}: {n} launches, worst error/bound of the stem op from camera bytes {worst_cam:.3f}, "
          f"from the tensor rng.frame(1234) {worst_tensor:.3f}")


# ------------------------------------------------------------------------------------ 2. against the two-step form

def two_step_tensor(env, c, f, t=0):
    """unina_preprocess_frame / _letterbox_frame of the case (tile t) into a NaN-filled tensor: equals the twin byte for byte."""
    torch, engine = env[0], env[1]
    images = torch.full((1, 3) + c.size, float("nan"), dtype=torch.float32, device="cuda")
    if c.geometry == "letterbox":
        engine.preprocess_letterbox_frame(f["frame"], images, S.PAD)
    else:
        engine.preprocess_frame(f["frame"], images, region=c.tiles[t] if c.geometry == "tiled" else None)
    torch.cuda.synchronize()
    assert images.cpu().numpy()[0].tobytes() == f["x"][t].tobytes(), (S.case_id(c), t)
    return images


def same_buffers(b, e, got, want, what):
    """Every buffer byte for byte (NaN-safe); the stem and every head plane the frame's decode launch does not compute itself are
    really written."""
    assert set(got) == set(want)
    for n in want:
        assert got[n].tobytes() == want[n].tobytes(), (what, n)
    assert np.isfinite(want["backbone.stem"]).all() and want["backbone.stem"].any()
    for h, folded in enumerate(e.folded_heads()):
        for n in (f"p{2 + h}_cls", f"p{2 + h}_reg"):
            assert folded or np.isfinite(want[n]).all(), (what, n)


def both_ways(env, e, c, f, **kw):
    """(synchronous records, asynchronous records) of the case's call, as bytes."""
    torch, engine = env[0], env[1]
    sync = S.call(e, c, f, **kw)
    buf = record_buffer(torch)
    assert S.call(e, c, f, out=buf, **kw) is buf
    torch.cuda.synchronize()
    return sync.tobytes(), engine.Engine.unpack(buf).tobytes()


def check_whole_frame(env, b, e, c, f, fusion, lists=True):
    """fusion off: every buffer is written and compared; on: the frame as launched by default."""
    torch, engine, twin = env[:3]
    H, W = c.size
    conf = S.CONF[c.size]
    images = two_step_tensor(env, c, f)
    read = (lambda: E.engine_buffers(b, e.read_buffer)) if not fusion else (lambda: {"backbone.stem": e.read_buffer("backbone.stem")})
    nan_heads(e)
    want = e.infer(images, conf, S.IOU, S.Q)
    want_bufs = read()
    nan_heads(e)
    bind_nan_images(torch, e, c.size)
    got = S.call(e, c, f)                                           # (a letterboxed call: map_boxes = 0)
    got_bufs = read()
    if fusion:
        assert got_bufs["backbone.stem"].tobytes() == want_bufs["backbone.stem"].tobytes(), S.case_id(c)
    else:
        same_buffers(b, e, got_bufs, want_bufs, S.case_id(c))
    assert not lists or len(want) >= 1, S.case_id(c)
    assert got.tobytes() == want.tobytes(), (S.case_id(c), fusion)
    sync, asyn = both_ways(env, e, c, f)
    assert sync == want.tobytes() and asyn == want.tobytes(), (S.case_id(c), fusion)
    if c.geometry == "letterbox":
        mapped = twin.unmap_boxes(want, c.w, c.h, W, H).tobytes()
        sync, asyn = both_ways(env, e, c, f, map_boxes=True)
        assert sync == mapped and asyn == mapped, (S.case_id(c), fusion)
        assert mapped != want.tobytes()
    return len(want)


def check_tiled(env, oracle_mod, b, e, c, f, fusion):
    torch, engine, twin, slicing, _x = env
    H, W = c.size
    conf = S.CONF[c.size]
    tiles = list(c.tiles)
    slots = np.zeros((len(tiles), S.MAXD), dtype=slicing.DET_DTYPE)
    counts = []
    for t, x in enumerate(f["x"]):
        two_step_tensor(env, c, f, t)
        buf = record_buffer(torch)
        nan_heads(e)
        e.infer_async(torch.from_numpy(x[None]).cuda(), conf, S.IOU, S.Q, out=buf)
        torch.cuda.synchronize()
        d = engine.Engine.unpack(buf)
        slots[t, :len(d)] = d
        counts.append(len(d))
    want_bufs = E.engine_buffers(b, e.read_buffer) if not fusion else None      # (of the last tile's tensor)
    union = slicing.map_records(slots, counts, tiles, net_w=W, net_h=H)
    want = oracle_sort_nms(oracle_mod, union, S.MERGE)
    assert slicing.merge_numpy(slots, counts, tiles, S.MERGE, net_w=W, net_h=H).tobytes() == want.tobytes()
    print(f"stem sources: {S.case_id(c)} fusion {int(fusion)}: per-tile counts {counts}, merged {len(want)}")
    # on the engine's own counts: at least two tiles contribute and the merge suppresses a record -- the map matters
    assert max(counts) <= S.MAXD and sum(n > 0 for n in counts) >= 2 and 1 <= len(want) < sum(counts), (counts, len(want))
    nan_heads(e)
    bind_nan_images(torch, e, c.size)
    got = S.call(e, c, f)
    assert got.tobytes() == want.tobytes(), (S.case_id(c), fusion)
    if not fusion:
        same_buffers(b, e, E.engine_buffers(b, e.read_buffer), want_bufs, S.case_id(c))
    sync, asyn = both_ways(env, e, c, f)
    assert sync == want.tobytes() and asyn == want.tobytes(), (S.case_id(c), fusion)
    return len(want)


@pytest.mark.parametrize("precision,size,geometry", RUNS, ids=RUN_IDS)
def test_in_stem_call_equals_the_two_step_form(env, oracle_mod, engines, frames, precision, size, geometry):
    b, e = engines(size, precision)
    assert_tiled_stem(env, b, e, precision)
    kept = []
    for fusion in (False, True):
        e.set_fusion(fusion)
        for c in S.cases(size, geometry):
            f = frames(c)
            if geometry == "tiled":
                kept.append(check_tiled(env, oracle_mod, b, e, c, f, fusion))
            else:
                kept.append(check_whole_frame(env, b, e, c, f, fusion))
    print(f"stem sources: {precision} {S.SIZE_ID(size)} {geometry}: {len(kept) // 2} cases, records kept {min(kept)}..{max(kept)}")


# ------------------------------------------------------------------------------------ 3. the one-thread-per-pixel stem

def test_one_thread_per_pixel_stem_gives_the_same_bytes(env, engines, frames, tmp_path):
    """UNINA_STEM_V1=1 is read once per process: one fresh child runs stem_source_cases.child_cases() through stem_conv_kernel on
    FP16 engines; the parent's default (tiled) run must give the same records and the same stem buffer."""
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stem_sources_child.py"), out], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, UNINA_STEM_V1="1"))
    assert r.returncode == 0 and "STEM_SOURCES_CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(out, allow_pickle=False)
    for size in S.SIZES:
        assert str(got["kernel_" + S.SIZE_ID(size)]) == "stem_conv_kernel<f16,32>"
        b, e = engines(size, "fp16")
        assert_tiled_stem(env, b, e, "fp16")
        e.set_fusion(True)
    for k, c in enumerate(S.child_cases()):
        b, e = engines(c.size, "fp16")
        want = S.call(e, c, frames(c))
        assert len(want) >= 1 and got[f"det{k}"].tobytes() == want.tobytes(), S.case_id(c)
        assert np.array_equal(got[f"stem{k}"], e.read_buffer("backbone.stem")), S.case_id(c)


# ------------------------------------------------------------------------------------ 4. one engine, many sources

@pytest.mark.parametrize("frame_graph", [True, False], ids=["frame_graph", "no_frame_graph"])
def test_one_engine_many_sources(env, pkg, sd7, frames, frame_graph):
    """On one 96 x 160 FP16 engine, in this order: tensor, NV12 tap, Bayer resize, YUYV letterbox with the box map, BGRA tiled,
    a refused frame (pitch too small), tensor. Each result is what a fresh engine returns for that call alone; the two tensor
    results are equal bytes. Once with the frame graph, once with UNINA_FULL_GRAPH=0 (read at load: set around construction)."""
    torch, engine, twin = env[:3]
    size = S.SEQUENCE_SIZE
    conf = S.CONF[size]
    seq = S.sequence_cases()
    assert [(c.geometry, NAMES[c.fmt]) for c in seq] == [("tap", "nv12"), ("resize", "rggb"), ("letterbox", "yuyv"), ("tiled", "bgra")]
    bytes_case = [c for c in S.cases(size, "tap", (NV12,)) if c.camera == "bytes"][0]
    images = torch.from_numpy(frames(bytes_case)["x"][0][None]).cuda()       # (a tensor the CPU oracle keeps records on)

    def make():
        old = os.environ.get("UNINA_FULL_GRAPH")
        if not frame_graph:
            os.environ["UNINA_FULL_GRAPH"] = "0"
        try:
            return engine.Engine.from_state_dict(sd7, pkg.graph.Graph(in_h=size[0], in_w=size[1]))
        finally:
            if not frame_graph:
                if old is None:
                    del os.environ["UNINA_FULL_GRAPH"]
                else:
                    os.environ["UNINA_FULL_GRAPH"] = old

    def run(e, step):
        if step is None:
            return e.infer(images, conf, S.IOU, S.Q).tobytes()
        return S.call(e, step, frames(step), map_boxes=step.geometry == "letterbox").tobytes()

    alone = []
    for step in [None] + seq:
        fresh = make()
        try:
            alone.append(run(fresh, step))
        finally:
            fresh.close()
    assert all(len(a) >= 32 for a in alone) and len(set(alone)) == len(alone)
    e = make()
    try:
        assert frame_graph or not any(e.folded_heads())
        got = [run(e, step) for step in [None] + seq]
        f = frames(seq[0])
        bad = engine.Frame.from_tensors(NV12, f["w"], f["h"], f["d"], f["w"] - 1, f["d_uv"], f["uv_pitch"])
        with pytest.raises(engine.EngineError, match=r"unina_infer_frame: \S"):
            e.infer_frame(bad, None, conf, S.IOU, S.Q)
        last = run(e, None)
    finally:
        e.close()
    for k, (g, a) in enumerate(zip(got, alone)):
        assert g == a, ("call", k)
    assert last == got[0]


# ------------------------------------------------------------------------------------ 5. the 64-channel stem

@pytest.mark.parametrize("precision", PRECISIONS)
def test_64_channel_stem_from_camera_frames(env, engines, frames, precision):
    """stem_tile_kernel<., 64>: the tap and resize cameras of one 4:2:2 and one Bayer format at 32 x 80, against float64 and
    against the two-step form. Buffers and whatever records there are; no list is required to hold one."""
    b, e = engines(S.B64_SIZE, precision, base_channels=64)
    assert_tiled_stem(env, b, e, precision, co=64)
    cases = S.b64_cases()
    assert len(cases) == 2 * 2 * 2
    n, worst = check_against_float64(env, b, e, frames, cases, f"{precision} base64 {S.SIZE_ID(S.B64_SIZE)}")
    print(f"stem sources: {precision} base64 {S.SIZE_ID(S.B64_SIZE)}: {n} launches, worst error/bound of the stem op from camera bytes {worst:.3f}")
    for fusion in (False, True):
        e.set_fusion(fusion)
        for c in cases:
            check_whole_frame(env, b, e, c, frames(c), fusion, lists=False)
