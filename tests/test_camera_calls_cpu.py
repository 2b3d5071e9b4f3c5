"""Camera calls, host side only: what Engine's nine camera methods hand to the C ABI, and that the cases of
tests/test_gpu_camera_calls.py cannot compare empty detection lists."""
import ctypes as C

import pytest

from camera_call_cases import CASES, FORMATS, TILES, reference_tensors
from letterbox_child import CONF, IOU, NET, Q, host_camera

# The parameters of each symbol as include/unina_mi355.h declares them (the `_async` form of a symbol has the same list, d_out and
# d_out_count in the place of out and out_count).
HEADER = {
    "unina_infer_bgra": "e d_bgra width height pitch norm conf iou q out count stream",
    "unina_infer_nv12": "e d_y d_uv width height y_pitch uv_pitch norm conf iou q out count stream",
    "unina_infer_letterbox_bgra": "e d_bgra width height pitch norm conf iou q pad_value map_boxes out count stream",
    "unina_infer_letterbox_nv12": "e d_y d_uv width height y_pitch uv_pitch norm conf iou q pad_value map_boxes out count stream",
    "unina_infer_tiled_bgra": "e d_bgra width height pitch tiles n_tiles norm conf iou q merge_iou out count stream",
    "unina_infer_tiled_nv12": "e d_y d_uv width height y_pitch uv_pitch tiles n_tiles norm conf iou q merge_iou out count stream",
    "unina_infer_frame": "e frame norm conf iou q out count stream",
    "unina_infer_letterbox_frame": "e frame norm conf iou q pad_value map_boxes out count stream",
    "unina_infer_tiled_frame": "e frame tiles n_tiles norm conf iou q merge_iou out count stream",
}
ASYNC = [s for s in HEADER if s not in ("unina_infer_bgra", "unina_infer_nv12")]   # (these two have no asynchronous form)


class Tensor:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


class Recorder:
    """Stands in for the loaded library: every symbol records its name and arguments and returns UNINA_OK."""

    def __init__(self, engine_mod):
        self.calls = []
        self.default_norm = engine_mod.NormParams()

    def create_norm_params_imagenet(self):
        return self.default_norm

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


@pytest.fixture()
def stub(pkg):
    from unina_yolo_dla_amd import engine

    class Stub(engine.Engine):
        def __init__(self):
            self.L = Recorder(engine)
            self.h = C.c_void_p(0x5150)
            self.width = self.height = NET

        def close(self):
            pass

    return engine, Stub()


@pytest.mark.parametrize("default_norm", (False, True))
@pytest.mark.parametrize("symbol,is_async", [(s, False) for s in HEADER] + [(s, True) for s in ASYNC])
def test_each_method_calls_its_own_symbol_in_the_header_order(stub, symbol, is_async, default_norm):
    engine, e = stub
    plane, y, uv, out = Tensor(0x1000), Tensor(0x2000), Tensor(0x3000), Tensor(0x8000)
    frame = engine.Frame.from_tensors(4, 128, 72, 0x4000, 256)
    norm = None if default_norm else engine.NormParams()
    v = dict(width=101, height=102, pitch=103, y_pitch=104, uv_pitch=105, conf=0.11, iou=0.22, q=0.33, pad_value=44.0, merge_iou=0.55,
             stream=777)
    planes = dict(bgra=(plane,), nv12=(y, uv), frame=(frame,))[symbol.rsplit("_", 1)[1]]
    size = () if planes == (frame,) else (v["width"], v["height"]) + ((v["pitch"],) if planes == (plane,) else (v["y_pitch"], v["uv_pitch"]))
    thr = (v["conf"], v["iou"], v["q"])
    kw = dict(stream=v["stream"], **(dict(out=out) if is_async else {}))
    method = getattr(e, symbol[len("unina_"):])
    if "_letterbox_" in symbol:
        got = method(*planes, *size, norm, *thr, v["pad_value"], True, **kw)
    elif "_tiled_" in symbol:
        got = method(*planes, *size, TILES, norm, *thr, v["merge_iou"], **kw)
    else:
        got = method(*planes, *size, norm, *thr, **kw)
    (name, args), = e.L.calls
    assert name == symbol + ("_async" if is_async else "")
    want = HEADER[symbol].split()
    assert len(args) == len(want), (args, want)
    for a, p in zip(args, want):
        if p == "e":
            assert a is e.h
        elif p in ("d_bgra", "d_y", "d_uv"):
            assert a == dict(d_bgra=plane, d_y=y, d_uv=uv)[p].address
        elif p == "frame":
            assert a._obj is frame
        elif p == "norm":
            assert a._obj is (e.L.default_norm if default_norm else norm)
        elif p == "tiles":
            assert [(t.x, t.y, t.w, t.h) for t in a] == [tuple(t) for t in TILES]
        elif p == "n_tiles":
            assert a == len(TILES)
        elif p == "map_boxes":
            assert a == 1 and type(a) is int
        elif p == "out":
            assert a == out.address + 32 if is_async else isinstance(a, int) and a != 0
        elif p == "count":
            assert a == out.address if is_async else isinstance(a._obj, C.c_int)
        else:
            assert a == v[p], p
    if is_async:
        assert got is out
    else:
        assert got.dtype == engine.DET_DTYPE and len(got) == 0      # (the stub wrote no count)


@pytest.mark.parametrize("geometry,name", CASES)
def test_the_oracle_alone_keeps_a_record_in_every_case(pkg, oracle_mod, oracle_sd7, geometry, name):
    """The threshold of the GPU comparisons comes from the CPU oracle (tests/letterbox_child.py at CONF): on every tensor the
    network sees in test_gpu_camera_calls.py -- every tile of a tiled call too -- oracle.forward + oracle.postprocess keep at least
    one record whose confidence lies 0.03 above the threshold: ten times what an fp16 engine's scores differ from the oracle's by
    (~3e-3), so the engine keeps that record too."""
    from unina_yolo_dla_amd import camera as twin
    c = host_camera(name)
    for fmt in FORMATS:
        for x in reference_tensors(twin, c, fmt, geometry):
            assert x.shape == (3, NET, NET)
            heads = oracle_mod.forward(oracle_sd7, x)
            dets, _n = oracle_mod.postprocess([heads[n] for n in pkg.graph.OUTPUT_NAMES], CONF, IOU, Q)
            print(geometry, name, fmt, len(dets), float(dets["confidence"].max()) if len(dets) else None)
            assert len(dets) >= 1 and dets["confidence"].max() >= CONF + 0.03, (geometry, name, fmt, len(dets))
