"""Camera calls carry what they need to the launch as a per-call description; the engine holds none of it. Two consequences, both
byte for byte on the 64 x 64 seed-7 FP16 engine with the cameras of tests/letterbox_child.py:

  * an engine without the frame graph (UNINA_FULL_GRAPH=0: the stem launched eagerly in front of the captured forward, the
    post-process behind it) returns what the default engine returns for plain, letterboxed and tiled calls of every format;
  * a call leaves nothing behind: tensor calls return the same records before and after camera calls, refused ones included.

Every compared list holds at least one record (the threshold comes from the CPU oracle: tests/test_camera_calls_cpu.py)."""
import os

import numpy as np
import pytest

from camera_call_cases import CASES, FORMATS, add_frames, call
from letterbox_child import CONF, IOU, NET, Q, device_camera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import camera as twin, engine
    return torch, engine, twin


def make_engine(env, pkg, sd7):
    return env[1].Engine.from_state_dict(sd7, pkg.graph.Graph(in_h=NET, in_w=NET))


@pytest.fixture(scope="module")
def eng(env, pkg, sd7):
    e = make_engine(env, pkg, sd7)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_eager(env, pkg, sd7):
    """UNINA_FULL_GRAPH is read at load: set around the construction of a second engine."""
    old = os.environ.get("UNINA_FULL_GRAPH")
    os.environ["UNINA_FULL_GRAPH"] = "0"
    try:
        e = make_engine(env, pkg, sd7)
    finally:
        if old is None:
            del os.environ["UNINA_FULL_GRAPH"]
        else:
            os.environ["UNINA_FULL_GRAPH"] = old
    yield e
    e.close()


@pytest.fixture(scope="module")
def cams(env):
    torch, engine, twin = env
    return {name: add_frames(torch, engine, twin, device_camera(torch, name)) for name in {n for _g, n in CASES}}


def both_ways(env, e, c, fmt, geometry, **kw):
    """(synchronous records, asynchronous records) of one call, as bytes."""
    torch, engine, _t = env
    sync = call(e, c, fmt, geometry, **kw)
    buf = torch.full((1024 * 8 + 8,), -1, dtype=torch.int32, device="cuda")
    assert call(e, c, fmt, geometry, out=buf, **kw) is buf
    torch.cuda.synchronize()
    return sync.tobytes(), engine.Engine.unpack(buf).tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("geometry,name", CASES)
def test_camera_calls_without_the_frame_graph(env, eng, eng_eager, cams, geometry, name, fmt):
    # the two engines do differ in the launch form: only the frame graph folds head output convs into the decode launch
    assert any(eng.folded_heads()) and not any(eng_eager.folded_heads())
    want, want_async = both_ways(env, eng, cams[name], fmt, geometry)
    assert len(want) >= 32 and want_async == want
    got, got_async = both_ways(env, eng_eager, cams[name], fmt, geometry)
    assert got == want
    assert got_async == want


def test_a_call_leaves_nothing_behind(env, pkg, sd7, eng, cams):
    torch, engine, _t = env
    c = cams["128x72_down"]
    images = torch.from_numpy(np.random.default_rng(93).standard_normal((1, 3, NET, NET)).astype(np.float32)).cuda()
    a = eng.infer(images, CONF, IOU, Q).tobytes()
    assert len(a) >= 32
    # a letterboxed call with the box map on: the next tensor call maps nothing and reads the tensor
    assert len(call(eng, c, "bgra", "letterbox", map_boxes=True)) >= 1
    assert eng.infer(None, CONF, IOU, Q).tobytes() == a
    # a synchronous tiled call (its completion word went to the merge): the next asynchronous call signals nothing and is whole
    assert len(call(eng, c, "nv12", "tiled")) >= 1
    buf = eng.infer_async(None, CONF, IOU, Q)
    torch.cuda.synchronize()
    assert engine.Engine.unpack(buf).tobytes() == a
    # a refused call (pitch too small for the width)
    with pytest.raises(engine.EngineError, match=r"unina_infer_letterbox_bgra: \S"):
        eng.infer_letterbox_bgra(c["d_bgra"], c["w"], c["h"], 4 * c["w"] - 4, None, CONF, IOU, Q)
    assert eng.infer(None, CONF, IOU, Q).tobytes() == a
    # ... and an unmapped letterboxed call after all of these is the first call of a fresh engine
    got = call(eng, c, "nv12", "letterbox", map_boxes=False).tobytes()
    fresh = make_engine(env, pkg, sd7)
    try:
        want = call(fresh, c, "nv12", "letterbox", map_boxes=False).tobytes()
    finally:
        fresh.close()
    assert len(want) >= 32 and got == want
