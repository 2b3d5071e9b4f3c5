"""csrc/locate.hip on the GPU through unina_locate_async: every comparison is BYTE equality of the MAX_DETECTIONS
unina_cone3d records with localize.locate_numpy (integers, and fp32 values with a fixed operation order: no tolerance). Maps are
97 x 61 on pitched planes (12 spare bytes per f32 row, 6 per u16 row, filled with garbage), plus one 600 x 600 map for the
windows that are strided on both axes or too large to stay on chip between the selection passes."""
import numpy as np
import pytest

import locate_cases as lc
from records import assert_records_equal, det_buffer

pytestmark = pytest.mark.gpu

SPARE = {0: 12, 1: 6}          # bytes behind each row: UNINA_DEPTH_F32, UNINA_DEPTH_U16


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import engine, localize
    return torch, engine, localize


@pytest.fixture(scope="module")
def locator(env):
    return env[2].DeviceLocator()


def pitched_plane(torch, depth, fmt):
    """[H, W] map -> uint8 CUDA tensor [H, pitch] whose spare bytes are 0xA5 (a NaN-free but wrong value in either format)."""
    h, w = depth.shape
    row = depth.dtype.itemsize * w
    host = np.full((h, row + SPARE[fmt]), 0xA5, dtype=np.uint8)
    host[:, :row] = np.ascontiguousarray(depth).view(np.uint8).reshape(h, row)
    return torch.from_numpy(host).cuda()


def run_device(env, locator, c, plane=None, buf=None):
    torch = env[0]
    plane = pitched_plane(torch, c["depth"], c["fmt"]) if plane is None else plane
    buf = det_buffer(torch, c["dets"], c["count"]) if buf is None else buf
    locator.out.fill_(0xFF)
    locator.update_from_buffer(buf, plane, c["unit"], c["cam"], c["params"], fmt=c["fmt"], width=c["depth"].shape[1])
    return locator.read()


def twin(env, c):
    return env[2].locate_numpy(c["dets"], c["count"], c["depth"], c["fmt"], c["unit"], c["cam"], c["params"])


def check(env, locator, c):
    got, want = run_device(env, locator, c), twin(env, c)
    assert_records_equal(got, want, c["name"])
    return got


@pytest.mark.parametrize("fmt", lc.FORMATS, ids=["f32", "u16"])
def test_edge_cases_equal_the_twin(env, locator, fmt):
    """Counts 0 / 1 / 1024 / 5000 (clamped) / negative; boxes outside, clipped at each edge, degenerate, inverted, non-finite;
    windows of 1, 63, 64, 65 samples, strided on one axis, 256 x 256 samples, 8192 and 8256 samples; all-hole maps; min_valid
    one above n_valid; even n_valid; all samples equal; samples differing in the lowest / the highest byte only; heavy ties."""
    seen = {}
    for c in lc.edge_cases(fmt):
        seen[c["name"]] = check(env, locator, c)
    # (what each case contains is asserted on the twin in tests/test_locate_cpu.py; here the ones whose point is the kernel's path)
    assert seen["count5000_clamped"]["n_samples"][1023] == 9 and not seen["count0"].view(np.uint8).any()
    assert seen["map600_256x256"]["n_samples"][0] == 65536 and seen["map600_256x256"]["valid"][0] == 1
    assert seen["map600_128x64_129x64"]["n_samples"][:2].tolist() == [8192, 8256]
    assert seen["even_n_valid"]["z"][0] == 5 and seen["min_valid_one_above"]["valid"][0] == 0


@pytest.mark.parametrize("fmt", lc.FORMATS, ids=["f32", "u16"])
def test_random_boxes_equal_the_twin(env, locator, fmt):
    c = lc.random_case(fmt, n=200)
    got = check(env, locator, c)
    v = got[:200]
    assert (v["valid"] == 1).sum() > 100 and (v["n_samples"] > 64).sum() >= 3 and (v["n_samples"] == 0).sum() > 3
    # the same boxes with the unstrided windows of max_side = 64: the large ones go through the LDS-resident path
    c = lc.case("random200_wide", fmt, c["dets"], c["depth"], shrink=1.0, max_side=64)
    got = check(env, locator, c)
    assert (got["n_samples"] > 1000).sum() >= 3


@pytest.mark.parametrize("fmt", lc.FORMATS, ids=["f32", "u16"])
def test_two_launches_give_identical_bytes(env, locator, fmt):
    torch = env[0]
    c = lc.case("repeat", fmt, lc.random_boxes(77, 300), lc.depth_map(78 + fmt, fmt), shrink=1.0, max_side=32)
    plane, buf = pitched_plane(torch, c["depth"], fmt), det_buffer(torch, c["dets"], c["count"])
    a = run_device(env, locator, c, plane, buf)          # the output buffer is filled with 0xFF before each launch
    b = run_device(env, locator, c, plane, buf)
    assert a.tobytes() == b.tobytes() == twin(env, c).tobytes()
    assert not a[300:].view(np.uint8).any()


def test_tensor_maps_and_other_streams(env, locator):
    """DeviceLocator.describe on typed tensors (a float32 map, an int16 view of a u16 map, a row-strided view), on a side stream."""
    torch = env[0]
    s = torch.cuda.Stream()
    for fmt in lc.FORMATS:
        c = lc.random_case(fmt, n=60, seed=31)
        wide = np.zeros((lc.H, lc.W + 5), dtype=c["depth"].dtype)
        wide[:, :lc.W] = c["depth"]
        t = torch.from_numpy(wide.view(np.int16) if fmt else wide).cuda()[:, :lc.W]      # a view: its row stride is the pitch
        buf = det_buffer(torch, c["dets"], c["count"])
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            locator.out.fill_(0xFF)
            locator.update_from_buffer(buf, t, c["unit"], c["cam"], c["params"], stream=s)
            got = locator.read(s)
        assert got.tobytes() == twin(env, c).tobytes()


def test_behind_a_letterboxed_frame_on_the_same_stream(env, locator, pkg, sd7):
    """The node's call order: infer_letterbox_frame (asynchronous, boxes in camera pixels) on a 96 x 72 BGRA frame, then
    unina_locate_async on the same stream with a 96 x 72 depth map; nothing between the two touches the host."""
    torch, engine, localize = env
    g = pkg.graph.Graph(in_h=64, in_w=64)
    eng = engine.Engine.from_state_dict(sd7, g, device=0)
    try:
        w, h = 96, 72
        rng = np.random.RandomState(5)
        d_bgra = torch.from_numpy(rng.randint(0, 256, (h, 4 * w)).astype(np.uint8)).cuda()
        frame = engine.Frame.from_tensors(engine.FMT_BGRA, w, h, d_bgra, 4 * w)
        depth = lc.depth_map(9, engine.DEPTH_F32, h, w)
        plane = pitched_plane(torch, depth, engine.DEPTH_F32)
        cam, par = (80.0, 80.0, 47.5, 35.5), lc.params(shrink=0.5, max_side=16)
        out = torch.full((lc.MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")
        locator.out.fill_(0xFF)
        eng.infer_letterbox_frame(frame, None, 0.05, 0.45, 0.1, 114.0, True, out=out)
        locator.update_from_buffer(out, plane, 1.0, cam, par, fmt=engine.DEPTH_F32, width=w)
        got = locator.read()
        dets = engine.Engine.unpack(out)
    finally:
        eng.close()
    assert len(dets) > 0
    want = localize.locate_numpy(dets, len(dets), depth, engine.DEPTH_F32, 1.0, cam, par)
    assert got.tobytes() == want.tobytes()
    assert (got["valid"][:len(dets)] == 1).sum() > 0
    print(f"{len(dets)} records, {(got['valid'] == 1).sum()} located")
