"""csrc/stereo.hip on the GPU through unina_locate_stereo_async: every comparison is BYTE equality of the MAX_DETECTIONS
unina_cone3d and the MAX_DETECTIONS unina_stereo_match records with localize.locate_stereo_numpy (integer costs, and fp32 values
with a fixed operation order: no tolerance). Both output buffers are filled with 0xFF before each launch. The planes are pitched
with garbage spare bytes (the small pairs at a pitch of 103, the wide one at 1307: both odd) and start 0, 1 or 3 bytes into their
allocations. What each constructed case contains is asserted on the twin in tests/test_stereo_cpu.py."""
import numpy as np
import pytest

import stereo_cases as sc
from records import assert_records_equal, det_buffer

pytestmark = pytest.mark.gpu

OFFSETS = ((0, 0), (1, 3), (3, 1), (0, 1))     # bytes in front of the left / the right plane


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import engine, localize
    return torch, engine, localize


@pytest.fixture(scope="module")
def locator(env):
    return env[2].DeviceStereoLocator()


def pitched_plane(torch, img, offset, spare=6):
    """[H, W] bytes -> a [H, W] view (row stride W + spare) that starts `offset` bytes into a CUDA allocation; every byte that is
    not the image's is garbage that changes from byte to byte."""
    h, w = img.shape
    pitch = w + spare
    host = (np.arange(offset + h * pitch, dtype=np.uint32) * 37 + 11).astype(np.uint8)
    rows = host[offset:].reshape(h, pitch)
    rows[:, :w] = img
    dev = torch.from_numpy(host).cuda()
    return dev[offset:].view(h, pitch)[:, :w]


def planes(torch, c, k=0):
    spare = 6 if c["left"].shape[1] % 2 else 7
    return pitched_plane(torch, c["left"], OFFSETS[k % 4][0], spare), pitched_plane(torch, c["right"], OFFSETS[k % 4][1], spare)


def run_device(env, locator, c, k=0, pair=None, buf=None, match=True):
    torch = env[0]
    left, right = planes(torch, c, k) if pair is None else pair
    buf = det_buffer(torch, c["dets"], c["count"]) if buf is None else buf
    locator.out.fill_(0xFF)
    locator.match.fill_(0xFF)
    locator.update_from_buffer(buf, left, right, c["cam"], c["baseline"], c["params"], match=match)
    return locator.read()


def twin(env, c):
    return env[2].locate_stereo_numpy(c["dets"], c["count"], c["left"], c["right"], c["cam"], c["baseline"], c["params"])


def assert_equal(got, want, name):
    for g, w, what in zip(got, want, ("cone", "match")):
        assert_records_equal(g, w, name, what)


def check(env, locator, c, k=0):
    got = run_device(env, locator, c, k)
    assert_equal(got, twin(env, c), c["name"])
    return got


def test_constructed_cases_equal_the_twin(env, locator):
    """Every case the CPU tests pin (integer and fractional shifts, the rejections, every boundary) and the cases whose point is
    the kernel's path: nd of 1, 2, 3, 63, 64, 65, 256, 257 and 1024; n_samples of 1, 63, 64, 65 and 4096; strides on one axis and on
    both; a 64-row strip that stays on chip and one that is read through L2; the maximal cost with the last index. The base
    addresses move through offsets of 0, 1 and 3 bytes from case to case."""
    seen = {}
    for k, c in enumerate(sc.all_cases()):
        seen[c["name"]] = check(env, locator, c, k)
    cones, m = seen["nd_small"]
    assert cones["n_valid"][:6].tolist() == [1, 2, 3, 63, 64, 65] and (cones["valid"][:6] == 1).all()
    cones, m = seen["nd_wide"]
    assert cones["n_valid"][:5].tolist() == [256, 257, 1024, 1024, 1024] and cones["n_samples"][4] == 4096
    assert m["d_best"][:5].tolist() == [5, 5, 1000, 5, 1000] and (cones["valid"][:5] == 1).all()
    assert seen["n_samples"][0]["n_samples"][:5].tolist() == [1, 63, 64, 65, 434]
    assert seen["samples4096"][0]["n_samples"][:3].tolist() == [4096] * 3 and seen["samples4096"][1]["d_best"][:2].tolist() == [1000, 300]
    assert seen["stride_one_axis"][0]["n_samples"][:2].tolist() == [8 * 8, 7 * 7] and (seen["stride_one_axis"][0]["valid"][:2] == 1).all()
    assert seen["stride_both_axes"][0]["n_samples"][0] == 8 * 7
    cones, m = seen["stride2_wide"]                       # 64 x (126 + 1024) = 73 600 bytes of strip: past the 68 KB kept on chip
    assert cones["n_samples"][:3].tolist() == [4096, 4096, 64 * 34] and cones["n_valid"][:3].tolist() == [1024, 600, 1024]
    assert m["d_best"][:3].tolist() == [1000, 300, 1000] and (cones["valid"][:3] == 1).all()
    assert seen["max_cost_dent1"][1][0].tolist() == (1024.0, 1024, 4096 * 255 - 1, 4096 * 255)
    assert seen["max_cost_dent0"][1][0].tolist() == (0.0, 1, 4096 * 255, 4096 * 255)


def test_counts(env, locator):
    """Counts 0, 1, 1024, 5000 (clamped) and negative: the slots at and beyond the count are zero bytes in both outputs."""
    left, right = sc.integer_scene()
    grid = [sc.cell(3 * (i % 32), i // 32, 3, 3) for i in range(sc.MAXD)]          # 3 x 3 windows, all on the pair
    got = {}
    for k, (name, n_boxes, count) in enumerate((("count0", 8, 0), ("count1", 8, 1), ("count1024", 1024, 1024), ("count5000", 1024, 5000),
                                                ("count_negative", 8, -3))):
        got[name] = check(env, locator, sc.case(name, sc.boxes(grid[:n_boxes]), left, right, count=count), k)
    for name in ("count0", "count_negative"):
        assert not got[name][0].view(np.uint8).any() and not got[name][1].view(np.uint8).any()
    assert got["count1"][0]["n_samples"][:2].tolist() == [9, 0] and not got["count1"][1][1:].view(np.uint8).any()
    assert (got["count5000"][0]["n_samples"] == 9).all() and got["count5000"][0].tobytes() == got["count1024"][0].tobytes()
    assert (got["count1024"][0]["valid"] == 1).sum() > 300


def test_random_boxes_equal_the_twin(env, locator):
    c = sc.random_case(200)
    cones, m = check(env, locator, c, 1)
    v = cones[:200]
    assert (v["valid"] == 1).sum() > 100
    assert (v["n_samples"] > 1000).sum() >= 3
    assert ((v["n_valid"] == 0) & (v["n_samples"] > 0)).sum() >= 3
    assert not cones[200:].view(np.uint8).any() and not m[200:].view(np.uint8).any()


def test_two_launches_give_identical_bytes(env, locator):
    torch = env[0]
    c = sc.random_case(300, seed=77)
    pair, buf = planes(torch, c, 2), det_buffer(torch, c["dets"], c["count"])
    a = run_device(env, locator, c, pair=pair, buf=buf)          # the output buffers are filled with 0xFF before each launch
    b = run_device(env, locator, c, pair=pair, buf=buf)
    want = twin(env, c)
    for x, y, z in zip(a, b, want):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_side_by_side_buffer_and_no_match_output(env, locator):
    """right = left + width in one buffer of pitch 2 * width + 5; then the same launch with d_match = NULL, which leaves the
    match buffer alone."""
    torch = env[0]
    c, _ = sc.integer_case()
    both = np.full((sc.H, 2 * sc.W + 5), 0x5A, dtype=np.uint8)
    both[:, :sc.W], both[:, sc.W:2 * sc.W] = c["left"], c["right"]
    dev = torch.from_numpy(both).cuda()
    pair = (dev[:, :sc.W], dev[:, sc.W:2 * sc.W])
    assert pair[1].data_ptr() == pair[0].data_ptr() + sc.W and pair[0].stride(0) == 2 * sc.W + 5
    want = twin(env, c)
    assert_equal(run_device(env, locator, c, pair=pair), want, "side_by_side")
    cones, match = run_device(env, locator, c, pair=pair, match=False)
    assert cones.tobytes() == want[0].tobytes()
    assert (match.view(np.uint8) == 0xFF).all()


def test_other_streams_and_strided_views(env, locator):
    """On a side stream, planes that are column windows of wider tensors (the row stride is the pitch)."""
    torch = env[0]
    s = torch.cuda.Stream()
    c = sc.random_case(60, seed=31)
    wide = [np.full((sc.H, sc.W + 9), 0xC3, dtype=np.uint8) for _ in range(2)]
    wide[0][:, 4:4 + sc.W], wide[1][:, 4:4 + sc.W] = c["left"], c["right"]
    left, right = (torch.from_numpy(x).cuda()[:, 4:4 + sc.W] for x in wide)
    buf = det_buffer(torch, c["dets"], c["count"])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        locator.out.fill_(0xFF)
        locator.match.fill_(0xFF)
        locator.update_from_buffer(buf, left, right, c["cam"], c["baseline"], c["params"], stream=s)
        got = locator.read(s)
    assert_equal(got, twin(env, c), "side stream")


def test_behind_a_letterboxed_frame_and_in_front_of_the_tracker(env, locator, pkg, sd7):
    """The node's call order on one stream: infer_letterbox_frame (asynchronous, boxes in camera pixels) on a 96 x 72 BGRA frame,
    unina_locate_stereo_async on a 96 x 72 pair whose left plane is that frame's luma, unina_track_update_async; nothing between
    the three touches the host. The three outputs equal locate_stereo_numpy followed by update_numpy."""
    torch, engine, localize = env
    from unina_yolo_dla_amd import tracking
    g = pkg.graph.Graph(in_h=64, in_w=64)
    eng = engine.Engine.from_state_dict(sd7, g, device=0)
    tracker = tracking.DeviceTracker()
    try:
        w, h = 96, 72
        rng = np.random.RandomState(5)
        bgra = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
        d_bgra = torch.from_numpy(bgra.reshape(h, 4 * w)).cuda()
        frame = engine.Frame.from_tensors(engine.FMT_BGRA, w, h, d_bgra, 4 * w)
        px = bgra.astype(np.int32)
        left = ((29 * px[:, :, 0] + 150 * px[:, :, 1] + 77 * px[:, :, 2] + 128) >> 8).astype(np.uint8)      # BT.601 luma of the frame
        right = rng.randint(0, 256, (h, w)).astype(np.uint8)
        right[:, :w - 4] = left[:, 4:]                                                                        # the scene at disparity 4
        c = sc.case("node", None, left, right, count=0, cam=(80.0, 80.0, 47.5, 35.5), baseline=0.25, shrink=0.5, max_side=16)
        pair = planes(torch, c, 1)
        par = tracking.make_params(gate=0.5, alpha=0.5, birth_confidence=0.05, confirm_hits=1, max_missed=1)
        out = torch.full((sc.MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")
        assign = torch.full((sc.MAXD,), -1, dtype=torch.int32, device="cuda")
        locator.out.fill_(0xFF)
        locator.match.fill_(0xFF)
        tracker.reset()
        torch.cuda.synchronize()
        eng.infer_letterbox_frame(frame, None, 0.05, 0.45, 0.1, 114.0, True, out=out)
        locator.update_from_buffer(out, pair[0], pair[1], c["cam"], c["baseline"], c["params"])
        tracker.update_from_buffer(out, locator.out, par, assign=assign)
        header, tracks = tracker.read()
        cones, match = locator.read()
        dets = engine.Engine.unpack(out)
        got_assign = assign.cpu().numpy()
    finally:
        tracker.close()
        eng.close()
    assert len(dets) > 0
    want_cones, want_match = localize.locate_stereo_numpy(dets, len(dets), left, right, c["cam"], c["baseline"], c["params"])
    assert_equal((cones, match), (want_cones, want_match), "node order")
    located = (cones["valid"][:len(dets)] == 1).sum()
    sure = (cones["valid"][:len(dets)] == 1) & (cones["n_samples"][:len(dets)] >= 9)           # too many samples to match noise by chance
    assert located > 0 and (match["d_best"][:len(dets)][sure] == 4).all()
    state, want_assign = tracking.update_numpy(tracking.new_state(), dets, len(dets), want_cones, par)
    assert header.tobytes() == state["header"].tobytes() and tracks.tobytes() == state["tracks"].tobytes()
    assert got_assign.tobytes() == want_assign.tobytes() and state["header"]["n_born"][0] > 0
    print(f"{len(dets)} records, {located} located, {state['header'][0]}")
