"""csrc/lidar.hip on the GPU through unina_locate_lidar_async: every comparison is BYTE equality of the MAX_DETECTIONS unina_cone3d
with localize.locate_lidar_numpy and of the n_points unina_lidar_pixel with localize.project_lidar_numpy (integer decisions, and
fp32 values with a fixed operation order: no tolerance). The cone buffer and the pixels of the workspace are filled with 0xFF
before each call. Clouds are uploaded as points of 12, 16, 32 or 48 bytes with NaN bit patterns in every byte that is not x, y
or z, at bases that are 16-byte aligned or only 4-byte aligned. What each constructed case contains is asserted on the twin in
tests/test_lidar_cpu.py.

The thresholds at which the select kernel changes path (tests/lidar_cases.py names them beside the kernel's constants):
  candidates (points in the 32 x 32 cells a window touches) 64 | 65: kWave, a wave per record | the workgroup   -- members_case
  valid keys 8191, 8192 | 8193: kCache, keys kept in LDS between the passes | candidates walked again            -- members_case
  cells 4096 | 4160, 8192: kScanBlock * kScanPer, one pass of the scan | two; 15 cells: kScanPer, a thread with three   -- scan_edge_cases, large_image_case"""
import ctypes as C

import numpy as np
import pytest

import lidar_cases as lc
from clouds import STRIDES, upload_cloud
from records import assert_records_equal, det_buffer

pytestmark = pytest.mark.gpu

LIMITS = dict(max_points=1 << 17, max_width=4096, max_height=2048)


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import engine, localize
    return torch, engine, localize


@pytest.fixture(scope="module")
def locator(env):
    loc = env[2].DeviceLidarLocator(**LIMITS)
    yield loc
    loc.close()


def fill_pixels(env, loc, n_points):
    """0xFF over the first n_points unina_lidar_pixel of the workspace, once there is one."""
    address = C.c_void_p()
    if n_points and loc.L.unina_lidar_buffers(loc.h, C.byref(address)) == 0:
        env[1].device_view(address.value, 4 * n_points, "<i4").fill_(-1)


def run_device(env, loc, c, stride=16, offset=0, cloud=None, buf=None):
    torch = env[0]
    cloud = upload_cloud(torch, c["points"], stride, offset) if cloud is None else cloud
    buf = det_buffer(torch, c["dets"], c["count"]) if buf is None else buf
    loc.out.fill_(0xFF)
    fill_pixels(env, loc, len(c["points"]))
    loc.update_from_buffer(buf, cloud, c["m"], c["cam"], c["width"], c["height"], c["params"])
    return loc.read(), loc.read_pixels()


def twin(env, c):
    p = c["params"]
    pixels = env[2].project_lidar_numpy(c["points"], c["m"], c["cam"], c["width"], c["height"], p["min_depth"], p["max_depth"])
    cones = env[2].locate_lidar_numpy(c["dets"], c["count"], c["points"], c["m"], c["cam"], c["width"], c["height"], p, pixels=pixels)
    return cones, pixels


def check(env, loc, c, stride=16, offset=0, want=None):
    got = run_device(env, loc, c, stride, offset)
    want = twin(env, c) if want is None else want
    assert_records_equal(got[1], want[1], c["name"], "pixel")
    assert_records_equal(got[0], want[0], c["name"], "cone")
    return got


def test_constructed_cases_equal_the_twin(env, locator):
    """Members of 0, 1, 2, 63, 64, 65 and more than 65 536; candidates of 64 and 65; valid keys of 8191, 8192, 8193; equal keys, two
    values, keys that differ in one byte, mixed validity; windows in one cell, across cell corners, along the last partial cell,
    over the whole image, identical, overlapping and empty; 8192 cells; random boxes on a mounted LiDAR."""
    seen = {}
    for k, c in enumerate(lc.all_cases()):
        seen[c["name"]] = check(env, locator, c, STRIDES[k % 4], (0, 4)[k % 2])
    cones = seen["members"][0]
    assert cones["n_samples"][:6].tolist() == [0, 1, 2, 63, 64, 65] and cones["n_samples"][13] == 66000
    assert cones["n_valid"][10:13].tolist() == [lc.CACHE_KEYS - 1, lc.CACHE_KEYS, lc.CACHE_KEYS + 1]
    assert (seen["keys"][0]["z"][[0, 1, 6, 7]] == [12.5, 3.0, 12.5, 3.0]).all()
    assert (seen["image4096x2048"][0]["valid"] == 1).sum() > 20
    assert (seen["random200"][0]["valid"] == 1).sum() > 50


def test_a_sweep_ordered_cloud_folds_its_cells(env, locator):
    """The members case in the order it was built: consecutive points share a cell, so a wave's 64 points fold into one or two
    atomics; 66 000 of them go to one cell."""
    c = lc.members_case(shuffle=False)
    got = check(env, locator, c)
    assert got[0]["n_samples"][13] == 66000


def test_cloud_sizes_strides_and_alignment(env, locator):
    """n_points of 0, 1, 63, 64, 65, 255, 256 and 257; strides of 12, 16, 32 and 48 bytes; bases 0, 4, 8 and 12 bytes past a 16-byte
    boundary. Only stride 16, 32 or 48 at offset 0 takes the 16-byte loads."""
    cases = lc.cloud_size_cases()
    for k, c in enumerate(cases):
        got = check(env, locator, c, STRIDES[k % 4], 4 * (k % 3))
        assert len(got[1]) == len(c["points"])
    full, want = cases[-1], twin(env, cases[-1])
    assert (want[1]["projectable"] == 1).sum() > 100 and (want[1]["projectable"] == 0).sum() > 10
    for stride in STRIDES:
        for offset in (0, 4, 8, 12):
            check(env, locator, full, stride, offset, want)
    assert not check(env, locator, cases[0])[0]["n_samples"].any()


def test_image_sizes_on_the_edges_of_the_scan(env, locator):
    """1, 4, 15, 4096 and 4160 cells: one cell, a last thread with fewer than four, exactly one pass, a short second pass."""
    for c in lc.scan_edge_cases():
        got = check(env, locator, c)
        assert got[0]["valid"][20] == 1


def test_counts(env, locator):
    """Counts 0, 1, 1024, 5000 (clamped) and negative: the slots at and beyond the count are zero bytes."""
    got = {c["name"]: check(env, locator, c)[0] for c in lc.count_cases()}
    for name in ("count0", "count_negative"):
        assert not got[name].view(np.uint8).any()
    assert got["count1"]["u"][0] == 1.5 and not got["count1"][1:].view(np.uint8).any()
    assert got["count5000"].tobytes() == got["count1024"].tobytes() and (got["count1024"]["u"] != 0).all()


def test_a_permuted_cloud_and_a_second_run_give_identical_cones(env, locator):
    torch = env[0]
    c = lc.random_case(300, 20000, seed=77)
    want = twin(env, c)
    cloud, buf = upload_cloud(torch, c["points"]), det_buffer(torch, c["dets"], c["count"])
    a = run_device(env, locator, c, cloud=cloud, buf=buf)
    b = run_device(env, locator, c, cloud=cloud, buf=buf)
    assert a[0].tobytes() == b[0].tobytes() == want[0].tobytes() and a[1].tobytes() == b[1].tobytes() == want[1].tobytes()
    order = np.random.RandomState(2).permutation(len(c["points"]))
    shuffled = dict(c, points=c["points"][order])
    p = run_device(env, locator, shuffled, stride=32)
    assert p[0].tobytes() == want[0].tobytes() and p[1].tobytes() == want[1][order].tobytes()
    assert (want[0]["valid"] == 1).sum() > 100 and (want[0]["n_samples"] > 1000).sum() >= 3


def test_one_handle_through_a_large_cloud_a_tiny_one_and_another_image_size(env, locator):
    """91 000 points on 512 x 128, one point on 100 x 70, 3000 points on 100 x 70, 20 000 on 4096 x 2048 and the first again: each
    result equals the twin and a fresh handle's."""
    localize = env[2]
    sequence = [lc.members_case(), lc.cloud_size_cases()[1], lc.geometry_case(), lc.large_image_case(), lc.members_case()]
    for c in sequence:
        want = twin(env, c)
        got = check(env, locator, c, want=want)
        fresh = localize.DeviceLidarLocator(**LIMITS)
        try:
            other = check(env, fresh, c, want=want)
        finally:
            fresh.close()
        assert got[0].tobytes() == other[0].tobytes() and got[1].tobytes() == other[1].tobytes()


def test_a_side_stream_and_a_float_tensor_cloud(env, locator):
    """On a side stream, with the cloud a [n, 4] float32 tensor (x, y, z, intensity): the row stride is the point stride."""
    torch = env[0]
    c = lc.random_case(60, 5000, seed=31)
    xyzi = np.concatenate([c["points"], np.full((len(c["points"]), 1), np.nan, dtype=np.float32)], axis=1)
    cloud, buf = torch.from_numpy(xyzi).cuda(), det_buffer(torch, c["dets"], c["count"])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        locator.out.fill_(0xFF)
        locator.update_from_buffer(buf, cloud, c["m"], c["cam"], c["width"], c["height"], c["params"], stream=s)
        cones, pixels = locator.read(s), locator.read_pixels(s)
    want = twin(env, c)
    assert_records_equal(pixels, want[1], "side stream", "pixel")
    assert_records_equal(cones, want[0], "side stream", "cone")


def test_in_front_of_the_tracker_for_three_frames(env, locator):
    """DeviceTracker behind DeviceLidarLocator on one stream, nothing between the two touches the host: tracks, header and assign
    equal tracking.update_numpy behind locate_lidar_numpy, and the eight cones keep their ids."""
    torch = env[0]
    from unina_yolo_dla_amd import tracking
    tracker = tracking.DeviceTracker()
    par = tracking.make_params(gate=1.0, alpha=0.5, birth_confidence=0.05, confirm_hits=2, max_missed=1)
    state = tracking.new_state()
    try:
        tracker.reset()
        for c in lc.tracker_frames():
            cloud, buf = upload_cloud(torch, c["points"]), det_buffer(torch, c["dets"], c["count"])
            locator.out.fill_(0xFF)
            tracker.assign.fill_(-1)
            locator.update_from_buffer(buf, cloud, c["m"], c["cam"], c["width"], c["height"], c["params"])
            tracker.update_from_buffer(buf, locator.out, par)
            header, tracks = tracker.read()
            cones = locator.read()
            want_cones, _ = twin(env, c)
            assert_records_equal(cones, want_cones, c["name"], "cone")
            assert (want_cones["valid"][:8] == 1).all() and (np.abs(want_cones["z"][:8] - (6.0 + 2.0 * np.arange(8))) < 0.1).all()
            state, want_assign = tracking.update_numpy(state, c["dets"], c["count"], want_cones, par)
            assert header.tobytes() == state["header"].tobytes() and tracks.tobytes() == state["tracks"].tobytes()
            assert tracker.assign.cpu().numpy().tobytes() == want_assign.tobytes()
            assert want_assign[:8].tolist() == list(range(1, 9))
    finally:
        tracker.close()
    assert state["header"]["n_confirmed"][0] == 8 and state["header"]["frame"][0] == 3
