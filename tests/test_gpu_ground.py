"""csrc/ground.hip on the GPU through unina_ground_filter_async: every comparison is BYTE equality with ground.ground_numpy -- of
the n_points entries of d_out, of the label bytes, of the nx * ny words of cellmin and of g, and of the header (integer
decisions, and fp32 values with a fixed operation order: no tolerance). d_out and what unina_ground_buffers hands out are filled
with 0xFF before each call. Clouds are uploaded as points of 12, 16, 32 or 48 bytes with NaN bit patterns in every byte that is
not x, y or z, at bases that are 16-byte aligned or only 4-byte aligned. What each constructed case contains is asserted on the
twin in tests/test_ground_cpu.py.

The sizes at which the kernels change path (tests/ground_cases.py names them beside the kernels' constants):
  points 63, 64 | 65: kWave; 1023, 1024 | 1025: kPtBlock, one word of the scan | two; 2049: three words, a scan thread with fewer
  than kScanPer; 70 001: 69 words                                                              -- cloud_size_cases
  lanes of a wave in one cell 1, 2, 3, 64: the fold in front of the atomicMin                   -- shared_lanes_case, one_cell_case
  grid 31, 32 | 33 x 7, 8 | 9: kTileX x kTileY, one envelope workgroup | two; reach 0 | 4: no halo | kGroundMaxReach   -- grid_cases"""
import numpy as np
import pytest

import ground_cases as gc
from clouds import STRIDES, upload_cloud
from records import assert_records_equal, det_buffer

pytestmark = pytest.mark.gpu

MAX_POINTS = 1 << 17
NAMES = ("out", "labels", "cellmin", "ground", "header")


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import engine, ground, localize
    return torch, ground, localize, engine


@pytest.fixture(scope="module")
def filt(env):
    f = env[1].DeviceGroundFilter(MAX_POINTS)
    yield f
    f.close()


def spoil(env, f, n_points, nx, ny):
    """0xFF over d_out and over what the call is to write of the workspace, once there is one."""
    f.out[:max(n_points, 1)].fill_(0xFF)
    if f.L.unina_ground_buffers(f.h, None, None, None, None) == 0:
        labels, cellmin, ground, header = f.buffers()
        for address, n_bytes in ((labels, n_points), (cellmin, 4 * nx * ny), (ground, 4 * nx * ny), (header, 32)):
            if n_bytes:
                env[3].device_view(address, n_bytes, device=f.device).fill_(0xFF)


def run_device(env, f, c, stride=16, offset=0, cloud=None):
    cloud = upload_cloud(env[0], c["points"], stride, offset) if cloud is None else cloud
    p = c["params"]
    spoil(env, f, len(c["points"]), p["nx"], p["ny"])
    f.filter_async(cloud, c["m"], p)
    header, out = f.read()
    cellmin, ground = f.read_grids()
    return {"out": out, "labels": f.read_labels(), "cellmin": cellmin, "ground": ground, "header": header}


def twin(env, c):
    return env[1].ground_numpy(c["points"], c["m"], c["params"])


def assert_equal(got, want, name):
    for what in NAMES:
        assert_records_equal(got[what], want[what], f"{name}: header {got['header']}", what)


def check(env, f, c, stride=16, offset=0, want=None):
    got = run_device(env, f, c, stride, offset)
    assert_equal(got, twin(env, c) if want is None else want, c["name"])
    return got


def test_cloud_sizes_on_the_edges_of_wave_workgroup_and_scan(env, filt):
    """0, 1, 63, 64, 65, 1023, 1024, 1025, 2049 and 70 001 points, keep_unknown 0 and 1 in turn. The empty cloud leaves d_out alone."""
    for k, c in enumerate(gc.cloud_size_cases()):
        got = check(env, filt, c, STRIDES[k % 4], (0, 4)[k % 2])
        assert got["header"]["n_points"][0] == len(c["points"]) == len(got["out"])
        if k == 0:
            assert (filt.out[:1].cpu().numpy() == 0xFF).all() and not got["header"].view(np.uint8).any()


def test_kept_patterns(env, filt):
    """Every point kept, none, every other one, and only points of the last workgroup: the scan's words are 1024, 0, 512 and 0, 0, 0, 50."""
    got = {c["name"]: check(env, filt, c) for c in gc.kept_pattern_cases()}
    n = 3 * gc.POINT_BLOCK + 100
    assert [int(got[k]["header"]["n_kept"][0]) for k in ("all_kept", "none_kept", "alternating", "last_workgroup")] == [n, 0, n // 2, 50]


def test_one_atomic_target_and_sixty_four(env, filt):
    """Every point in one cell; every lane of a wave in a cell of its own; runs of 2, 3 and 64 lanes that share a cell with the
    minimum in the first, a middle and the last lane."""
    assert check(env, filt, gc.one_cell_case())["header"]["n_cells_seeded"][0] == 1
    assert check(env, filt, gc.distinct_cells_case())["header"]["n_cells_seeded"][0] == 4096
    c, runs = gc.shared_lanes_case()
    got = check(env, filt, c)
    assert got["header"]["n_cells_seeded"][0] == len(runs) == 165


def test_grids_on_the_edges_of_the_envelope_tile(env, filt):
    """1 x 1, 1 x 300, 300 x 1, and 31, 32, 33 by 7, 8, 9 cells, each with reach 0 and 4; 1024 x 1024 with seeds only in the four corners."""
    for k, c in enumerate(gc.grid_cases()):
        check(env, filt, c, STRIDES[k % 4], 4 * (k % 3))
    for reach in (0, gc.MAX_REACH):
        got = check(env, filt, gc.corners_case(reach))
        assert got["header"]["n_cells_seeded"][0] == 4 and (got["ground"] != 0xffffffff).sum() == 4 * (reach + 1) ** 2


def test_strides_and_alignment(env, filt):
    """Strides of 12, 16, 32 and 48 bytes; bases 0, 4, 8 and 12 bytes past a 16-byte boundary. Only stride 16, 32 or 48 at offset 0
    takes the 16-byte loads, in the seed kernel and in the scatter."""
    c = gc.random_case(50, 3001, keep_unknown=1)
    want = twin(env, c)
    assert 500 < want["header"]["n_kept"][0] < 2000
    for stride in STRIDES:
        for offset in (0, 4, 8, 12):
            check(env, filt, c, stride, offset, want)


def test_two_runs_and_a_permuted_cloud(env, filt):
    """Two runs give identical bytes; a permuted cloud gives every point its label and the same grids and header."""
    c = gc.random_case(51, 20000, nx=40, ny=30, reach=2)
    want = twin(env, c)
    cloud = upload_cloud(env[0], c["points"])
    a, b = run_device(env, filt, c, cloud=cloud), run_device(env, filt, c, cloud=cloud)
    assert_equal(a, want, "first run")
    assert_equal(b, want, "second run")
    order = np.random.RandomState(2).permutation(len(c["points"]))
    shuffled = dict(c, points=c["points"][order], name="permuted")
    p = check(env, filt, shuffled, stride=32)
    assert p["labels"].tobytes() == want["labels"][order].tobytes()
    for what in ("cellmin", "ground", "header"):
        assert p[what].tobytes() == want[what].tobytes(), what


def test_one_handle_through_a_large_cloud_a_tiny_one_and_another_grid(env, filt):
    """70 001 points on 16 x 12, one point, 1024 x 1024, 3 x 3 and the first again: each result equals the twin and a fresh handle's."""
    sizes = gc.cloud_size_cases()
    for c in (sizes[-1], sizes[1], gc.corners_case(1), gc.one_cell_case(), sizes[-1]):
        want = twin(env, c)
        got = check(env, filt, c, want=want)
        fresh = env[1].DeviceGroundFilter(MAX_POINTS)
        try:
            other = check(env, fresh, c, want=want)
        finally:
            fresh.close()
        assert all(got[k].tobytes() == other[k].tobytes() for k in NAMES)


def test_a_side_stream_and_a_float_tensor_cloud(env, filt):
    """On a side stream, with the cloud a [n, 4] float32 tensor (x, y, z, intensity): the row stride is the point stride."""
    torch = env[0]
    c = gc.random_case(52, 5000)
    xyzi = np.concatenate([c["points"], np.full((len(c["points"]), 1), np.nan, dtype=np.float32)], axis=1)
    cloud = torch.from_numpy(xyzi).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        spoil(env, filt, len(xyzi), 16, 12)
        filt.filter_async(cloud, c["m"], c["params"], stream=s)
        header, out = filt.read(s)
        cellmin, ground = filt.read_grids(s)
        got = {"out": out, "labels": filt.read_labels(s), "cellmin": cellmin, "ground": ground, "header": header}
    assert_equal(got, twin(env, c), "side stream")


def test_in_front_of_the_locator_with_nothing_between_the_two_calls(env, filt):
    """The filtered buffer goes straight into DeviceLidarLocator on the same stream, no synchronisation between the two calls: the
    unina_cone3d bytes equal locate_lidar_numpy on the twin's `out`. On the cone scene the raw cloud's depth is a road return
    4.8 m behind the cone, the filtered cloud's a cone return, exactly as tests/test_ground_cpu.py established on the twins; then
    the same chain on a mounted LiDAR with 200 random records."""
    torch, ground, localize, _ = env
    import lidar_cases as lc
    locator = localize.DeviceLidarLocator(max_points=MAX_POINTS, max_width=2048, max_height=2048)
    try:
        s = gc.cone_scene()
        buf, cloud = det_buffer(torch, s["dets"], s["count"]), upload_cloud(torch, s["points"], 32)
        args = (s["to_cam"], s["cam"], s["width"], s["height"], s["lidar_params"])
        locator.out.fill_(0xFF)
        locator.update_from_buffer(buf, cloud, *args)
        raw = locator.read()
        spoil(env, filt, len(s["points"]), s["params"]["nx"], s["params"]["ny"])
        locator.out.fill_(0xFF)
        kept = filt.filter_async(cloud, s["m"], s["params"])
        locator.update_from_buffer(buf, kept, *args)
        filtered = locator.read()
        header, out = filt.read()
        g = ground.ground_numpy(s["points"], s["m"], s["params"])
        assert out.tobytes() == g["out"].tobytes() and header.tobytes() == g["header"].tobytes()
        assert raw.tobytes() == localize.locate_lidar_numpy(s["dets"], 1, s["points"], *args).tobytes()
        assert filtered.tobytes() == localize.locate_lidar_numpy(s["dets"], 1, g["out"], *args).tobytes()
        gc.assert_scene(s, raw, filtered, out)
        assert raw["n_samples"][0] == 45 and filtered["n_samples"][0] == 16

        c = lc.random_case(200, 30000, seed=78)       # points all over a 100 x 70 image, seen by a LiDAR whose z is up
        level = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.5)
        par = dict(x_min=0.0, y_min=-20.0, cell=0.5, nx=100, ny=80, z_lo=-2.0, z_hi=0.5, rise=0.1, band=0.3, max_height=2.0, reach=2, keep_unknown=1)
        args = (c["m"], c["cam"], c["width"], c["height"], c["params"])
        buf, cloud = det_buffer(torch, c["dets"], c["count"]), upload_cloud(torch, c["points"], 48, 4)
        spoil(env, filt, len(c["points"]), par["nx"], par["ny"])
        locator.out.fill_(0xFF)
        locator.update_from_buffer(buf, filt.filter_async(cloud, level, par), *args)
        cones = locator.read()
        g = ground.ground_numpy(c["points"], level, par)
        want = localize.locate_lidar_numpy(c["dets"], c["count"], g["out"], *args)
        assert cones.tobytes() == want.tobytes()
        unfiltered = localize.locate_lidar_numpy(c["dets"], c["count"], c["points"], *args)
        assert 0.05 * len(c["points"]) < g["header"]["n_kept"][0] < 0.9 * len(c["points"]) and (want["valid"] == 1).sum() > 20
        assert (want["n_samples"] < unfiltered["n_samples"]).sum() > 20
    finally:
        locator.close()
