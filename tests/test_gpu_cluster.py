"""csrc/cluster.hip on the GPU through unina_cluster_async: every comparison is BYTE equality with cluster.cluster_numpy -- of the
header, of the n_components entries of the table, of the per-point component indices, and of all MAX_DETECTIONS GpuDetection and
unina_cone3d records and the count (integer decisions, and fp32 values with a fixed operation order: no tolerance). The outputs
and what unina_cluster_buffers hands out are filled with 0xFF before each call. Clouds are uploaded as points of 12, 16, 32 or 48
bytes with NaN bit patterns in every byte that is not x, y or z, at bases that are 16-byte aligned or only 4-byte aligned. What
each constructed case contains is asserted on the twin in tests/test_cluster_cpu.py.

The sizes at which the kernels change path (tests/cluster_cases.py names them beside the kernels' constants):
  points 63, 64 | 65: kWave; 255, 256 | 257: kPtBlock; 1023, 1024 | 1025: kSumBlock; 70 001 in one cell: one atomic target in LDS
  and in the table, Sx > 2^32; more components in a workgroup than kSlots: the rest goes to the table directly   -- cloud_size_cases, wall_case
  grid 31, 32 | 33 in each axis: kTile, one label workgroup | two, with or without a merge launch           -- grid_cases
  components on a tile border, on the corner of four tiles, chains through one tile and through nine        -- straddle_case, shape_cases
  cones 1023, 1024 | 1025: MAX_DETECTIONS; components 2500: three workgroups of kRowBlock in finish and emit -- count_cases"""
import numpy as np
import pytest

import cluster_cases as cc
import ground_cases as gc
from clouds import STRIDES, upload_cloud
from records import assert_records_equal

pytestmark = pytest.mark.gpu

MAX_POINTS = 1 << 17
NAMES = ("header", "components", "point_component", "dets", "cones", "count")


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import cluster, engine, ground, tracking
    return torch, cluster, engine, ground, tracking


@pytest.fixture(scope="module")
def clus(env):
    c = env[1].DeviceClusterer(MAX_POINTS)
    yield c
    c.close()


def spoil(env, c, n_points):
    """0xFF over the outputs and over what the call is to write of the workspace, once there is one: the header, the per-point
    array, and as many table entries as there can be components."""
    c.det_buf.fill_(-1)
    c.cones.fill_(0xFF)
    if c.L.unina_cluster_buffers(c.h, None, None, None) == 0:
        table, comp, header = c.buffers()
        for address, n_bytes in ((table, 48 * n_points), (comp, 4 * n_points), (header, 32)):
            if n_bytes:
                env[2].device_view(address, n_bytes, device=c.device).fill_(0xFF)


def run_device(env, c, case, stride=16, offset=0, cloud=None, stream=None):
    cloud = upload_cloud(env[0], case["points"], stride, offset) if cloud is None else cloud
    spoil(env, c, len(case["points"]))
    c.cluster_async(cloud, case["m"], case["params"], stream=stream)
    header, dets, cones, count = c.read(stream)
    return {"header": header, "components": c.read_components(stream), "point_component": c.read_point_components(stream), "dets": dets,
            "cones": cones, "count": count}


def twin(env, case):
    return env[1].cluster_numpy(case["points"], case["m"], case["params"])


def assert_equal(got, want, name):
    for what in NAMES:
        assert_records_equal(got[what], want[what], f"{name}: header {got['header']}", what)


def check(env, c, case, stride=16, offset=0, want=None):
    got = run_device(env, c, case, stride, offset)
    assert_equal(got, twin(env, case) if want is None else want, case["name"])
    return got


def test_cloud_sizes_on_the_edges_of_wave_and_workgroup(env, clus):
    """0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024 and 1025 points. The empty cloud gives all-zero outputs and an all-zero header."""
    for k, c in enumerate(cc.cloud_size_cases()):
        got = check(env, clus, c, STRIDES[k % 4], (0, 4)[k % 2])
        assert got["header"]["n_points"][0] == len(c["points"]) == len(got["point_component"])
        if k == 0:
            assert not any(got[w].view(np.uint8).any() for w in ("header", "dets", "cones", "count"))


def test_one_atomic_target_and_sums_above_32_bits(env, clus):
    """70 001 points in the last cell of a 1024-wide row."""
    got = check(env, clus, cc.wall_case())
    assert got["components"]["n_points"].tolist() == [70001] and got["components"]["root"].tolist() == [1023]


def test_grids_on_the_edges_of_the_label_tile(env, clus):
    """1 x 1, 1 x 300, 300 x 1, and 31, 32, 33 cells in each axis; 1024 x 1024 with points only in the four corners."""
    for k, c in enumerate(cc.grid_cases()):
        check(env, clus, c, STRIDES[k % 4], 4 * (k % 3))
    got = check(env, clus, cc.corners_case())
    assert got["header"]["n_components"][0] == 4


def test_components_against_the_tile(env, clus):
    """Two cells across a vertical border, a horizontal border and both diagonals of a corner of four tiles; a serpentine that fills
    one tile, one of 33 x 33, a serpentine and a spiral across 3 x 3 tiles; a fully occupied 64 x 64 grid; a checkerboard."""
    c, cells = cc.straddle_case()
    got = check(env, clus, c)
    assert (got["components"]["n_cells"] == 2).all() and len(got["components"]) == len(cells) // 2
    for c in cc.shape_cases():
        got = check(env, clus, c)
        assert got["header"]["n_components"][0] == (33 * 33 if c["name"] == "checkerboard" else 1), c["name"]


def test_counts_around_max_detections(env, clus):
    """1023, 1024 and 1025 cones; 2500 components and no cone; cones only among the last components."""
    dropped = [int(check(env, clus, c)["header"]["n_dropped"][0]) for c in cc.count_cases()]
    assert dropped == [0, 0, 1, 0, 0]


def test_gate_thresholds(env, clus):
    c, cones = cc.gate_case()
    got = check(env, clus, c, stride=12)
    assert got["components"]["cone"].tolist() == [int(v) for v in cones]


def test_strides_and_alignment(env, clus):
    """Strides of 12, 16, 32 and 48 bytes; bases 0, 4, 8 and 12 bytes past a 16-byte boundary. Only stride 16, 32 or 48 at offset 0
    takes the 16-byte loads, in mark and in sums."""
    c = cc.random_case(50, 3001, nx=120, ny=90, max_width=2.0)
    want = twin(env, c)
    assert want["header"]["n_components"][0] > 5 and 0 < want["count"][0] < want["header"]["n_components"][0]
    for stride in STRIDES:
        for offset in (0, 4, 8, 12):
            check(env, clus, c, stride, offset, want)


def test_two_runs_and_a_permuted_cloud(env, clus):
    """Two runs give identical bytes; a permuted cloud gives the same header, table, records and count, and every point its component."""
    occupied = np.random.RandomState(3).rand(90, 120) < 0.3
    c = cc.occupancy_case("random_occupancy", occupied, per_cell=3, seed=5, max_width=2.5)
    want = twin(env, c)
    assert want["header"]["n_components"][0] > 100 and 10 < want["count"][0] < want["header"]["n_components"][0]
    cloud = upload_cloud(env[0], c["points"])
    a, b = run_device(env, clus, c, cloud=cloud), run_device(env, clus, c, cloud=cloud)
    assert_equal(a, want, "first run")
    assert_equal(b, want, "second run")
    order = np.random.RandomState(2).permutation(len(c["points"]))
    p = check(env, clus, dict(c, points=c["points"][order], name="permuted"), stride=32)
    assert p["point_component"].tobytes() == want["point_component"][order].tobytes()
    for what in ("header", "components", "dets", "cones", "count"):
        assert p[what].tobytes() == want[what].tobytes(), what


def test_one_handle_through_a_large_cloud_a_tiny_one_and_another_grid(env, clus):
    """70 001 points on 1024 x 1, one point, 1024 x 1024, 96 x 96 and the first again: each result equals the twin and a fresh handle's."""
    first = cc.wall_case()
    for c in (first, cc.cloud_size_cases()[1], cc.corners_case(), cc.straddle_case()[0], first):
        want = twin(env, c)
        got = check(env, clus, c, want=want)
        fresh = env[1].DeviceClusterer(MAX_POINTS)
        try:
            other = check(env, fresh, c, want=want)
        finally:
            fresh.close()
        assert all(got[k].tobytes() == other[k].tobytes() for k in NAMES)


def test_a_side_stream_and_a_float_tensor_cloud(env, clus):
    """On a side stream, with the cloud a [n, 4] float32 tensor (x, y, z, intensity): the row stride is the point stride."""
    torch = env[0]
    c = cc.random_case(52, 5000, nx=160, ny=120, max_width=2.0)
    xyzi = np.concatenate([c["points"], np.full((len(c["points"]), 1), np.nan, dtype=np.float32)], axis=1)
    cloud = torch.from_numpy(xyzi).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = run_device(env, clus, c, cloud=cloud, stream=s)
    assert_equal(got, twin(env, c), "side stream")


def chain_numpy(env, frames, ground_params, cluster_params, track_params):
    """The twins of the three stages, frame by frame -> the tracker's state, and the clusterer's result of the last frame."""
    _, cluster, _, ground, tracking = env
    state = tracking.new_state()
    for points, m, pose in frames:
        kept = ground.ground_numpy(points, m, ground_params)["out"]
        r = cluster.cluster_numpy(kept, m, cluster_params)
        state, _ = tracking.update_numpy(state, r["dets"], int(r["count"][0]), r["cones"], dict(track_params, pose=pose))
    return state, r


def chain_device(env, clus, frames, ground_params, cluster_params, track_params):
    """Ground filter -> clusterer -> tracker on the current stream, nothing synchronised between the calls or between the frames."""
    torch, _, _, ground, tracking = env
    filt, tracker = ground.DeviceGroundFilter(MAX_POINTS), tracking.DeviceTracker()
    try:
        tracker.reset()
        clouds = [upload_cloud(torch, points, 32) for points, _, _ in frames]
        for cloud, (points, m, pose) in zip(clouds, frames):
            filt.out[:len(points)].fill_(0xFF)
            spoil(env, clus, len(points))
            kept = filt.filter_async(cloud, m, ground_params)
            det_buf, cones = clus.cluster_async(kept, m, cluster_params)
            tracker.update_from_buffer(det_buf, cones, dict(track_params, pose=pose))
        header, tracks = tracker.read()
        return {"header": header, "tracks": tracks}, clus.read()
    finally:
        filt.close()
        tracker.close()


def test_ground_filter_clusterer_and_tracker_on_one_stream(env, clus):
    """Three frames with a moving pose, on the cone scene and on two rows of cones beside a wall and a pole: the tracks equal
    tracking.update_numpy fed by the twins, byte for byte. The cone scene holds one confirmed track, the rows twelve."""
    track = dict(gate=0.5, alpha=0.5, birth_confidence=0.5, class_aware=1, confirm_hits=3, max_missed=2)
    s = gc.cone_scene()
    par = dict(x_min=0.0, y_min=-25.6, cell=0.1, nx=512, ny=512, confidence=0.9, class_id=1)
    pose = lambda dx: (1.0, 0.0, 0.0, dx, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)   # level frame -> tracking frame
    frames = [(s["points"], s["m"], pose(0.05 * f)) for f in range(3)]
    want, last = chain_numpy(env, frames, s["params"], par, track)
    got, (header, dets, cones, count) = chain_device(env, clus, frames, s["params"], par, track)
    assert got["header"].tobytes() == want["header"].tobytes() and got["tracks"].tobytes() == want["tracks"].tobytes()
    assert header.tobytes() == last["header"].tobytes() and dets.tobytes() == last["dets"].tobytes() and cones.tobytes() == last["cones"].tobytes()
    assert count[0] == 1 and (got["header"]["n_live"][0], got["header"]["n_confirmed"][0]) == (1, 1)
    assert abs(got["tracks"]["x"][0] - 15.0) < 0.2 and abs(got["tracks"]["y"][0]) < 0.05

    frames = []
    for f in range(3):
        r = cc.two_row_scene(shift=0.25 * f)                                  # the car moves 0.25 m a frame; the pose says so
        frames.append((r["points"], r["m"], pose(0.25 * f)))
    want, last = chain_numpy(env, frames, r["params"], r["cluster"], track)
    got, (header, dets, cones, count) = chain_device(env, clus, frames, r["params"], r["cluster"], track)
    assert got["header"].tobytes() == want["header"].tobytes() and got["tracks"].tobytes() == want["tracks"].tobytes()
    assert header.tobytes() == last["header"].tobytes() and dets.tobytes() == last["dets"].tobytes() and cones.tobytes() == last["cones"].tobytes()
    assert count[0] == 12 and (got["header"]["n_live"][0], got["header"]["n_confirmed"][0]) == (12, 12)
