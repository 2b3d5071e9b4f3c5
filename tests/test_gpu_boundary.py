"""csrc/boundary.hip on the GPU through unina_boundary_async: every comparison is BYTE equality with boundary.boundary_numpy -- of
the header and of all 256 points (integers, and fp32 values with a fixed operation order: no tolerance). What each constructed
case contains is asserted on the twin in tests/test_boundary_cpu.py; every output byte is 0xFF before each launch."""
import numpy as np
import pytest

import boundary_cases as bc
import pose_cases as pc
from records import assert_records_equal, det_buffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import boundary, engine
    return torch, engine, boundary


@pytest.fixture(scope="module")
def finder(env):
    return env[2].DeviceBoundaryFinder(None)


def words(torch, records):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.int32).reshape(-1).copy()).cuda()


def run_device(env, finder, c, stream=None):
    """One call -> (header, points)."""
    torch = env[0]
    finder.tracks = words(torch, c["tracks"])
    finder.pose = None if c["dpose"] is None else words(torch, c["dpose"])

    def go():
        finder.points.fill_(0xFF)
        finder.header.fill_(0xFF)
        finder.find_async(c["params"], stream=stream)
    torch.cuda.synchronize()
    if stream is None:
        go()
    else:
        with torch.cuda.stream(stream):
            go()
    return finder.read(stream)


def compare(name, got, want):
    assert got[0].tobytes() == want[0].tobytes(), (name, got[0], want[0])
    assert_records_equal(got[1], want[1], name, "point")


def test_edge_cases_equal_the_twin(env, finder):
    """An empty table, one side only, a free slot with coordinates, hits one short, a third class, NaN and inf in x and y, |x| =
    32768 and just beyond; the first gate, the step gate and the turn test on their bounds and one ulp beyond; a cone abeam and one
    behind; a second track at the current cone's place; a closed ring of 8; equal d2 towards slots 5 and 1000; max_chain = 1; 63,
    64 and 65 cones in a line; 1024 candidates of one class; ladders of 1 x 64 and 64 x 64; the width gate on its bound and beyond;
    an advance tie; no heading from the forward axis and from a NaN in the device pose; a device pose beside another pose."""
    cases = bc.edge_results()
    assert len(cases) == 35
    for c, want in cases:
        compare(c["name"], run_device(env, finder, c), want)


def test_edge_cases_on_a_side_stream_equal_the_twin(env, finder):
    stream = env[0].cuda.Stream()
    for c, want in bc.edge_results():
        compare(c["name"] + " side stream", run_device(env, finder, c, stream=stream), want)


def test_oval_repeats_and_permuted_slots(env, finder):
    """The oval at one seed; two runs give identical bytes; another order of the slots gives the same points and header."""
    c, want, n = bc.oval_result(0, 1 / 3)
    a, b = run_device(env, finder, c), run_device(env, finder, c)
    compare(c["name"], a, want)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert want[0]["n_chain"][0].tolist() == [n, n]
    compare("permuted", run_device(env, finder, bc.permuted(c)), want)
    k = {c["name"]: (c, w) for c, w in bc.edge_results()}["all_1024_of_one_class"]
    a, b = run_device(env, finder, k[0]), run_device(env, finder, k[0])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_misaligned_and_overlapping_pointers_are_refused(env, finder):
    """Real device buffers, 4 or 8 bytes off a 16-byte boundary, or the header inside the points: UNINA_ERR_ARG, nothing written."""
    import ctypes as C
    torch, engine, boundary = env
    c = bc.edge_results()[2][0]
    assert c["name"] == "plain"
    tracks = words(torch, c["tracks"])
    wide = torch.full((4096,), -1, dtype=torch.int32, device="cuda")
    par = boundary.as_params(c["params"])
    good = dict(tracks=tracks.data_ptr(), pose=wide.data_ptr() + 8192, points=wide.data_ptr(), hdr=wide.data_ptr() + 4096)
    for key, off in (("tracks", 4), ("tracks", 8), ("pose", 4), ("pose", 8), ("points", 4), ("points", 8), ("hdr", 8), ("hdr", 4), ("hdr", -16), ("hdr", -4096)):
        a = dict(good)
        a[key] += off
        assert finder.L.unina_boundary_async(a["tracks"], a["pose"], C.byref(par), a["points"], a["hdr"], None) == 4, (key, off)
    torch.cuda.synchronize()
    assert (wide.cpu().numpy() == -1).all()
    with pytest.raises(engine.EngineError):
        finder.tracks = tracks[1:]
        finder.find_async(c["params"])


def test_the_drive_on_the_device_equals_the_chain_of_twins(env):
    """12 frames of a vehicle driving the oval, on one stream with nothing read in between: unina_pose_async (the earlier result
    chained, the cones in place) -> unina_track_update_async with the identity -> unina_boundary_async on the tracker's own
    buffers with the pose stage's d_result as d_pose. After the last frame the table, the pose and the boundary equal the three
    twins chained the same way, byte for byte -- and so do the boundary's bytes of every frame before, copied on the stream."""
    torch, engine, boundary = env
    from unina_yolo_dla_amd import pose, tracking
    frames, incs, _, n = bc.drive_inputs()
    want = bc.drive_results()
    tracker = tracking.DeviceTracker()
    try:
        tracker.reset()
        torch.cuda.synchronize()
        tracks_at, header_at = tracker.buffers()
        table = engine.device_view(header_at, 32 + 32 * bc.MAXD)
        est = pose.DevicePoseEstimator.from_tracker(tracker)
        find = boundary.DeviceBoundaryFinder(tracker, pose=est.result)
        assert find.tracks == tracks_at
        bufs, cones = [], []
        for f in frames:
            dets, cn = pc.padded_frame(f)
            bufs.append(det_buffer(torch, dets, f["count"]))
            cones.append(words(torch, cn))
        find.points.fill_(0xFF)
        find.header.fill_(0xFF)
        torch.cuda.synchronize()
        snaps = []
        for k, f in enumerate(frames):
            moved = est.estimate_from_buffer(bufs[k], cones[k], dict(bc.DRIVE_POSE, inc=incs[k]), chain=k > 0, in_place=True)
            tracker.update_from_buffer(bufs[k], moved, dict(f["params"], pose=None), assign=False)
            points, header = find.find_async(bc.DRIVE_BOUNDARY)
            snaps.append((header.clone(), points.clone()))                                  # copies on the same stream, no synchronisation
        last = (est.result.clone(), table.clone())
        torch.cuda.synchronize()
        got = [(h.cpu().numpy().view(engine.BOUNDARY_HEADER_DTYPE), p.cpu().numpy().view(engine.BOUNDARY_POINT_DTYPE)) for h, p in snaps]
        result, tab = (t.cpu().numpy() for t in last)
    finally:
        tracker.close()
    r, state, _ = want[-1]
    assert result.tobytes() == r["result"].tobytes()
    assert tab[:32].tobytes() == state["header"].tobytes()
    assert_records_equal(tab[32:].view(tracking.TRACK_DTYPE), state["tracks"], "drive", "slot")
    for k, (g, w) in enumerate(zip(got, want)):
        compare(f"drive frame {k}", g, w[2])
    # both chains in ring order: each cone 2 .. 6.5 m of centre-line arc behind the next (the cones stand 4 m apart)
    header, points = got[-1]
    left, right, centre = boundary.split(header, points)
    assert min(len(left), len(right)) >= 4 and len(centre) == len(left) + len(right) - 1
    line = bc.cached(("line", 30.0, 15.0), bc.oval_line)
    quarter = slice(0, len(line[0]) // 4, 20)
    for side in (left, right):
        along = [float(line[0][quarter][((line[1][quarter] - np.array([p["x"], p["y"]])) ** 2).sum(axis=1).argmin()]) for p in side]
        assert (np.diff(along) > 2.0).all() and (np.diff(along) < 6.5).all(), along
