"""csrc/fuse.hip on the GPU through unina_fuse_async: every comparison is BYTE equality with fusion.fuse_numpy -- of the header and
the count, of all 1024 records of both arrays, of all 1024 links and of all 1024 d_lidar_slot words (integers, and fp32 values with
a fixed operation order: no tolerance). What each constructed case contains is asserted on the twin in tests/test_fuse_cpu.py; the
input buffers carry NaN bit patterns behind the records, every output word is -1 before each launch."""
import numpy as np
import pytest

import cluster_cases as cc
import fuse_cases as fc
from clouds import upload_cloud
from records import assert_records_equal, det_buffer, padded_words

pytestmark = pytest.mark.gpu

NAMES = ("header", "dets", "cones", "count", "links", "lidar_slot")


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import engine, fusion
    return torch, engine, fusion


@pytest.fixture(scope="module")
def fuser(env):
    return env[2].DeviceFuser()


def upload(torch, c):
    """The four input buffers of a case on the device, garbage behind the records."""
    cones = lambda a: torch.from_numpy(padded_words(a, 8 * fc.MAXD)).cuda()      # noqa: E731
    return det_buffer(torch, c["dets"], c["count"]), cones(c["cones"]), det_buffer(torch, c["ldets"], c["lcount"]), cones(c["lcones"])


def spoil(fuser):
    fuser.det_buf.fill_(-1)
    fuser.lidar_slot.fill_(-1)
    for t in (fuser.cones, fuser.links, fuser.header):
        t.fill_(0xFF)


def run_device(env, fuser, c, stream=None, lidar_slot=None, buffers=None):
    torch = env[0]
    buffers = upload(torch, c) if buffers is None else buffers
    torch.cuda.synchronize()
    if stream is None:
        spoil(fuser)
        fuser.fuse_from_buffers(*buffers, c["params"], lidar_slot=lidar_slot)
    else:
        with torch.cuda.stream(stream):
            spoil(fuser)
            fuser.fuse_from_buffers(*buffers, c["params"], stream=stream, lidar_slot=lidar_slot)
    return dict(zip(NAMES, fuser.read(stream)))


def compare(name, got, want, skip=()):
    for what in NAMES:
        if what not in skip:
            assert_records_equal(got[what], want[what], f"{name}: header {got['header']}", what)


def test_edge_cases_equal_the_twin(env, fuser):
    """Counts 0 / 1 / 63 / 64 / 65 / 1024 / 5000 (clamped) / negative on either side; 24 of 100 LiDAR-only cones written and 76
    dropped; all dropped; all cones invalid; NaN and inf coordinates and a transform that overflows; a cone behind the camera; zc
    on and one ulp outside both depth bounds; a pixel on the grown box's border and one ulp outside, on each axis; the depth gate
    at equality and one ulp over; a camera cone without a depth; inverted and NaN boxes; grow = pad = 0; grid ties; one cone in
    two boxes, with and without a separating depth; two cones in one box; the 64-round chain, also across a wave boundary; NaN
    confidences; scaled records."""
    cases = fc.cached("edges", fc.edge_cases)
    assert len(cases) == 42
    for c, want in cases:
        compare(c["name"], run_device(env, fuser, c), want)


def test_scene_equals_the_twin(env, fuser):
    """About 150 cones on a track seen by both sensors, noise-free, noisy with pad = 0 and noisy with pad = 4."""
    for c, want in fc.cached("scene", fc.scene_cases):
        compare(c["name"], run_device(env, fuser, c), want)
        assert set(want["links"]["kind"][:want["count"][0]].tolist()) == {1, 2, 3}


def test_repeats_side_stream_no_slot_array_and_other_counts_give_the_same_bytes(env, fuser):
    torch = env[0]
    cases = dict((c["name"], (c, want)) for c, want in fc.cached("edges", fc.edge_cases))
    (scene, want), = [x for x in fc.cached("scene", fc.scene_cases) if x[0]["name"] == "scene_noisy_pad4"]
    a = run_device(env, fuser, scene)
    b = run_device(env, fuser, scene)
    for what in NAMES:
        assert a[what].tobytes() == b[what].tobytes(), what
    compare("repeat", b, want)
    compare("side stream", run_device(env, fuser, scene, stream=torch.cuda.Stream()), want)
    got = run_device(env, fuser, scene, lidar_slot=False)                       # d_lidar_slot = NULL: nothing is written there
    compare("no slot array", got, want, skip=("lidar_slot",))
    assert (got["lidar_slot"] == -1).all()
    # d_lidar_slot 4 bytes off a 16-byte boundary takes the word stores
    wide = torch.full((fc.MAXD + 9,), -1, dtype=torch.int32, device="cuda")
    off = 1 + (-(wide.data_ptr() // 4) % 4)
    view = wide[off:off + fc.MAXD]
    assert view.data_ptr() % 16 == 4
    compare("unaligned slot array", run_device(env, fuser, scene, lidar_slot=view), want, skip=("lidar_slot",))
    host = wide.cpu().numpy()
    assert host[off:off + fc.MAXD].tobytes() == want["lidar_slot"].tobytes() and (host[:off] == -1).all() and (host[off + fc.MAXD:] == -1).all()
    # wildly different counts on the same input and output buffers: full lists, then almost nothing, then the scene again
    buffers = upload(torch, cases["lidar1024"][0])
    for name in ("lidar1024", "camera1", "both_empty", "room_for_24", "chain64"):
        c, w = cases[name]
        for dst, src in zip(buffers, upload(torch, c)):
            dst.copy_(src)
        compare(f"same buffers: {name}", run_device(env, fuser, c, buffers=buffers), w)


def chain_frames(fusion):
    """Three sweeps of two rows of six cones, a wall and a pole, the car 0.25 m further in each; a camera with a long lens at the
    LiDAR's place looks along x and sees the ten cones from 7 m on, the two at 4 m are outside its image. The camera records are
    boxes of 0.23 m x 0.3 m around nine of the ten: one cone in the image is left to the LiDAR."""
    lidar_to_cam = (0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0)
    cam, width, height = (2000.0, 2000.0, 640.0, 360.0), 1280, 720
    frames = []
    for f in range(3):
        r = cc.two_row_scene(shift=0.25 * f)
        seen = [(x, y) for x, y in r["cones"] if x > 6.0][:-1]
        assert len(seen) == 9 and len(r["cones"]) == 12
        u = np.array([cam[2] - cam[0] * y / x for x, y in seen])
        v = np.array([cam[3] + cam[1] * (cc.gc.LIDAR_HEIGHT - 0.15) / x for x, _ in seen])
        w, h = np.array([cam[0] * 0.23 / x for x, _ in seen]), np.array([cam[1] * 0.3 / x for x, _ in seen])
        dets, _ = fc.camera(np.stack([u - w / 2, v - h / 2, u + w / 2, v + h / 2], axis=1), cls=[0 if y < 0 else 1 for _, y in seen],
                            conf=np.linspace(0.6, 0.9, 9))
        frames.append(dict(points=r["points"], m=r["m"], ground=r["params"], cluster=dict(r["cluster"], confidence=0.8, class_id=fc.UNKNOWN),
                           dets=dets, lidar_to_cam=lidar_to_cam, cam=cam, width=width, height=height,
                           locate=dict(sx=1.0, sy=1.0, shrink=0.5, min_depth=0.3, max_depth=40.0, min_valid=1),
                           fuse=dict(level_to_cam=fusion.level_to_camera(r["m"], lidar_to_cam), cam=cam, lift=0.15, min_depth=0.5, max_depth=40.0,
                                     grow=1.0, pad=4.0, range_abs=0.5, range_rel=0.1),
                           track=dict(pose=(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.25 * f), gate=0.5, alpha=0.5, birth_confidence=0.5, class_aware=1,
                                      confirm_hits=3, max_missed=2)))
    return frames


def chain_numpy(frames):
    """The twins of the five stages, frame by frame -> [(tracker state, assign, fuse result)]."""
    from unina_yolo_dla_amd import cluster, fusion, ground, localize, tracking
    state, out = tracking.new_state(), []
    for f in frames:
        kept = ground.ground_numpy(f["points"], f["m"], f["ground"])["out"]
        r = cluster.cluster_numpy(kept, f["m"], f["cluster"])
        located = localize.locate_lidar_numpy(f["dets"], len(f["dets"]), kept, f["lidar_to_cam"], f["cam"], f["width"], f["height"], f["locate"])
        fused = fusion.fuse_numpy(f["dets"], len(f["dets"]), located, r["dets"], int(r["count"][0]), r["cones"], f["fuse"])
        state, assign = tracking.update_numpy(state, fused["dets"], int(fused["count"][0]), fused["cones"], f["track"])
        out.append((state, assign, fused))
    return out


def test_the_whole_chain_on_one_stream(env):
    """Ground filter -> clusterer -> LiDAR locator on the camera records -> fuser -> ONE tracker, three frames on one stream with
    no synchronisation in between: the tracker's table and assign words after each frame equal the chain of twins, byte for
    byte. A cone both sensors see holds one track id with the camera's class, a cone outside the image one id with the
    clusterer's."""
    torch, engine, fusion = env
    from unina_yolo_dla_amd import cluster, ground, localize, tracking
    frames = chain_frames(fusion)
    want = chain_numpy(frames)
    n_max = max(len(f["points"]) for f in frames)
    filt, clus, tracker = ground.DeviceGroundFilter(n_max), cluster.DeviceClusterer(n_max), tracking.DeviceTracker()
    locators, fusers = [localize.DeviceLidarLocator(n_max, 1280, 720) for _ in frames], [fusion.DeviceFuser() for _ in frames]
    try:
        clouds = [upload_cloud(torch, f["points"], 32) for f in frames]
        det_bufs = [det_buffer(torch, f["dets"], len(f["dets"])) for f in frames]
        assigns = [torch.full((fc.MAXD,), -1, dtype=torch.int32, device="cuda") for _ in frames]
        tracker.reset()
        torch.cuda.synchronize()
        tracks_at, header_at = tracker.buffers()
        table = engine.device_view(header_at, 32 + 32 * fc.MAXD)               # the header, then the slots
        tables = []
        for k, f in enumerate(frames):
            spoil(fusers[k])
            kept = filt.filter_async(clouds[k], f["m"], f["ground"])
            ldet_buf, lcones = clus.cluster_async(kept, f["m"], f["cluster"])
            located = locators[k].update_from_buffer(det_bufs[k], kept, f["lidar_to_cam"], f["cam"], f["width"], f["height"], f["locate"])
            det_buf, cones = fusers[k].fuse_from_buffers(det_bufs[k], located, ldet_buf, lcones, f["fuse"])
            tracker.update_from_buffer(det_buf, cones, f["track"], assign=assigns[k])
            tables.append(table.clone())                                          # a copy on the same stream, not a synchronisation
        torch.cuda.synchronize()
        got = [(t.cpu().numpy(), a.cpu().numpy(), dict(zip(NAMES, fz.read()))) for t, a, fz in zip(tables, assigns, fusers)]
    finally:
        for h in (filt, clus, tracker, *locators):
            h.close()
    assert tracks_at == header_at + 32
    for k, ((table, assign, fused), (state, want_assign, want_fused)) in enumerate(zip(got, want)):
        compare(f"chain frame {k}", fused, want_fused)
        assert table[:32].tobytes() == state["header"].tobytes(), (k, table[:32].view(np.int32), state["header"])
        assert_records_equal(table[32:].view(tracking.TRACK_DTYPE), state["tracks"], f"chain frame {k}", "slot")
        assert assign.tobytes() == want_assign.tobytes(), k
    # what the chain is for: one id per cone over the three frames
    heads = [fz["header"][0] for _, _, fz in got]
    assert all((h["n_camera"], h["n_matched"], h["n_lidar_only"], h["n_written"]) == (9, 9, 3, 12) for h in heads), heads
    ids = np.stack([a[:12] for _, a, _ in got])
    assert (ids[:, :9] == ids[0, :9]).all() and len(set(ids[0, :9].tolist())) == 9 and (ids[0, :9] > 0).all()     # camera slot i is record i in every frame
    lidar_ids = [sorted(a[9:12].tolist()) for _, a, _ in got]
    assert lidar_ids[0] == lidar_ids[1] == lidar_ids[2] and all(v > 0 for v in lidar_ids[0]) and not set(lidar_ids[0]) & set(ids[0, :9].tolist())
    tracks = got[2][0][32:].view(tracking.TRACK_DTYPE)
    live = tracks[tracks["id"] != 0]
    assert len(live) == 12 and (live["hits"] == 3).all()
    by_id = {int(t["id"]): int(t["class_id"]) for t in live}
    assert [by_id[i] for i in ids[0, :9].tolist()] == frames[0]["dets"]["class_id"].tolist() and {0, 1} == set(frames[0]["dets"]["class_id"].tolist())
    assert [by_id[i] for i in lidar_ids[0]] == [fc.UNKNOWN] * 3
    outside = [int(a[9 + k]) for (_, a, fz) in got[:1] for k in range(3) if fz["dets"]["x1"][9 + k] < 0 or fz["dets"]["x1"][9 + k] >= 1280]
    assert len(outside) == 2                                                     # the two cones at 4 m project beside the image
