"""csrc/colour.hip on the GPU through unina_colour_async: every comparison is BYTE equality with colour.colour_numpy -- of the
header, of all 1024 records and of all 1024 colour entries (integers behind a window of fp32 values with a fixed operation order:
no tolerance). What each constructed case contains is asserted on the twin in tests/test_colour_cpu.py; the record buffers carry
NaN bit patterns behind the records, an image lies in a buffer of exactly its size at the case's offset and pitch, every output
byte is 0xFF before each launch. Images are at most 256 x 192."""
import numpy as np
import pytest

import colour_cases as cc
import fuse_cases as fc
from records import assert_records_equal, det_buffer, padded_words

pytestmark = pytest.mark.gpu

NAMES = ("header", "dets", "colours")


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import colour, engine
    return torch, engine, colour


@pytest.fixture(scope="module")
def clf(env):
    return env[2].DeviceColourClassifier()


def upload_image(torch, c):
    """The case's image on the device as the [H, W, C] view of a buffer of exactly its bytes: the row stride is the case's pitch,
    the first pixel lies `offset` bytes into the allocation."""
    h, w, ch = c["image"].shape
    buf = torch.from_numpy(cc.image_bytes(c)).cuda()
    return torch.as_strided(buf, (h, w, ch), (c["pitch"], ch, 1), c["offset"])


def upload(torch, c):
    cones = None if c["cones"] is None else torch.from_numpy(padded_words(c["cones"], 8 * cc.MAXD)).cuda()
    return det_buffer(torch, c["dets"], c["count"]), cones, upload_image(torch, c)


def spoil(clf):
    clf.det_buf.fill_(-1)
    clf.colours.fill_(0xFF)
    clf.header.fill_(0xFF)


def run_device(env, clf, c, stream=None, in_place=False, buffers=None):
    torch = env[0]
    det_buf, cones, image = upload(torch, c) if buffers is None else buffers
    torch.cuda.synchronize()
    if stream is None:
        spoil(clf)
        out = clf.classify_from_buffers(det_buf, cones, image, c["cam"], c["params"], in_place=in_place)
    else:
        with torch.cuda.stream(stream):
            spoil(clf)
            out = clf.classify_from_buffers(det_buf, cones, image, c["cam"], c["params"], stream=stream, in_place=in_place)
    assert (out is det_buf) == in_place
    got = dict(zip(NAMES, clf.read(stream)))
    got["count"] = int(out[:1].cpu()[0])
    return got


def compare(name, got, want):
    for what in NAMES:
        assert_records_equal(got[what], want[what], f"{name}: header {got['header']}", what)


def test_constructed_cases_equal_the_twin(env, clf):
    """Counts 0 / 1 / 63 / 64 / 65 / 1024 / 5000 (clamped) / negative; windows of 1 x 1, 1 x 64, 64 x 1, 64 x 64 at strides 1, 4 x 3
    and (max_side = 48) 5, clipped at each border, wholly outside, NaN, inf and inverted boxes, point boxes with a valid cone, an
    invalid one, z <= 0, non-finite u, v or z, half extents that overflow, and without the cones array; a 1 x 1 image; 3 and 4
    channels in both orders at odd pitches and addresses, a 3-channel image whose last pixel ends the buffer; every pixel class
    on and off its bound, the six hue branches, each hue bound and one off, a range across 0 and overlapping ranges; tapers 0, 64
    and 256 with cols = 1 and rows = 1; the decision on and one vote off each bound, equal votes, no coloured pixel, class_of
    entries of -1; the row strings; and the selection. Disjoint outputs here, in place in the next test."""
    cases = cc.cached("edges", cc.edge_cases)
    assert len(cases) == 44
    for c, want in cases:
        got = run_device(env, clf, c)
        compare(c["name"], got, want)
        assert got["count"] == c["count"], c["name"]                  # the count word travels with the records


def test_in_place_equals_the_twin(env, clf):
    """d_out_dets == d_dets: a workgroup reads and writes its own record only. The slots behind the count are zeroed in the
    caller's buffer too."""
    cases = dict((c["name"], (c, want)) for c, want in cc.cached("edges", cc.edge_cases))
    for name in ("count65", "count1024", "count5000", "count-7", "windows", "stripes", "only_unknown", "scene_c4_o0_odd"):
        c, want = cases[name]
        compare(f"in place: {name}", run_device(env, clf, c, in_place=True), want)


def test_rendered_cones_equal_the_twin(env, clf):
    for c, want in cc.cached("rendered", cc.rendered_cases):
        compare(c["name"], run_device(env, clf, c), want)
        assert want["header"]["n_decided"][0] == 16


def test_repeats_side_stream_and_other_images_give_the_same_bytes(env, clf):
    torch = env[0]
    cases = dict((c["name"], (c, want)) for c, want in cc.cached("edges", cc.edge_cases))
    c, want = cases["windows"]
    a = run_device(env, clf, c)
    b = run_device(env, clf, c)
    for what in NAMES:
        assert a[what].tobytes() == b[what].tobytes(), what
    compare("repeat", b, want)
    side = torch.cuda.Stream()
    compare("side stream", run_device(env, clf, c, stream=side), want)
    compare("side stream, in place", run_device(env, clf, c, stream=side, in_place=True), want)
    # one classifier through images of other sizes and channel counts, and back
    for name in ("image_1x1", "scene_c4_o1", "pixels_c3_o0", "scene_c3_width_253", "stripes", "count1024", "windows"):
        c, w = cases[name]
        compare(f"same classifier: {name}", run_device(env, clf, c), w)


# ---------------------------------------------------------------- the chain: fuser -> colour (in place) -> tracker
CHAIN_PIXELS = ((100.0, 80.0), (180.0, 120.0))     # a blue cone the camera sees in frame 0 only, a yellow one it never sees


def chain_frames():
    """Two cones 4 m in front of fuse_cases' placed camera, painted on a 256 x 192 image where they project. Frame 0: the camera
    reports the blue one (a box, class 1, with a depth); the clusterer reports both, class UNKNOWN. Frame 1: the camera reports
    nothing. The SIZE window at 4 m is 15 x 21 pixels around the represented point."""
    img = np.empty((192, 256, 3), dtype=np.int64)
    img[:] = cc.BACKGROUNDS["asphalt"]
    for (u, v), kind in zip(CHAIN_PIXELS, ("blue", "yellow")):
        cc.render_cone(img, int(u) - 7, int(v) - 11, 15, 21, kind)
    img = np.clip(img + np.random.default_rng(2).integers(-12, 13, img.shape), 0, 255).astype(np.uint8)
    pts = fc.pixels_to_points([p[0] for p in CHAIN_PIXELS], [p[1] for p in CHAIN_PIXELS])
    (u, v), frames = CHAIN_PIXELS[0], []
    for f in range(2):
        boxes = np.array([[u - 8, v - 12, u + 8, v + 10]]) if f == 0 else np.zeros((0, 4))
        frames.append(dict(camera=fc.camera(boxes, depth=np.full(len(boxes), 4.0), cls=1), lidar=fc.lidar(pts, cls=cc.UNKNOWN, conf=0.5)))
    fuse = fc.params(pad=2.0)
    colour = cc.params(only_class=cc.UNKNOWN)
    track = dict(gate=0.5, alpha=0.5, birth_confidence=0.25, class_aware=1, confirm_hits=1, max_missed=3)
    return img, frames, fuse, colour, track


def chain_numpy(img, frames, fuse, colour_par, track, with_colour=True):
    from unina_yolo_dla_amd import colour, fusion, tracking
    state, out = tracking.new_state(), []
    for f in frames:
        (dets, cones), (ldets, lcones) = f["camera"], f["lidar"]
        fused = fusion.fuse_numpy(dets, len(dets), cones, ldets, len(ldets), lcones, fuse)
        named = colour.colour_numpy(fused["dets"], int(fused["count"][0]), fused["cones"], img, fc.CAM, colour_par) if with_colour else None
        state, assign = tracking.update_numpy(state, named["dets"] if with_colour else fused["dets"], int(fused["count"][0]), fused["cones"], track)
        out.append((state, assign, named))
    return out


def test_the_chain_names_a_lidar_only_cone_and_joins_its_coloured_track(env):
    """Clusterer-style records -> DeviceFuser -> DeviceColourClassifier in place -> DeviceTracker with class_aware = 1, two frames
    on one side stream with no synchronisation in between, against the numpy twins chained the same way. The cone the camera
    saw in frame 0 is LiDAR-only in frame 1: named blue from its pixels it joins the track the camera record founded; without
    the stage it founds a second track."""
    torch, engine, colour = env
    from unina_yolo_dla_amd import fusion, tracking
    img, frames, fuse, colour_par, track = chain_frames()
    want = chain_numpy(img, frames, fuse, colour_par, track)
    without = chain_numpy(img, frames, fuse, colour_par, track, with_colour=False)
    tracker, fusers, clfs = tracking.DeviceTracker(), [fusion.DeviceFuser() for _ in frames], [colour.DeviceColourClassifier() for _ in frames]
    try:
        image = torch.from_numpy(img).cuda()
        cone_words = lambda a: torch.from_numpy(padded_words(a, 8 * cc.MAXD)).cuda()      # noqa: E731
        bufs = [(det_buffer(torch, f["camera"][0], len(f["camera"][0])), cone_words(f["camera"][1]), det_buffer(torch, f["lidar"][0], len(f["lidar"][0])),
                 cone_words(f["lidar"][1])) for f in frames]
        assigns = [torch.full((cc.MAXD,), -1, dtype=torch.int32, device="cuda") for _ in frames]
        tracker.reset()
        torch.cuda.synchronize()
        tracks_at, header_at = tracker.buffers()
        table = engine.device_view(header_at, 32 + 32 * cc.MAXD)
        side, tables = torch.cuda.Stream(), []
        with torch.cuda.stream(side):
            for k in range(len(frames)):
                spoil(clfs[k])
                det_buf, cones = fusers[k].fuse_from_buffers(*bufs[k], fuse, stream=side)
                named = clfs[k].classify_from_buffers(det_buf, cones, image, fc.CAM, colour_par, stream=side, in_place=True)
                assert named is det_buf
                tracker.update_from_buffer(named, cones, track, stream=side, assign=assigns[k])
                tables.append(table.clone())                                      # a copy on the same stream, not a synchronisation
        side.synchronize()
        got = [(t.cpu().numpy(), a.cpu().numpy(), dict(zip(NAMES, c.read(side)))) for t, a, c in zip(tables, assigns, clfs)]
    finally:
        tracker.close()
    assert tracks_at == header_at + 32
    for k, ((tab, assign, named), (state, want_assign, want_named)) in enumerate(zip(got, want)):
        compare(f"chain frame {k}", named, want_named)
        assert tab[:32].tobytes() == state["header"].tobytes(), (k, tab[:32].view(np.int32), state["header"])
        assert_records_equal(tab[32:].view(tracking.TRACK_DTYPE), state["tracks"], f"chain frame {k}", "slot")
        assert assign.tobytes() == want_assign.tobytes(), k
    # what the stage is for, on the twin the device equals: frame 0 the camera's blue record and the LiDAR-only yellow cone, frame 1
    # two LiDAR-only cones named from their pixels, the blue one on the camera's track
    named0, named1 = want[0][2], want[1][2]
    assert named0["dets"]["class_id"][:2].tolist() == [1, 0] and named0["header"]["n_selected"][0] == 1
    assert named1["dets"]["class_id"][:2].tolist() == [1, 0] and named1["header"]["n_decided"][0] == 2
    assert (named1["colours"]["status"][:2] & 16 != 0).all() and (named1["colours"]["n_stripes"][:2] == 1).all()
    ids0, ids1 = want[0][1][:2].tolist(), want[1][1][:2].tolist()
    assert ids0 == ids1 and 0 not in ids0 and want[1][0]["header"]["n_live"][0] == 2 and want[1][0]["header"]["n_born"][0] == 0
    live = want[1][0]["tracks"][want[1][0]["tracks"]["id"] != 0]
    assert sorted(live["class_id"].tolist()) == [0, 1] and (live["hits"] == 2).all()
    # without the stage the unknown record cannot join the blue track: a second track for the same cone
    assert without[1][0]["header"]["n_live"][0] == 3 and without[1][0]["header"]["n_born"][0] == 1
    assert without[1][1][0] != without[0][1][0]
