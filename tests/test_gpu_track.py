"""csrc/track.hip on the GPU through unina_track_*: every comparison is BYTE equality with tracking.update_numpy of the 1024-slot
table, the header and the 1024 assign words, after EVERY update of every sequence (integers, and fp32 values with a fixed
operation order: no tolerance). What each constructed case contains is asserted on the twin in tests/test_track_cpu.py; the
record and cone buffers carry NaN bit patterns behind the records, the assign buffer -1 before each launch."""
import numpy as np
import pytest

import track_cases as tc
from records import assert_records_equal, det_buffer, padded_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import engine, tracking
    return torch, engine, tracking


@pytest.fixture(scope="module")
def tracker(env):
    t = env[2].DeviceTracker()
    yield t
    t.close()


def upload(torch, f):
    """(Engine.infer_async's int32 buffer, the cone records) of one frame on the device, garbage behind the records."""
    return det_buffer(torch, f["dets"], f["count"]), torch.from_numpy(padded_words(f["cones"], 8 * tc.MAXD)).cuda()


def run_device(env, tracker, c, stream=None, frames=None):
    """The case from a reset table; [(header, tracks, assign)] read back after every update."""
    torch = env[0]
    out = []
    tracker.reset(stream)
    for f in (c["frames"] if frames is None else frames):
        buf, cones = upload(torch, f)
        torch.cuda.synchronize()
        if stream is None:
            tracker.assign.fill_(-1)
            tracker.update_from_buffer(buf, cones, f["params"])
        else:
            with torch.cuda.stream(stream):
                tracker.assign.fill_(-1)
                tracker.update_from_buffer(buf, cones, f["params"], stream=stream)
        header, tracks = tracker.read(stream)                 # synchronises the stream
        out.append((header, tracks, tracker.assign.cpu().numpy()))
    return out


def compare(name, got, want):
    assert len(got) == len(want)
    for k, ((header, tracks, assign), (state, want_assign)) in enumerate(zip(got, want)):
        where = f"{name} frame {k}"
        assert header.tobytes() == state["header"].tobytes(), (where, header, state["header"])
        assert_records_equal(tracks, state["tracks"], where, "slot")
        if assign.tobytes() != want_assign.tobytes():
            bad = np.nonzero(assign != want_assign)[0]
            raise AssertionError(f"{where}: {len(bad)} assign words differ, first {bad[0]}: got {assign[bad[0]]}, want {want_assign[bad[0]]}")


def test_edge_cases_equal_the_twin(env, tracker):
    """Counts 0 / 1 / 63 / 64 / 65 / 1024 / 5000 (clamped) / negative; all cones invalid; NaN and inf coordinates and a pose that
    overflows; a NaN confidence; an empty table; a full table with 1024 gated records and with births that are dropped; a death
    and a birth that reuse a slot; max_missed = 0; alpha 1 and 0.25; a distance equal to gate * gate and one ulp above; two
    classes at one position, class-aware and class-blind; grid ties; one record between two slots and two records around one;
    the 64-round chain, also across a wave boundary."""
    cases = tc.cached("edges", tc.edge_cases)
    assert len(cases) == 27
    for c, want in cases:
        compare(c["name"], run_device(env, tracker, c), want)


@pytest.mark.parametrize("class_aware", (1, 0), ids=["class_aware", "class_blind"])
def test_world_sequence_equals_the_twin_on_every_frame(env, tracker, class_aware):
    """40 frames of 150 cones from a moving, rotating pose: 2 cm noise, 15 % dropouts, 10 false positives per frame."""
    (c, want), = tc.cached(f"world{class_aware}", lambda: tc.world_sequence(class_aware))
    compare(c["name"], run_device(env, tracker, c), want)
    h = [s["header"][0] for s, _ in want]
    assert sum(x["n_matched"] for x in h) > 1500 and sum(x["n_born"] for x in h) > 300 and sum(x["n_died"] for x in h) > 200
    assert h[-1]["n_confirmed"] > 50


def test_repeats_side_stream_and_reset_give_the_same_bytes(env, tracker):
    torch, _, tracking = env
    (c, want), = tc.cached("world1", lambda: tc.world_sequence(1))
    frames, want = c["frames"][:12], want[:12]
    a = run_device(env, tracker, c, frames=frames)
    b = run_device(env, tracker, c, frames=frames)                     # the reset in front of it restarts the ids at 1
    for (ha, ta, aa), (hb, tb, ab) in zip(a, b):
        assert ha.tobytes() == hb.tobytes() and ta.tobytes() == tb.tobytes() and aa.tobytes() == ab.tobytes()
    compare("repeat", b, want)
    s = torch.cuda.Stream()
    other = tracking.DeviceTracker()                                   # its first call, on the side stream, allocates and resets
    try:
        compare("side stream", run_device(env, other, c, stream=s, frames=frames), want)
        tracks, header = other.buffers()
        assert tracks and header and tracks == header + 32
    finally:
        other.close()
    # a reset in the middle of a sequence: five frames, reset, the sequence again from its start
    run_device(env, tracker, c, frames=frames[:5])
    again = run_device(env, tracker, c, frames=frames[:5])
    compare("after reset", again, want[:5])
    assert again[0][0]["next_id"][0] == 1 + again[0][0]["n_born"][0] and again[0][1]["id"].max() == again[0][0]["n_born"][0]


def test_assign_unaligned_and_absent(env, tracker):
    """d_assign 4 bytes off a 16-byte boundary takes the word stores, NULL writes nothing; the table is the same."""
    torch = env[0]
    c, want = next(x for x in tc.cached("edges", tc.edge_cases) if x[0]["name"] == "count65")
    wide = torch.full((tc.MAXD + 9,), -1, dtype=torch.int32, device="cuda")
    tracker.reset()
    for k, f in enumerate(c["frames"]):
        buf, cones = upload(torch, f)
        wide.fill_(-1)
        off = 1 + (-(wide.data_ptr() // 4) % 4)                        # word offset that is 4 bytes past a 16-byte boundary
        view = wide[off:off + tc.MAXD]
        assert view.data_ptr() % 16 == 4
        tracker.update_from_buffer(buf, cones, f["params"], assign=view if k != 1 else False)
        header, tracks = tracker.read()
        host = wide.cpu().numpy()
        assert header.tobytes() == want[k][0]["header"].tobytes() and tracks.tobytes() == want[k][0]["tracks"].tobytes()
        if k == 1:
            assert (host == -1).all()
        else:
            assert host[off:off + tc.MAXD].tobytes() == want[k][1].tobytes()
            assert (host[:off] == -1).all() and (host[off + tc.MAXD:] == -1).all()


def test_ids_stop_at_int_max(env, tracker):
    """next_id two below INT_MAX, written into the device header through unina_track_buffers: of five births two are taken and
    three dropped, and the counter stays at INT_MAX afterwards."""
    torch, engine, tracking = env
    int_max = 2 ** 31 - 1

    tracker.reset()
    torch.cuda.synchronize()
    engine.device_view(tracker.buffers()[1], 8, "<i4")[3] = int_max - 2      # the device header as a tensor
    state = tracking.new_state()
    state["header"]["next_id"] = int_max - 2
    for f in (tc.frame(tc.grid(5)), tc.frame(tc.grid(8) + np.float32(0.01))):
        buf, cones = upload(torch, f)
        tracker.assign.fill_(-1)
        tracker.update_from_buffer(buf, cones, f["params"])
        header, tracks = tracker.read()
        state, want_assign = tracking.update_numpy(state, f["dets"], f["count"], f["cones"], f["params"])
        assert header.tobytes() == state["header"].tobytes() and tracks.tobytes() == state["tracks"].tobytes()
        assert tracker.assign.cpu().numpy().tobytes() == want_assign.tobytes()
    assert state["header"]["next_id"][0] == int_max and state["header"]["n_dropped"][0] == 6 and state["header"]["n_live"][0] == 2


def test_behind_locate_on_one_stream(env, tracker, pkg, sd7):
    """The node's call order on the 64 x 64 engine: infer_letterbox_frame, unina_locate_async, unina_track_update_async for three
    frames on one stream, nothing touching the host in between; the twin is fed with the records and cones read back afterwards."""
    import locate_cases as lc
    from unina_yolo_dla_amd import localize
    torch, engine, tracking = env
    g = pkg.graph.Graph(in_h=64, in_w=64)
    eng = engine.Engine.from_state_dict(sd7, g, device=0)
    locators = [localize.DeviceLocator() for _ in range(3)]
    try:
        w, h = 96, 72
        rng = np.random.RandomState(5)
        d_bgra = torch.from_numpy(rng.randint(0, 256, (h, 4 * w)).astype(np.uint8)).cuda()
        frame = engine.Frame.from_tensors(engine.FMT_BGRA, w, h, d_bgra, 4 * w)
        depth = lc.depth_map(9, engine.DEPTH_F32, h, w)
        plane = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
        cam, par = (80.0, 80.0, 47.5, 35.5), lc.params(shrink=0.5, max_side=16)
        outs = [torch.full((tc.MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
        assigns = [torch.full((tc.MAXD,), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
        poses = [tc.params(pose=[1, 0, 0, 0.05 * k, 0, 1, 0, -0.03 * k, 0, 0, 1, 0], gate=0.5, alpha=0.5, birth_confidence=0.05,
                           confirm_hits=2, max_missed=1) for k in range(3)]
        tracker.reset()
        torch.cuda.synchronize()
        for k in range(3):
            eng.infer_letterbox_frame(frame, None, 0.05, 0.45, 0.1, 114.0, True, out=outs[k])
            locators[k].update_from_buffer(outs[k], plane, 1.0, cam, par)
            tracker.update_from_buffer(outs[k], locators[k].out, poses[k], assign=assigns[k])
        header, tracks = tracker.read()
        dets = [engine.Engine.unpack(o) for o in outs]
        cones = [loc.read() for loc in locators]
        got_assign = [a.cpu().numpy() for a in assigns]
    finally:
        eng.close()
    state = tracking.new_state()
    for k in range(3):
        assert len(dets[k]) > 0
        state, want_assign = tracking.update_numpy(state, dets[k], len(dets[k]), cones[k], poses[k])
        assert got_assign[k].tobytes() == want_assign.tobytes(), k
        assert k == 0 or state["header"]["n_matched"][0] > 0
    assert header.tobytes() == state["header"].tobytes() and tracks.tobytes() == state["tracks"].tobytes()
    assert state["header"]["n_confirmed"][0] > 0
    print(f"{len(dets[0])} records, {state['header'][0]}")
