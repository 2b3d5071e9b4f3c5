"""csrc/pose.hip on the GPU through unina_pose_async: every comparison is BYTE equality with pose.pose_numpy -- of the header, of the
result and of all 1024 out cones (integers, and fp32 / float64 values with a fixed operation order: no tolerance; only the sign and
payload of a NaN coordinate that an operation produced are the processor's, pose_cases.canon_cones). What each constructed case
contains is asserted on the twin in tests/test_pose_cpu.py; the record and cone buffers carry NaN bit patterns behind the records,
every output byte is 0xFF before each launch."""
import numpy as np
import pytest

import pose_cases as pc
import track_cases as tc
from records import assert_records_equal, det_buffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import engine, pose
    return torch, engine, pose


@pytest.fixture(scope="module")
def est(env):
    return env[2].DevicePoseEstimator(None)


def words(torch, records):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.int32).reshape(-1).copy()).cuda()


def upload(torch, c):
    """(Engine.infer_async's int32 buffer, the cones, the slots, the earlier result or None) of a case on the device."""
    return (det_buffer(torch, c["dets"], c["count"]), words(torch, c["cones"]), words(torch, c["tracks"]),
            None if c["prev"] is None else words(torch, c["prev"]))


def run_device(env, est, c, in_place=False, over_prev=False, stream=None):
    """One call -> header, result, out cones and the input cones buffer afterwards. over_prev: d_result == d_prev."""
    torch, engine, _ = env
    buf, cones, tracks, prev = upload(torch, c)
    est.tracks = tracks

    def go():
        for t in (est.cones, est.header, est.result):
            t.fill_(0xFF)
        if prev is None:
            est.estimate_from_buffer(buf, cones, c["params"], in_place=in_place, stream=stream)
        elif over_prev:
            est.result.copy_(prev.view(torch.uint8))
            est.estimate_from_buffer(buf, cones, c["params"], chain=True, in_place=in_place, stream=stream)
        else:
            est.estimate_async(*engine.det_buffer_ptrs(buf), cones, c["params"], in_place=in_place, stream=stream, prev=prev)
    torch.cuda.synchronize()
    if stream is None:
        go()
    else:
        with torch.cuda.stream(stream):
            go()
    header, result, out = est.read(stream)
    return {"header": header, "result": result, "cones": out, "input": cones.cpu().numpy().view(out.dtype)}


def compare(name, got, want):
    assert got["header"].tobytes() == want["header"].tobytes(), (name, got["header"], want["header"])
    assert got["result"].tobytes() == want["result"].tobytes(), (name, got["result"], want["result"], got["header"])
    assert_records_equal(pc.canon_cones(got["cones"]), pc.canon_cones(want["cones"]), name, "cone")


def test_edge_cases_equal_the_twin(env, est):
    """An empty table and count = 0, counts of 1025 and -1; exactly min_pairs pairs and one fewer; TOO_FEW reached at iteration 2;
    two pairs at one point (DEGENERATE, the translation taken); half a turn; two records nearest to one landmark; equal d2 towards
    two landmarks and from two records; d2 on the gate and one ulp beyond; class-aware and class-blind; slots one hit short; NaN
    and inf cones and landmarks, valid = 0; a point and a landmark at 32768 m and just beyond; 1024 x 1024 pairs of one class at
    +-32768 m; an earlier result in front of the increment. Out of place: the input cones stay as they were."""
    cases = pc.edge_results()
    assert len(cases) == 28
    for c, want in cases:
        got = run_device(env, est, c)
        compare(c["name"], got, want)
        assert got["input"].tobytes() == c["cones"].tobytes(), c["name"]


def test_in_place_and_result_over_prev_give_the_same_bytes(env, est):
    cases = {c["name"]: (c, want) for c, want in pc.edge_results()}
    for name in ("plain", "plain_prev", "count1025", "non_finite_and_invalid", "too_few_at_iteration_2", "fixed_point_edge", "empty_count0"):
        c, want = cases[name]
        got = run_device(env, est, c, in_place=True)
        compare(name + " in place", got, want)
        assert got["input"].tobytes() == got["cones"].tobytes()
    c, want = cases["plain_prev"]
    compare("result over prev", run_device(env, est, c, over_prev=True), want)
    compare("result over prev, in place", run_device(env, est, c, in_place=True, over_prev=True), want)


def test_repeats_side_stream_and_permuted_records_give_the_same_bytes(env, est):
    torch = env[0]
    cases = {c["name"]: (c, want) for c, want in pc.edge_results()}
    for name in ("plain_prev", "fixed_point_edge"):
        c, want = cases[name]
        a, b = run_device(env, est, c), run_device(env, est, c)
        for what in ("header", "result", "cones"):
            assert a[what].tobytes() == b[what].tobytes(), (name, what)
        compare(name + " side stream", run_device(env, est, c, stream=torch.cuda.Stream()), want)
    # another order of the records of a call without ties: the same result and header, the out cones in the new order
    c, want = cases["plain_prev"]
    p, order = pc.permuted(c)
    want_p = pc.run_twin(p)
    assert want_p["header"].tobytes() == want["header"].tobytes() and want_p["result"].tobytes() == want["result"].tobytes()
    got = run_device(env, est, p)
    compare("permuted", got, want_p)
    assert got["cones"][:len(order)].tobytes() == want["cones"][order].tobytes()


def test_misaligned_and_overlapping_pointers_are_refused(env, est):
    """Real device buffers, 4 or 8 bytes off a 16-byte boundary or overlapping their input: UNINA_ERR_ARG, and nothing is written."""
    torch, engine, pose = env
    c = pc.edge_results()[5][0]
    assert c["name"] == "plain"
    buf, cones, tracks, _ = upload(torch, c)
    wide = torch.full((16 * pc.MAXD,), -1, dtype=torch.int32, device="cuda")
    dets, count = engine.det_buffer_ptrs(buf)
    L, par = est.L, pose.as_params(c["params"])
    import ctypes as C
    assert wide.data_ptr() % 16 == 0
    good = dict(dets=dets, count=count, cones=cones.data_ptr(), tracks=tracks.data_ptr(), prev=wide.data_ptr() + 48000, out=wide.data_ptr(),
                res=wide.data_ptr() + 40000, hdr=wide.data_ptr() + 40064)
    for key, off in (("tracks", 4), ("tracks", 8), ("prev", 8), ("out", 4), ("out", 8), ("res", 4), ("res", 8), ("hdr", 8), ("cones", 8), ("dets", 8),
                     ("count", 2)):
        a = dict(good)
        a[key] += off
        rc = L.unina_pose_async(a["dets"], a["count"], a["cones"], a["tracks"], a["prev"], C.byref(par), a["out"], a["res"], a["hdr"], None)
        assert rc == 4, (key, off)
    assert L.unina_pose_async(dets, count, cones.data_ptr(), tracks.data_ptr(), None, C.byref(par), cones.data_ptr() + 32, good["res"], good["hdr"],
                              None) == 4
    torch.cuda.synchronize()
    assert (wide.cpu().numpy() == -1).all() and cones.cpu().numpy().tobytes() == c["cones"].tobytes()
    with pytest.raises(engine.EngineError):
        est.tracks = tracks[1:]
        est.estimate_from_buffer(buf, cones, c["params"])


def test_the_chain_on_the_device_equals_the_twin_chain_on_every_frame(env):
    """40 frames of the world sequence with the biased odometry on one stream, nothing synchronised in between: pose (the earlier
    result chained, d_result == d_prev, the cones in place) -> tracker with the identity. Per frame the result, the header, the
    table and the assign words equal the chain of twins."""
    torch, engine, pose = env
    from unina_yolo_dla_amd import tracking
    seed = 5
    frames, truth, incs = pc.world_chain_inputs(seed)
    want = pc.chain_results(seed)
    tracker = tracking.DeviceTracker()
    try:
        tracker.reset()
        torch.cuda.synchronize()
        tracks_at, header_at = tracker.buffers()
        table = engine.device_view(header_at, 32 + 32 * pc.MAXD)
        est = pose.DevicePoseEstimator.from_tracker(tracker)
        bufs, cones = [], []
        for f in frames:
            dets, cn = pc.padded_frame(f)
            bufs.append(det_buffer(torch, dets, f["count"]))
            cones.append(words(torch, cn))
        assigns = [torch.full((pc.MAXD,), -1, dtype=torch.int32, device="cuda") for _ in frames]
        torch.cuda.synchronize()
        snaps = []
        for k, f in enumerate(frames):
            moved = est.estimate_from_buffer(bufs[k], cones[k], dict(pc.POSE_PAR, inc=incs[k]), chain=k > 0, in_place=True)
            tracker.update_from_buffer(bufs[k], moved, dict(f["params"], pose=None), assign=assigns[k])
            snaps.append((est.result.clone(), est.header.clone(), table.clone()))          # copies on the same stream, no synchronisation
        torch.cuda.synchronize()
        got = [(r.cpu().numpy(), h.cpu().numpy(), t.cpu().numpy(), a.cpu().numpy(), c.cpu().numpy()) for (r, h, t), a, c in zip(snaps, assigns, cones)]
    finally:
        tracker.close()
    assert tracks_at == header_at + 32
    for k, ((result, header, tab, assign, moved), (r, state, want_assign, _)) in enumerate(zip(got, want)):
        where = f"chain frame {k}"
        assert header.tobytes() == r["header"].tobytes(), (where, header.view(np.int32), r["header"])
        assert result.tobytes() == r["result"].tobytes(), (where, result.view(np.float32), r["result"])
        assert_records_equal(pc.canon_cones(moved.view(r["cones"].dtype)), pc.canon_cones(r["cones"]), where, "cone")
        assert tab[:32].tobytes() == state["header"].tobytes(), (where, tab[:32].view(np.int32), state["header"])
        assert_records_equal(tab[32:].view(tracking.TRACK_DTYPE), state["tracks"], where, "slot")
        assert assign.tobytes() == want_assign.tobytes(), where
    dt, dyaw = pc.pose_error(got[-1][0].view(np.float32)[:12], truth[-1])
    print(f"device chain, seed {seed}: final pose error {dt:.4f} m, {dyaw:.5f} rad")
    assert dt <= 0.25 and dyaw <= 0.02
