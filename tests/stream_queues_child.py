"""Child of tests/test_gpu_stream_queues.py: ONE case per process, on the 64x64 graph.

Which hardware queue a stream lands on depends on every stream the process made before it (the runtime hands out a fresh
queue while there is one, then the least-referenced), so a case is only meaningful in a process that holds nothing but what the
case itself creates -- not in the pytest process, with the streams of dozens of earlier tests. GPU_MAX_HW_QUEUES is inherited
from the command, never set here.

    python stream_queues_child.py handles_first | streams_first | plan_change | failed_capture

Prints one JSON line with what it measured (before the parent asserts on it)."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

CONF = 0.05          # keeps a few dozen detections of the seeded synthetic heads at 64x64 (the smoke run's threshold)
REPS = 3


def _engine_file(u):
    from unina_yolo_dla_amd import export
    g = u.graph.Graph(in_h=64, in_w=64)
    sd = u.synth.make_state_dict(7, g)
    fd, path = tempfile.mkstemp(suffix=".une")
    os.close(fd)
    export.export_engine(sd, path, g, export.FP16, None)
    return path


def two_frames(handles_first: bool):
    """Two handles and two torch streams, in bench.py's order or the other one; one frame per handle on its own stream (which
    captures both graphs); then the count of library streams and the probe on (stream 0, stream 1) and (stream 0, stream 0)."""
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine as E
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    path = _engine_file(u)
    try:
        if handles_first:
            engines = [E.Engine(path, device=0) for _ in range(2)]
            streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        else:
            streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
            engines = [E.Engine(path, device=0) for _ in range(2)]
    finally:
        os.unlink(path)
    owned = [E.owned_streams()]
    frames = [torch.from_numpy(u.rng.frame(1234 + k, 64, 64)).to(dev) for k in range(2)]
    outs = [torch.zeros((8 + 8 * E.MAX_DETECTIONS,), dtype=torch.int32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            engines[k].infer_async(frames[k], CONF, 0.45, 0.1, out=outs[k], stream=streams[k])
        owned.append(E.owned_streams())
    torch.cuda.synchronize()
    counts = [int(o[0].item()) for o in outs]
    pair, pair_stamps = E.streams_overlap(streams[0], streams[1], REPS)
    same, same_stamps = E.streams_overlap(streams[0], streams[0], REPS)
    owned.append(E.owned_streams())
    for e in engines:
        e.close()
    return {"owned": owned, "detections": counts, "reps": REPS, "overlap_s0_s1": pair, "overlap_s0_s0": same,
            "stamps_s0_s1": pair_stamps.tolist(), "stamps_s0_s0": same_stamps.tolist(),
            "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES")}


def plan_change():
    """One handle through two plan changes (each drops the graph: the next call captures again) beside handles that never
    switched: one loaded as usual, one loaded with fusion off from the start."""
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine as E
    torch.cuda.set_device(0)
    path = _engine_file(u)
    try:
        e = E.Engine(path, device=0)
        steady_on = E.Engine(path, device=0)
        os.environ["UNINA_FUSE"] = "0"
        try:
            steady_off = E.Engine(path, device=0)
        finally:
            del os.environ["UNINA_FUSE"]
    finally:
        os.unlink(path)
    x = torch.from_numpy(u.rng.frame(1234, 64, 64)).cuda()
    torch.cuda.synchronize()
    owned, got = [E.owned_streams()], []
    groups = [e.L.unina_fusion_groups(e.h)]
    for fuse in (None, False, True):
        if fuse is not None:
            groups.append(e.set_fusion(fuse))
        got.append(e.infer(x, CONF, 0.45, 0.1))
        owned.append(E.owned_streams())
    want_on = steady_on.infer(x, CONF, 0.45, 0.1)
    want_off = steady_off.infer(x, CONF, 0.45, 0.1)
    owned.append(E.owned_streams())
    res = {"owned": owned, "groups": groups, "steady_groups": [steady_on.L.unina_fusion_groups(steady_on.h), steady_off.L.unina_fusion_groups(steady_off.h)],
           "detections": [len(d) for d in got], "steady_detections": [len(want_on), len(want_off)],
           "same_bytes": [got[0].tobytes() == want_on.tobytes(), got[1].tobytes() == want_off.tobytes(), got[2].tobytes() == want_on.tobytes()],
           "unfused_equals_fused": got[1].tobytes() == want_on.tobytes()}
    for h in (e, steady_on, steady_off):
        h.close()
    return res


def failed_capture():
    """A first call that fails (no 'images' tensor bound), then the same handle used properly."""
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine as E
    torch.cuda.set_device(0)
    path = _engine_file(u)
    try:
        e = E.Engine(path, device=0)
        steady = E.Engine(path, device=0)
    finally:
        os.unlink(path)
    owned = [E.owned_streams()]
    error = None
    try:
        e.infer_async(None, CONF, 0.45, 0.1)
    except E.EngineError as ex:
        error = str(ex)
    owned.append(E.owned_streams())
    x = torch.from_numpy(u.rng.frame(1234, 64, 64)).cuda()
    torch.cuda.synchronize()
    got = e.infer(x, CONF, 0.45, 0.1)
    owned.append(E.owned_streams())
    want = steady.infer(x, CONF, 0.45, 0.1)
    res = {"owned": owned, "error": error, "detections": len(got), "same_bytes": got.tobytes() == want.tobytes()}
    for h in (e, steady):
        h.close()
    return res


CASES = {"handles_first": lambda: two_frames(True), "streams_first": lambda: two_frames(False), "plan_change": plan_change,
         "failed_capture": failed_capture}

if __name__ == "__main__":
    print(json.dumps(CASES[sys.argv[1]]()))
