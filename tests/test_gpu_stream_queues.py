"""Two frames in flight overlap at whatever GPU_MAX_HW_QUEUES the command was given (profiles/r05).

The runtime maps a stream onto a hardware queue when the stream is created -- a fresh queue while fewer than GPU_MAX_HW_QUEUES
(default 4) exist at that priority, the least-referenced one after that -- and two streams on one queue run one after the
other. Until round 5 every handle kept an idle capture stream: with the null stream that made three queues before the
caller's first stream existed, and the caller's two frame streams could share the fourth. Now the library holds no stream
(unina_debug_owned_streams() == 0 at rest; a capture makes one and destroys it), and unina_debug_streams_overlap measures what
the caller's streams got.

Every case runs in a child process of its own (stream_queues_child.py says why), which inherits GPU_MAX_HW_QUEUES."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "stream_queues_child.py")


def _case(name):
    r = subprocess.run([sys.executable, CHILD, name], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"{name}: {res}")
    return res


@pytest.mark.parametrize("order", ["handles_first", "streams_first"])
def test_two_frame_streams_overlap(order):
    """handles_first is bench.py's order (two handles, then two torch.cuda.Stream()s), streams_first the other one. One
    infer_async per handle on its own stream captures both graphs. Then: the library holds no stream (before, between and after
    the calls), the probe's 300 us kernels on (stream 0, stream 1) overlap in 3 of 3 repetitions, and on (stream 0, stream 0),
    the negative control, in none."""
    res = _case(order)
    assert min(res["detections"]) > 0, res["detections"]                 # the frames ran
    assert res["owned"] == [0] * len(res["owned"]), res["owned"]
    assert res["overlap_s0_s0"] == 0, res["stamps_s0_s0"]
    assert res["overlap_s0_s1"] == res["reps"] == 3, res["stamps_s0_s1"]


def test_plan_change_recaptures_and_holds_no_stream():
    """infer, set_fusion(False), infer (captures again), set_fusion(True), infer (and again). The first and the last call give
    the bytes of a handle that never switched; the call with fusion off gives the bytes of a handle that never switched either,
    loaded with fusion off (UNINA_FUSE=0). The library's stream count is 0 after each call."""
    res = _case("plan_change")
    assert res["groups"][0] > 0 and res["groups"][1] == 0 and res["groups"][2] == res["groups"][0], res["groups"]   # the plan did change
    assert res["steady_groups"] == [res["groups"][0], 0], res["steady_groups"]
    assert min(res["detections"]) > 0 and res["steady_detections"] == [res["detections"][0], res["detections"][1]], res
    assert res["same_bytes"] == [True, True, True], res
    assert res["owned"] == [0] * len(res["owned"]), res["owned"]


def test_failed_first_call_leaves_no_stream_and_a_usable_engine():
    """The error the ABI can raise without a device fault: infer_async with no 'images' tensor bound (UNINA_ERR_STATE). The
    count stays 0 and the handle's next frame equals a fresh handle's. make_ready raises it BEFORE hipStreamBeginCapture; no
    error between Begin and End can be provoked from outside without a faulty launch, so those paths are checked by reading:
    capture() and capture_full() hold the stream in a CaptureStream object (engine.hip) whose destructor ends an open capture,
    destroys the recorded graph and the stream, and decrements the count, whichever return statement is taken."""
    res = _case("failed_capture")
    assert res["error"] and "not bound" in res["error"], res["error"]
    assert res["owned"] == [0, 0, 0], res["owned"]
    assert res["detections"] > 0 and res["same_bytes"], res
