"""bench.py's plain run as the measurement harness sees it: exactly --steps timed frames, the headline fields only, and
--dump-outputs holding the detections of the LAST timed frame (what unina_infer_async left in that frame's slot)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from detcmp import compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def test_plain_run_times_steps_and_dumps_the_last_frame(pkg, sd7, torch_cuda, tmp_path):
    from unina_yolo_dla_amd.engine import DET_DTYPE, Engine
    steps, warmup = 8, 2                  # < N_SEEDED: the last timed frame is the seeded host frame 1234 + steps - 1
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["unit"] == "frames/s"
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-3)
    assert not {"latency_ms", "roofline", "cpu_baseline"} & set(line), "plain run measured more than the headline"

    got = np.load(out / "detections.npy")
    assert got.dtype == np.float32 and got.ndim == 2 and got.shape[1] == 6 and len(got) > 0
    dets = np.zeros(len(got), dtype=DET_DTYPE)
    for i, f in enumerate(("x1", "y1", "x2", "y2", "confidence", "class_id")):
        dets[f] = got[:, i]
    conf = line["config"]["thresholds"]["conf"]
    eng = Engine.from_state_dict(sd7, pkg.graph.Graph(), device=0)
    try:
        x = torch_cuda.from_numpy(pkg.rng.frame(1234 + steps - 1, 640, 640)).cuda()
        want = eng.infer(x, conf, 0.45, 0.1)
    finally:
        eng.close()
    # the bench autotunes its handles: tile choices may move fp16 head values by < 5e-3 (test_gpu_parity.py, autotune)
    stats = compare(dets, want, conf, min_iou=0.99, score_tol=2e-3)
    assert stats["matched"] >= len(want) - 2, stats
