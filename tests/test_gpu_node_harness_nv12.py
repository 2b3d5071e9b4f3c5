"""tools/node_harness.cpp mode N: the compiled C++ consumer of the ABI feeding an NV12 buffer to unina_infer_nv12, run as a
child process and compared, byte for byte, with Engine.infer_nv12 through ctypes on the same frame."""
import subprocess

import numpy as np
import pytest

from nv12_child import nv12_planes, upload

pytestmark = pytest.mark.gpu


def test_node_harness_nv12_mode_matches_ctypes_byte_for_byte(pkg, sd7, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import build, engine, export
    exe = build.build_harness()
    une = str(tmp_path / "fp16.une")
    export.export_engine(sd7, une)
    sh, sw, pitch = 720, 1280, 1536                       # one pitch for both planes, the chroma plane right behind the luma
    y, uv = nv12_planes(81, sh, sw, pitch, pitch)
    fpath = str(tmp_path / "frame.nv12")
    np.concatenate([y, uv]).tofile(fpath)
    out = str(tmp_path / "out_N.bin")
    conf, iou, q = 0.3, 0.45, 0.1
    r = subprocess.run([exe, une, fpath, str(sw), str(sh), str(pitch), "N", out, str(conf), str(iou), str(q)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = open(out, "rb").read()
    recs = np.frombuffer(raw[4:], dtype=engine.DET_DTYPE)
    assert len(recs) == int(np.frombuffer(raw[:4], dtype="<i4")[0])
    e = engine.Engine(une)
    try:
        want = e.infer_nv12(upload(torch, y), upload(torch, uv), sw, sh, pitch, pitch, None, conf, iou, q)
    finally:
        e.close()
    assert len(want) > 0 and recs.tobytes() == want.tobytes()
