"""tools/node_harness.cpp mode F<code>: the compiled C++ consumer of the ABI building a unina_frame from its GpuBufferHandle -- the
dispatch on the message's format code that the reference node lacks -- run as a child process and compared, byte for byte, with
Engine.infer_frame through ctypes on the same frame."""
import subprocess

import numpy as np
import pytest

from frame_child import GRBG, NV12, UYVY, frame_rows
from nv12_child import nv12_planes, upload

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", [NV12, UYVY, GRBG], ids=["nv12", "uyvy", "grbg"])
def test_node_harness_frame_mode_matches_ctypes_byte_for_byte(pkg, sd7, tmp_path, fmt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import build, camera as twin, engine, export
    exe = build.build_harness()
    une = str(tmp_path / "fp16.une")
    export.export_engine(sd7, une)
    sh, sw = 720, 1280
    if fmt == NV12:
        pitch = 1536                                          # one pitch for both planes, the chroma plane right behind the luma
        y, uv = nv12_planes(95, sh, sw, pitch, pitch)
        buf = np.concatenate([y, uv])
    else:
        rows, _ = frame_rows(twin, fmt, 96, sh, sw)
        pitch = rows.shape[1] + 64
        buf = np.random.default_rng(97).integers(0, 256, (sh, pitch), dtype=np.uint8)
        buf[:, :rows.shape[1]] = rows
    fpath = str(tmp_path / "frame.bin")
    buf.tofile(fpath)
    out = str(tmp_path / "out_F.bin")
    conf, iou, q = 0.3, 0.45, 0.1
    r = subprocess.run([exe, une, fpath, str(sw), str(sh), str(pitch), f"F{fmt}", out, str(conf), str(iou), str(q)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = open(out, "rb").read()
    recs = np.frombuffer(raw[4:], dtype=engine.DET_DTYPE)
    assert len(recs) == int(np.frombuffer(raw[:4], dtype="<i4")[0])
    e = engine.Engine(une)
    try:
        d = upload(torch, buf)
        uvp = d.data_ptr() + pitch * sh if fmt == NV12 else None
        frame = engine.Frame.from_tensors(fmt, sw, sh, d, pitch, uvp, pitch if fmt == NV12 else 0)
        want = e.infer_frame(frame, None, conf, iou, q)
    finally:
        e.close()
    assert len(want) > 0 and recs.tobytes() == want.tobytes()
    # a format code the engine does not know is refused, not pre-processed as BGRA
    r = subprocess.run([exe, une, fpath, str(sw), str(sh), str(pitch), "F12", out], capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "unknown pixel format" in r.stderr, (r.stdout, r.stderr)
