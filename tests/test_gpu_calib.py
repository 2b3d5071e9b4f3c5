"""GPU tests of INT8 calibration on the device (csrc/calib.hip behind unina_abs_histogram_f16 / unina_calib_*), through the
C ABI and engine.py.

Everything here is exact: the kernel counts integers (counts[bits & 0x7fff] += 1), so its table equals np.bincount of the
same bits, two runs give the same bytes, and the ranges export.calibrate_counts selects from the tables are the floats
export.calibrate selects from the tensors. No tolerance anywhere in this file."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BINS = 32768
# tails (n % 8 != 0, n < 8), one full vector, more than one workgroup (2^20 + 3 elements: 9 chunks of the kernel's 2^17-element
# minimum, merged by global atomics) and, with it, a tail behind a multi-workgroup body
SIZES = (1, 7, 8, 9, 4097, (1 << 20) + 3)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def bincount(bits):
    return np.bincount(np.asarray(bits, dtype=np.uint16).reshape(-1) & 0x7fff, minlength=BINS).astype(np.uint32)


def patterns(kind, n):
    r = np.random.default_rng(n * 7 + len(kind))
    if kind == "zeros":
        return np.zeros(n, np.uint16)
    if kind == "signed_zeros":                       # +0 and -0 share bin 0
        return np.where(r.integers(0, 2, n) == 1, 0x8000, 0).astype(np.uint16)
    if kind == "ones":                               # every lane of every wave adds to ONE bin: the worst contention
        return np.full(n, 0x3c00, np.uint16)
    if kind == "random":                             # all 65 536 patterns, Inf / NaN included: counted, not interpreted
        return r.integers(0, 1 << 16, n).astype(np.uint16)
    if kind == "relu":                               # a post-ReLU activation: about half exact zeros
        return np.maximum(r.standard_normal(n), 0).astype(np.float16).view(np.uint16)
    raise KeyError(kind)


def to_device(torch, bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.float16)


@pytest.mark.parametrize("kind", ["zeros", "signed_zeros", "ones", "random", "relu"])
def test_abs_histogram_is_bincount(pkg, torch_cuda, kind):
    from unina_yolo_dla_amd.engine import abs_histogram_f16
    for n in SIZES:
        bits = patterns(kind, n)
        t = to_device(torch_cuda, bits)
        got = abs_histogram_f16(t)
        assert got.dtype == np.uint32 and got.shape == (BINS,)
        assert int(got.sum(dtype=np.uint64)) == n, (kind, n)
        assert np.array_equal(got, bincount(bits)), (kind, n)
        assert abs_histogram_f16(t).tobytes() == got.tobytes(), (kind, n)      # a second run: the same bytes
    if kind == "random":
        assert bincount(patterns(kind, SIZES[-1]))[0x7c00:].sum() > 0          # the case does hold non-finite patterns


def test_abs_histogram_rejects_bad_arguments(pkg, torch_cuda):
    from unina_yolo_dla_amd.engine import load_library, abs_histogram_f16, EngineError
    L = load_library()
    torch = torch_cuda
    t = torch.zeros(64, dtype=torch.float16, device="cuda")
    out = torch.zeros(BINS + 8, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ARG = 4
    assert L.unina_abs_histogram_f16(t.data_ptr(), 64, out.data_ptr(), s) == 0
    assert L.unina_abs_histogram_f16(None, 64, out.data_ptr(), s) == ARG
    assert L.unina_abs_histogram_f16(t.data_ptr(), 64, None, s) == ARG
    assert L.unina_abs_histogram_f16(t.data_ptr(), 0, out.data_ptr(), s) == ARG
    assert L.unina_abs_histogram_f16(t.data_ptr() + 2, 8, out.data_ptr(), s) == ARG          # fp16-aligned, not 16-byte aligned
    assert L.unina_abs_histogram_f16(t.data_ptr(), 64, out.data_ptr() + 4, s) == ARG
    torch.cuda.synchronize()
    with pytest.raises(EngineError, match="ARG"):
        abs_histogram_f16(t[1:9])


ENGINES = {
    "A64": dict(in_h=64, in_w=64),
    "A96x160": dict(in_h=96, in_w=160),
    "B64": dict(in_h=64, in_w=64, variant="B"),
    "bc16": dict(in_h=64, in_w=64, base_channels=16),
}


@pytest.mark.parametrize("which", list(ENGINES))
def test_engine_tables_are_the_buffers_bincounts(pkg, torch_cuda, which):
    """Fusion off: after forward(x) every row of calib_counts() is the bincount of read_buffer(name) taken back to fp16
    bits (an fp16 value survives the trip through fp32 exactly); the names are the list calibrate_amax iterates; and
    calib_counts(x) is forward(x) followed by calib_counts()."""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    g = pkg.graph.Graph(**ENGINES[which])
    sd = pkg.synth.make_state_dict(7, g)
    b = export.EngineBuilder(sd, g)
    want_names = [n for (n, _h, _w, _c, dtype, _f, _s) in b.buffers if dtype == export.BUF_F16]
    x = torch_cuda.from_numpy(pkg.rng.frame(1234, g.in_h, g.in_w)).cuda()
    x2 = torch_cuda.from_numpy(pkg.rng.frame(77, g.in_h, g.in_w) * np.float32(0.5)).cuda()
    e = Engine.from_state_dict(sd, g)
    try:
        e.set_fusion(False)
        names = e.calib_buffer_names()
        assert names == want_names and len(names) > 20
        e.forward(x)
        got = e.calib_counts()
        assert got.shape == (len(names), BINS) and got.dtype == np.uint32
        for i, n in enumerate(names):
            buf = e.read_buffer(n)
            assert int(got[i].sum(dtype=np.uint64)) == buf.size, n
            assert np.array_equal(got[i], bincount(buf.astype(np.float16).view(np.uint16))), n
        assert e.calib_counts().tobytes() == got.tobytes()
        one_call = e.calib_counts(x2)
        assert not np.array_equal(one_call, got)
        e.forward(x2)
        assert e.calib_counts().tobytes() == one_call.tobytes()
    finally:
        e.close()


def test_calibration_is_refused_where_it_cannot_be_right(pkg, sd7, torch_cuda):
    """Fusion on: UNINA_ERR_STATE, and the message names unina_set_fusion. int8 / fp32 / STRICT engines: UNINA_ERR_UNSUPPORTED.
    A calibration call leaves the frame path alone: infer gives the same bytes before and after it."""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine, EngineError, calibrate_amax_device
    g = pkg.graph.Graph(in_h=64, in_w=64)
    sd = pkg.synth.make_state_dict(7, g)
    x = torch_cuda.from_numpy(pkg.rng.frame(1234, 64, 64)).cuda()
    e = Engine.from_state_dict(sd, g)
    try:
        assert e.set_fusion(True) > 0
        before = e.infer(x, conf_thr=0.05)
        assert len(before) > 0
        for call in (lambda: e.calib_counts(), lambda: e.calib_counts(x)):
            with pytest.raises(EngineError, match=r"STATE.*unina_set_fusion\(e, 0\)"):
                call()
        e.set_fusion(False)
        assert e.calib_counts(x).sum(dtype=np.uint64) > 0
        e.set_fusion(True)
        after = e.infer(x, conf_thr=0.05)
        assert after.tobytes() == before.tobytes()
    finally:
        e.close()
    amax = calibrate_amax_device(sd, g, [pkg.rng.frame(5000, 64, 64)])
    for precision, kw in ((export.INT8, dict(amax=amax)), (export.FP32, {}), (export.STRICT, {})):
        e = Engine.from_state_dict(sd, g, precision=precision, **kw)
        try:
            e.set_fusion(False)
            for call in (lambda: e.calib_counts(), lambda: e.calib_counts(x)):
                with pytest.raises(EngineError, match="UNSUPPORTED"):
                    call()
        finally:
            e.close()


@pytest.fixture(scope="module")
def calib_case(pkg):
    """64 x 64, three frames, the second scaled x4: the calibrators' ranges open on frame 0 and grow by whole bins on frame 1."""
    g = pkg.graph.Graph(in_h=64, in_w=64)
    sd = pkg.synth.make_state_dict(7, g)
    frames = [pkg.rng.frame(5000 + i, 64, 64) for i in range(3)]
    frames[1] = (frames[1] * np.float32(4.0)).astype(np.float32)
    return sd, g, frames


@pytest.mark.parametrize("method,pct", [(None, None), ("max", None), ("entropy", None), ("mse", None), ("percentile", 99.9)])
def test_calibrate_amax_device_is_calibrate_amax(pkg, torch_cuda, calib_case, method, pct):
    """The same dict, float for float. (The entropy / mse cases spend their time in the HOST range search, which both sides run:
    it is quadratic in the bin count and the x4 frame grows 2048 bins to about 8192.)"""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import calibrate_amax, calibrate_amax_device
    sd, g, frames = calib_case
    want = calibrate_amax(sd, g, frames, percentile=pct, method=method)
    got = calibrate_amax_device(sd, g, frames, percentile=pct, method=method)
    assert len(want) > 20 and got == want
    if method is None:                                           # the INT8 engine file does not depend on the range source
        assert export.EngineBuilder(sd, g, export.INT8, got).tobytes() == export.EngineBuilder(sd, g, export.INT8, want).tobytes()
        with pytest.raises(ValueError, match="calibrate_amax"):
            calibrate_amax_device(sd, g, frames, percentile=99.9)


def test_calibrate_amax_device_specs_is_calibrate_amax_specs(pkg, torch_cuda, calib_case):
    from unina_yolo_dla_amd.engine import calibrate_amax, calibrate_amax_device
    sd, g, frames = calib_case
    specs = {"max": ("max", None), "mse": ("mse", None), "p99.9": ("percentile", 99.9), "p": ("percentile", None)}
    want = calibrate_amax(sd, g, frames, specs=specs)
    got = calibrate_amax_device(sd, g, frames, specs=specs)
    assert set(got) == set(specs) and got == want


def test_cli_int8_calibrates_from_an_image_folder(pkg, torch_cuda, tmp_path):
    """python -m unina_yolo_dla_amd.export --precision int8 --calib-dir: the file equals export_engine's with the ranges
    calibrate_amax_device gives on the same frames (mine.load_frame), and it loads and infers."""
    from PIL import Image
    from unina_yolo_dla_amd import export, mine
    from unina_yolo_dla_amd.engine import Engine, calibrate_amax_device
    g = pkg.graph.Graph(in_h=64, in_w=64)
    sd = pkg.synth.make_state_dict(7, g)
    weights = tmp_path / "w.unsd"
    pkg.statedict.save(str(weights), sd)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    r = np.random.default_rng(5)
    for i, (w, h) in enumerate([(64, 64), (80, 48), (64, 64), (100, 100)]):     # one letterboxed, one resized; the 4th is not taken
        Image.fromarray(r.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(imgs / f"f{i}.png"))
    out = tmp_path / "m.une"
    p = subprocess.run([sys.executable, "-m", "unina_yolo_dla_amd.export", "--weights", str(weights), "--out", str(out),
                        "--precision", "int8", "--size", "64", "64", "--calib-dir", str(imgs), "--calib-frames", "3",
                        "--calibrator", "percentile", "--percentile", "99.9"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    files = mine.list_files(str(imgs))[:3]
    assert [os.path.basename(f) for f in files] == ["f0.png", "f1.png", "f2.png"]
    amax = calibrate_amax_device(sd, g, [mine.load_frame(f, 64, 64)[None] for f in files], percentile=99.9, method="percentile")
    assert out.read_bytes() == export.EngineBuilder(sd, g, export.INT8, amax).tobytes()
    assert export.read_engine_header(str(out))["precision"] == export.INT8
    e = Engine(str(out))
    try:
        dets = e.infer(torch_cuda.from_numpy(mine.load_frame(files[0], 64, 64)[None]).cuda(), conf_thr=0.05)
        assert dets.dtype.itemsize == 32 and bool((dets["valid"] == 1).all())
    finally:
        e.close()
