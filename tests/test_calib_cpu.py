"""INT8 calibration from |x| value-count tables (export.HistogramCalibrator.collect_counts, export.calibrate_counts) and
the exporter's command line (python -m unina_yolo_dla_amd.export), without a GPU.

An fp16 tensor has at most 32 768 distinct |x|, so the table "how many elements carry each 15-bit pattern" (what
csrc/calib.hip counts on the device) is a lossless summary of it: folding the table must give the SAME histogram, edges
and selected range as folding the tensor -- array_equal and float equality, no tolerance anywhere in this file."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

METHODS = ("entropy", "mse", "percentile")


def table(x):
    """What the kernel computes, on the host: counts[bits & 0x7fff] over the fp16 elements of x."""
    bits = np.ascontiguousarray(x, dtype=np.float16).reshape(-1).view(np.uint16)
    return np.bincount(bits & 0x7fff, minlength=32768).astype(np.uint32)


def _frames(seed):
    """fp16 frame sequences that walk every branch of collect: restart after a dead first frame, growth by whole bins, a
    maximum exactly on the current last edge (no growth, right-inclusive last bin), an empty frame. The ranges grow by
    factors below 4: the entropy / mse searches are quadratic in the bin count, and a few hundred appended bins walk the
    same code as tens of thousands."""
    r = np.random.default_rng(seed)

    def relu(n, scale):
        return np.maximum(r.standard_normal(n) * scale, 0).astype(np.float16)
    a = relu(5000, 1.0)
    on_edge = relu(3000, 0.5)
    on_edge[7] = a.max()                                  # equals the last edge after frame `a` opened the range
    signed = (r.standard_normal(4097) * 3).astype(np.float16)   # negative values: |x| folds the sign away
    seqs = {
        "dead_first": [np.zeros(1000, np.float16), np.zeros(10, np.float16), relu(4000, 2.0), relu(4000, 2.6)],
        "growth": [a, relu(5000, 1.3), relu(100, 1.7), signed],
        "on_edge": [a, on_edge, on_edge * np.float16(0.5)],
        "empty": [a, np.zeros(0, np.float16), relu(777, 2.0)],
        "empty_first": [np.zeros(0, np.float16), a],
        "tiny": [np.full(64, 6e-8, np.float16), relu(500, 1.0)],     # subnormal-only first frame: the range (0, 1e-6] restarts too
    }
    assert float(on_edge.max()) == float(a.max())
    return seqs


@pytest.mark.parametrize("case", ["dead_first", "growth", "on_edge", "empty", "empty_first", "tiny"])
def test_collect_counts_is_collect(pkg, case):
    from unina_yolo_dla_amd import export
    frames = _frames(11)[case]
    ct, cc = export.HistogramCalibrator(), export.HistogramCalibrator()
    for i, f in enumerate(frames):
        ct.collect(f.astype(np.float32))
        cc.collect_counts(table(f))
        assert np.array_equal(ct.hist, cc.hist), (case, i)
        assert np.array_equal(ct.edges, cc.edges), (case, i)
        assert cc.hist.dtype == ct.hist.dtype and cc.edges.dtype == ct.edges.dtype
    assert cc.hist.sum() == sum(f.size for f in frames)
    for m in METHODS:
        assert ct.amax(m, 99.9) == cc.amax(m, 99.9), (case, m)


def test_collect_itself_is_unchanged(pkg):
    """collect now shares its body with collect_counts: its result on a fixed sequence is what the restated algorithm gives
    when written out by hand (first frame: np.histogram over (0, max); second: whole bins appended)."""
    from unina_yolo_dla_amd import export
    r = np.random.default_rng(3)
    a = np.abs(r.standard_normal(2000)).astype(np.float32)
    b = (np.abs(r.standard_normal(2000)) * 3).astype(np.float32)
    c = export.HistogramCalibrator(num_bins=256)
    c.collect(a)
    c.collect(-b)
    h0, e0 = np.histogram(a, bins=256, range=(0.0, float(a.max())))
    width = e0[1] - e0[0]
    extra = int(np.ceil((float(b.max()) - e0[-1]) / width))
    e1 = np.concatenate([e0, e0[-1] + width * np.arange(1, extra + 1)])
    h1 = np.concatenate([h0.astype(np.float64), np.zeros(extra)]) + np.histogram(b, bins=e1)[0]
    assert np.array_equal(c.edges, e1) and np.array_equal(c.hist, h1)


@pytest.fixture(scope="module")
def emulated(pkg):
    """The fp16 activation buffers of 4 frames at 64x64 from the op-table emulator, rounded through float16 (what the engine
    stores), and their value-count tables."""
    from emulate import run_op_table
    from unina_yolo_dla_amd import export
    g = pkg.graph.Graph(in_h=64, in_w=64)
    b = export.EngineBuilder(pkg.synth.make_state_dict(7, g), g)
    names = [n for (n, _h, _w, _c, dtype, _f, _s) in b.buffers if dtype == export.BUF_F16]
    named, tables = [], []
    for i in range(4):
        bufs = run_op_table(b, pkg.rng.frame(5000 + i, 64, 64))[1]
        named.append({n: np.asarray(bufs[n]).astype(np.float16).astype(np.float32) for n in names})
        tables.append(np.stack([table(named[-1][n]) for n in names]))
    return names, named, tables


@pytest.mark.parametrize("method,pct", [(None, None), ("max", None), ("entropy", None), ("mse", None), ("percentile", None),
                                        ("percentile", 99.9)])
def test_calibrate_counts_is_calibrate(pkg, emulated, method, pct):
    from unina_yolo_dla_amd import export
    names, named, tables = emulated
    want = export.calibrate(named, pct, method)
    got = export.calibrate_counts(tables, names, pct, method)
    assert len(got) == len(names) > 20
    assert got == want


def test_calibrate_counts_all_is_calibrate_all(pkg, emulated):
    from unina_yolo_dla_amd import export
    names, named, tables = emulated
    specs = {"max": ("max", None), "mse": ("mse", None), "p999": ("percentile", 99.9), "p": ("percentile", None)}
    assert export.calibrate_counts_all(tables, names, specs) == export.calibrate_all(named, specs)


def test_non_finite_patterns_and_max_percentile_are_refused(pkg):
    from unina_yolo_dla_amd import export
    ok = table(np.array([0.0, 1.0, -2.0], np.float16))
    for pattern in (0x7c00, 0x7c01, 0x7fff):               # +Inf, a signalling NaN, the last NaN
        t = ok.copy()
        t[pattern] = 1
        with pytest.raises(ValueError, match="non-finite"):
            export.HistogramCalibrator().collect_counts(t)
        with pytest.raises(ValueError, match="non-finite"):
            export.calibrate_counts([t[None]], ["x"])
    t = ok.copy()
    t[0x7bff] = 2                                          # 65504, the largest finite fp16: fine
    c = export.HistogramCalibrator()
    c.collect_counts(t)
    assert c.edges[-1] == 65504.0 and c.hist.sum() == 5
    assert export.calibrate_counts([t[None]], ["x"]) == {"x": 65504.0}
    with pytest.raises(ValueError, match="calibrate_amax"):
        export.calibrate_counts([ok[None]], ["x"], percentile=99.9)
    with pytest.raises(ValueError, match="calibrate_amax"):
        export.calibrate_counts([ok[None]], ["x"], percentile=99.9, method="max")
    with pytest.raises(ValueError):
        export.HistogramCalibrator().collect_counts(ok[:100])       # not a 32 768-entry table
    with pytest.raises(ValueError):
        export.calibrate_counts([ok[None]], ["x", "y"])              # rows and names disagree


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "unina_yolo_dla_amd.export", *args], cwd=ROOT, capture_output=True, text=True)


@pytest.fixture(scope="module")
def weights(pkg, tmp_path_factory):
    g = pkg.graph.Graph(in_h=64, in_w=96)
    sd = pkg.synth.make_state_dict(7, g)
    path = str(tmp_path_factory.mktemp("calib_cli") / "w.unsd")
    pkg.statedict.save(path, sd)
    return path, sd, g


@pytest.mark.parametrize("precision", ["fp16", "fp32", "strict"])
def test_cli_writes_export_engine_bytes(pkg, weights, tmp_path, precision):
    from unina_yolo_dla_amd import export
    path, sd, g = weights
    out = tmp_path / "m.une"
    r = _cli("--weights", path, "--out", str(out), "--precision", precision, "--size", "64", "96")
    assert r.returncode == 0, r.stderr
    want = export.EngineBuilder(sd, g, export.PRECISIONS[precision]).tobytes()
    assert out.read_bytes() == want
    hdr = export.read_engine_header(str(out))
    assert (hdr["in_h"], hdr["in_w"], hdr["precision"]) == (64, 96, export.PRECISIONS[precision])


def test_cli_reads_the_graph_off_the_state_dict(pkg, tmp_path):
    """Variant, width, class count and lite_p2 come from the tensors: a graph (B) model with 7 classes needs no flags."""
    from unina_yolo_dla_amd import export
    for g in (pkg.graph.Graph(num_classes=7, in_h=64, in_w=64, variant="B"), pkg.graph.Graph(lite_p2=True, in_h=64, in_w=64)):
        sd = pkg.synth.make_state_dict(5, g)
        got = export.graph_for(sd, 64, 64)
        assert (got.variant, got.num_classes, got.base_channels, got.lite_p2) == (g.variant, g.num_classes, g.base_channels, g.lite_p2)


def test_cli_argument_errors_exit_non_zero(pkg, weights, tmp_path):
    path, _sd, _g = weights
    out = str(tmp_path / "m.une")
    bad = tmp_path / "bad.unsd"
    bad.write_bytes(b"not a state dict")
    empty = tmp_path / "empty_dir"
    empty.mkdir()
    for args in (
        ["--out", out],                                                                        # no weights
        ["--weights", path],                                                                   # no output
        ["--weights", path, "--out", out, "--precision", "int4"],                              # unknown precision
        ["--weights", path, "--out", out, "--precision", "int8"],                              # int8 without calibration images
        ["--weights", path, "--out", out, "--precision", "int8", "--calib-dir", str(empty)],   # ... with none in the folder
        ["--weights", path, "--out", out, "--precision", "int8", "--calib-dir", str(empty), "--calibrator", "kl"],
        ["--weights", path, "--out", out, "--precision", "int8", "--calib-dir", str(empty), "--calib-frames", "0"],
        ["--weights", path, "--out", out, "--calib-dir", str(empty)],                          # calibration images for fp16
        ["--weights", path, "--out", out, "--percentile", "99.9"],                             # percentile without its calibrator
        ["--weights", path, "--out", out, "--size", "64"],                                     # H without W
        ["--weights", path, "--out", out, "--size", "60", "64"],                               # not a multiple of 16
        ["--weights", str(bad), "--out", out],                                                 # not a weights file
        ["--weights", str(tmp_path / "missing.unsd"), "--out", out],
    ):
        r = _cli(*args)
        assert r.returncode != 0 and "Traceback" not in r.stderr, (args, r.stderr)
        assert not os.path.exists(out), args
