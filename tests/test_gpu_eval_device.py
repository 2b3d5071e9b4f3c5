"""csrc/evalmatch.hip on the GPU through the unina_eval_* entry points: the small-object counters against the reference's
stored counts, conformal scores bit-equal and in order to metrics.conformal_quantile's, true-positive masks equal to
metrics.ap_rows_numpy, at the shapes where the kernel takes another path (lane stride, empty inputs, the full record
buffer), for shuffled and tied input, over several updates, and past the capacity of the lists; then evaluate() end to end
on the engine, device metrics against host metrics."""
import numpy as np
import pytest

from conftest import load_golden
from eval_cases import conformal_scores, host_image   # noqa: F401  (the host path of one image, shared with the edge tests)
from records import MAXD, det_buffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def gold():
    g = load_golden("evalmatch_seed1234.npz")
    n = len(g["counts"])
    return {"n": n, "counts": g["counts"], "geom": g["geom"], "names": [str(s) for s in g["names"]],
            "dets": [g[f"dets/{i:02d}"] for i in range(n)], "labels": [g[f"labels/{i:02d}"] for i in range(n)]}


def params(engine, geom, imgsz=640):
    w, h, nw, nh = (int(v) for v in geom)
    return engine.EvalParams(w / nw, h / nh, imgsz / nw, imgsz / nh, w, h, imgsz, 15.0, 0.5)


ALL = 7   # UNINA_EVAL_SMALL | UNINA_EVAL_CONFORMAL | UNINA_EVAL_AP


def run_device(torch, engine, images, max_scores=1 << 16, max_rows=1 << 16, what=ALL, num_classes=4):
    """images: [(dets, labels, geom)] -> (EvalResult, scores, rows) after one update per image."""
    ev = engine.DeviceEval(num_classes, max_scores, max_rows)
    try:
        ev.reset()
        for dets, labels, geom in images:
            ev.update(det_buffer(torch, dets, len(dets)), labels, params(engine, geom), what)
        return ev.read()
    finally:
        ev.close()


def check_against_host(torch, engine, metrics, images):
    res, scores, rows = run_device(torch, engine, images)
    want = [host_image(metrics, *im) for im in images]
    counts = np.sum([w[0] for w in want], axis=0) if want else np.zeros(3)
    assert [res.tp, res.fp, res.fn] == [int(v) for v in counts]
    ws = np.concatenate([w[1] for w in want]) if want else np.zeros(0)
    wr = np.concatenate([w[2] for w in want]) if want else np.zeros(0, dtype=metrics.AP_ROW_DTYPE)
    assert res.n_scores == len(ws) and scores.tobytes() == ws.tobytes()          # bit-equal float64, in order
    assert res.n_rows == len(wr) and rows.tobytes() == wr.tobytes()
    lc = np.zeros(4, dtype=np.int64)
    for _, labels, _ in images:
        lc += np.bincount(labels[:, 0].astype(np.int64), minlength=4)[:4]
    assert list(res.label_counts[:4]) == lc.tolist() and not any(res.label_counts[4:])
    assert res.overflow == 0 and res.guard_intact == 1
    return res, scores, rows


def test_golden_images_match_reference_counts_and_host_scores(pkg, torch_cuda, gold):
    from unina_yolo_dla_amd import engine, metrics
    images = [(gold["dets"][i], gold["labels"][i], gold["geom"][i]) for i in range(gold["n"])]
    res, scores, rows = check_against_host(torch_cuda, engine, metrics, images)
    assert [res.tp, res.fp, res.fn] == gold["counts"].sum(axis=0).tolist()        # the reference's SmallObjectMetric
    assert len(scores) >= 100 and len(np.unique(rows["tp_mask"])) >= 5
    # image by image, so that an error cannot cancel across images
    for i, im in enumerate(images):
        r, _, _ = run_device(torch_cuda, engine, [im], what=1)
        assert [r.tp, r.fp, r.fn] == gold["counts"][i].tolist(), gold["names"][i]


def synth_image(seed, n, m, tie_every=0):
    """n records and m labels on a 1/8-pixel grid: every label small or mid-sized, records jittered copies of labels."""
    from unina_yolo_dla_amd.engine import DET_DTYPE
    rng = np.random.RandomState(seed)
    q = lambda v: np.round(v * 8) / 8                                     # noqa: E731
    w, h = q(rng.uniform(4, 24, m)), q(rng.uniform(4, 24, m))
    x1, y1 = q(rng.uniform(0, 640 - 24, m)), q(rng.uniform(0, 640 - 24, m))
    cls = rng.randint(0, 4, m)
    labels = np.stack([cls, (x1 + w / 2) / 640, (y1 + h / 2) / 640, w / 640, h / 640], axis=1).astype(np.float64).reshape(-1, 5)
    dets = np.zeros(n, dtype=DET_DTYPE)
    for i in range(n):
        if m and rng.rand() < 0.7:
            g = rng.randint(m)
            j = q(rng.uniform(-2, 2, 4))
            box, c = (x1[g] + j[0], y1[g] + j[1], x1[g] + w[g] + j[2], y1[g] + h[g] + j[3]), cls[g]
        else:
            bw, bh = q(rng.uniform(2, 30, 2))
            bx, by = q(rng.uniform(0, 600, 2))
            box, c = (bx, by, bx + bw, by + bh), rng.randint(0, 4)
        dets[i] = (*box, rng.randint(1, 1 << 20) / float(1 << 20), int(c), 1, 0)
    if tie_every:
        dets["confidence"][::tie_every] = np.float32(0.5)
    return dets, labels, np.array([640, 640, 640, 640])


def test_shapes_at_the_kernel_boundaries(pkg, torch_cuda):
    """Empty inputs, the exact-0.5 pair, the lane stride (64 | 65 labels), the label limit and the full record buffer."""
    from unina_yolo_dla_amd import engine, metrics
    from unina_yolo_dla_amd.engine import DET_DTYPE
    geom = np.array([640, 640, 640, 640])
    one = np.zeros(1, dtype=DET_DTYPE)
    one[0] = (160, 320, 170, 325, 0.9, 3, 1, 0)
    half = np.array([[3, 162.5 / 640, 322.5 / 640, 5 / 640, 5 / 640]])
    r, s, rows = check_against_host(torch_cuda, engine, metrics, [(one, half, geom)])
    assert [r.tp, r.fp, r.fn] == [1, 0, 0] and s.tolist() == [0.5] and rows["tp_mask"].tolist() == [1]   # IoU exactly 0.5: >= on both paths
    cases = {"n0": synth_image(1, 0, 20), "m0": synth_image(2, 30, 0), "n0m0": synth_image(3, 0, 0), "m64": synth_image(4, 90, 64),
             "m65": synth_image(5, 90, 65), "m256": synth_image(6, 300, 256), "n1024": synth_image(7, 1024, 32)}
    for name, im in cases.items():
        r, s, rows = check_against_host(torch_cuda, engine, metrics, [im])
        assert r.n_rows == len(im[0]), name
        if name in ("m64", "m65", "m256", "n1024"):
            assert r.tp > 0 and r.n_scores > 0, name
    # a label matched in the last lane slot and one past the stride: label 64 / 255 is the only one of its class
    dets, labels, geom = synth_image(8, 40, 256)
    for g in (63, 64, 255):
        lab = labels.copy()
        lab[:, 0] = np.where(np.arange(256) == g, 1, 0)
        d = dets[:1].copy()
        xc, yc, w, h = lab[g, 1:] * 640
        d[0] = (xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2, 0.9, 1, 1, 0)
        r, s, rows = check_against_host(torch_cuda, engine, metrics, [(d, lab, geom)])
        assert r.n_scores == 1 and rows["tp_mask"][0] == 0x3ff, g


def test_record_order_does_not_matter(pkg, torch_cuda):
    """The kernel sorts for itself: records in any order, with tied confidences, give what the host's stable sort gives.
    For the shuffled copy the tie order is the shuffled index order, so it is compared with the host on the same shuffle."""
    from unina_yolo_dla_amd import engine, metrics
    dets, labels, geom = synth_image(11, 200, 60, tie_every=3)
    assert (dets["confidence"] == np.float32(0.5)).sum() > 60
    by_conf = dets[np.argsort(-dets["confidence"], kind="stable")]
    a = check_against_host(torch_cuda, engine, metrics, [(dets, labels, geom)])
    b = check_against_host(torch_cuda, engine, metrics, [(by_conf, labels, geom)])
    assert [a[0].tp, a[0].fp, a[0].fn] == [b[0].tp, b[0].fp, b[0].fn] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    perm = np.random.RandomState(5).permutation(len(dets))
    check_against_host(torch_cuda, engine, metrics, [(dets[perm], labels, geom)])
    # distinct confidences: any shuffle gives the same bytes
    d2, l2, _ = synth_image(12, 150, 40)
    assert len(np.unique(d2["confidence"])) == len(d2)
    x = run_device(torch_cuda, engine, [(d2, l2, geom)])
    y = run_device(torch_cuda, engine, [(d2[np.random.RandomState(6).permutation(len(d2))], l2, geom)])
    assert x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes() and [x[0].tp, x[0].fp, x[0].fn] == [y[0].tp, y[0].fp, y[0].fn]


def test_updates_accumulate_reset_zeroes_and_runs_repeat(pkg, torch_cuda):
    from unina_yolo_dla_amd import engine, metrics
    images = [synth_image(21, 120, 50), synth_image(22, 80, 70)]
    first = check_against_host(torch_cuda, engine, metrics, images)      # two updates, one read == one host run over both
    again = run_device(torch_cuda, engine, images)
    assert bytes(first[0]) == bytes(again[0]) and first[1].tobytes() == again[1].tobytes() and first[2].tobytes() == again[2].tobytes()
    ev = engine.DeviceEval(4, 4096, 4096)
    try:
        ev.reset()
        for dets, labels, geom in images:
            ev.update(det_buffer(torch_cuda, dets, len(dets)), labels, params(engine, geom), ALL)
        ev.reset()
        res, scores, rows = ev.read()
        assert bytes(res)[:48 - 4] == bytes(44) and res.guard_intact == 1 and not any(res.label_counts) and len(scores) == 0 and len(rows) == 0
        ev.update(det_buffer(torch_cuda, images[1][0], len(images[1][0])), images[1][1], params(engine, images[1][2]), ALL)   # and it counts from zero again
        res, scores, rows = ev.read()
        want = host_image(metrics, *images[1])
        assert (res.tp, res.fp, res.fn) == want[0] and scores.tobytes() == want[1].tobytes() and rows.tobytes() == want[2].tobytes()
    finally:
        ev.close()


def test_lists_past_their_capacity_set_the_flag_and_stay_in_bounds(pkg, torch_cuda):
    from unina_yolo_dla_amd import engine, metrics
    images = [synth_image(31, 100, 60), synth_image(32, 100, 60)]
    full = run_device(torch_cuda, engine, images)
    assert full[0].n_scores > 10 and full[0].overflow == 0
    res, scores, rows = run_device(torch_cuda, engine, images, max_scores=2, max_rows=150)
    assert res.overflow == 3 and res.guard_intact == 1                       # canary words behind both lists untouched
    assert res.n_scores == full[0].n_scores and res.n_rows == 200            # the counts stay true
    assert scores.tobytes() == full[1][:2].tobytes() and rows.tobytes() == full[2][:150].tobytes()
    assert (res.tp, res.fp, res.fn) == (full[0].tp, full[0].fp, full[0].fn)
    res, scores, rows = run_device(torch_cuda, engine, images, max_scores=0, max_rows=0)
    assert res.overflow == 3 and res.guard_intact == 1 and len(scores) == 0 and len(rows) == 0


def test_evaluate_device_metrics_equal_host_metrics(pkg, sd7, torch_cuda, tmp_path):
    """evaluate() on a 64 x 64 engine over six labelled frames (five network tensors, one camera frame): the device path
    returns the host path's small_object dict, conformal dict (every key, exactly) and AP numbers."""
    from unina_yolo_dla_amd import evaluate as ev, export
    g = pkg.graph.Graph(in_h=64, in_w=64)
    path = str(tmp_path / "m.une")
    export.export_engine(sd7, path, g)
    root = tmp_path / "set"
    (root / "images").mkdir(parents=True)
    (root / "labels").mkdir()
    det = ev.EngineDetector(path, autotune=False)
    try:
        rng = np.random.RandomState(9)
        frames = {f"f{s}": pkg.rng.frame(s, 64, 64)[0] for s in (1234, 1235, 1236, 1237, 1238)}
        frames["cam"] = rng.randint(0, 256, (48, 80, 3)).astype(np.uint8)
        n_labels = 0
        for name, x in frames.items():
            np.save(root / "images" / f"{name}.npy", x)
            w, h = ev.frame_size(x)
            dets = det(x, 0.05, 0.45, 0.0)
            rows = []
            for i, d in enumerate(dets[::2][:40]):       # every second detection, shifted / shrunk by a fixed pattern
                s = 0.8 if i % 3 == 0 else 1.0
                bw, bh = (d["x2"] - d["x1"]) * s, (d["y2"] - d["y1"]) * s
                xc, yc = (d["x1"] + d["x2"]) / 2 + 0.25 * (i % 4), (d["y1"] + d["y2"]) / 2 + 0.25 * (i % 3)
                rows.append(f"{int(d['class_id'])} {xc / 64:.6f} {yc / 64:.6f} {bw / 64:.6f} {bh / 64:.6f}")
            rows.append("0 0.100000 0.900000 0.050000 0.050000")
            (root / "labels" / f"{name}.txt").write_text("\n".join(rows) + "\n")
            n_labels += len(rows)
        assert n_labels > 30
        size = (det.width, det.height)
        host = ev.evaluate(det, str(root), 64, 0.05, 0.45, 0.0, str(tmp_path / "host"), size, 0.1, map_metrics=True)
        dev = ev.evaluate(det, str(root), 64, 0.05, 0.45, 0.0, str(tmp_path / "dev"), size, 0.1, map_metrics=True, device_metrics=True)
    finally:
        det.close()
    assert host["small_object"]["small_object_tp"] > 0 and host["conformal"]["num_calibration_samples"] >= 10 and host["map50"] > 0
    assert dev["small_object"] == host["small_object"]
    assert dev["conformal"] == host["conformal"]                                 # every key, exactly
    assert dev["map50"] == host["map50"] and dev["map50_95"] == host["map50_95"]
    assert dev["predictions"] == host["predictions"]
    print(f"small_object {dev['small_object']} | conformal {dev['conformal']} | map50 {dev['map50']:.4f} map50_95 {dev['map50_95']:.4f}")
