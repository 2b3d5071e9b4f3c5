"""CPU tests of the data-mining path: the numpy twins against the reference's recorded results
(tests/golden/mining_seed1234.npz, made by tests/golden/make_golden_mining.py from active_learning.py), the C ABI's new
symbols and argument checks, the command line with a stub engine."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

NEW_SYMBOLS = ["unina_embedding_dim", "unina_mine_async", "unina_mine", "unina_mine_heads_async", "unina_kcenter"]
ERR_ARG = 4


def score_bound(ref32, ref64):
    """Scores on IDENTICAL logits: the only freedom is the rounding of exp / log, so allow max(8 ulp of the value,
    4 x |ref32 - ref64|) -- the reference's own fp32 error against its float64 evaluation."""
    return np.maximum(8 * np.spacing(np.abs(ref32).astype(np.float32)).astype(np.float64), 4 * np.abs(ref32.astype(np.float64) - ref64))


def assert_scores(got, ref32, ref64, what):
    dev = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    bound = score_bound(ref32, ref64)
    print(f"{what}: worst |got - ref32| {dev.max():.3g}, bound there {bound[np.argmax(dev - bound)]:.3g}")
    assert (dev <= bound).all(), (what, got, ref32, dev, bound)


@pytest.fixture(scope="module")
def gold():
    return load_golden("mining_seed1234.npz")


def head_case_names(gold):
    return sorted({k.split("/")[1] for k in gold.files if k.startswith("heads/")})


def test_difficulty_from_heads_matches_reference_on_golden_frame(pkg, gold):
    """frame640_seed1234.npz holds the reference's six heads of frame seed 1234 in fp32 = frame 0 of the mining fixture.
    Observed worst deviation: 0 (numpy and torch round exp / log alike here)."""
    from unina_yolo_dla_amd import mining
    f = load_golden("frame640_seed1234.npz")
    got = mining.difficulty_from_heads({n: f[f"head/{n}"] for n in mining.CLS_NAMES})
    assert_scores(got, gold["f640/scores32"][0], gold["f640/scores64"][0], "frame 1234")


def test_difficulty_from_heads_matches_reference_on_head_cases(pkg, gold):
    """Synthetic logits away from zero (nothing saturates at ln 2), num_classes 1, 4, 20, extremum in P4 only, mixed signs.
    Observed worst deviation: 6e-8 (one ulp)."""
    from unina_yolo_dla_amd import mining
    names = head_case_names(gold)
    assert {"nc1", "nc4", "nc20", "nc4_p4only"} <= set(names)
    for name in names:
        planes = [gold[f"heads/{name}/p{l}_cls"] for l in (2, 3, 4)]
        got = mining.difficulty_from_heads(planes)
        assert_scores(got, gold[f"heads/{name}/scores32"], gold[f"heads/{name}/scores64"], name)
    # the attenuated frames are what makes the frame fixture discriminating: everything else sits at ln 2
    ent = gold["f640/scores32"][:, 6]
    assert (np.abs(ent[[3, 5]] - np.log(2)) > 1e-3).all() and (np.abs(np.delete(ent, [3, 5]) - np.log(2)) < 1e-6).all()


# fp32 oracle (C, its own summation order) against the reference's fp32 torch forward, pooled: a P4 element is a chain of
# fp32 convs with up to 2304-term sums, each rounding ~2^-24 relative to the running sum, so element errors stay below
# ~1e-4 of the tensor's scale (the bound tests/test_gpu_strict.py uses per buffer); the mean over H*W cannot exceed the
# element bound. Values are ~0.1..0.5. Observed worst: 1.6e-7 absolute at 640x640, 2.0e-7 at 64x64.
EMBED_RTOL, EMBED_ATOL = 1e-4, 1e-5


@pytest.mark.parametrize("tag,size,idx", [("f640", 640, 0), ("f640", 640, 5), ("f64", 64, 1)])
def test_oracle_pool_matches_reference_embedding(pkg, oracle_mod, oracle_sd7, gold, tag, size, idx):
    x = pkg.rng.frame(int(gold[f"{tag}/seeds"][idx]), size, size)
    if tag == "f640":
        for i, m in zip(gold["f640/attenuate_idx"], gold["f640/attenuate_mul"]):
            if i == idx:
                x = (x * np.float32(m)).astype(np.float32)
    ref = oracle_mod.forward(oracle_sd7, x, keep_all=True)
    p4 = ref["backbone.stage3_c3k2.cv3"]
    got = p4.astype(np.float64).mean(axis=(1, 2))
    want = gold[f"{tag}/embed"][idx]
    assert got.shape == want.shape == (256,)
    print(f"{tag}[{idx}]: worst |oracle pool - reference embedding| {np.abs(got - want).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=EMBED_RTOL, atol=EMBED_ATOL)


def kcenter_data(gold):
    seed, n, d, k, sel_seed = (int(v) for v in gold["kcenter/params"])
    emb = np.maximum(np.random.RandomState(seed).normal(0.16, 0.24, size=(n, d)), 0).astype(np.float32)
    return emb, k, sel_seed


def test_kcenter_numpy_and_coreset_selection_reproduce_reference(pkg, gold):
    from unina_yolo_dla_amd import mining
    emb, k, seed = kcenter_data(gold)
    want = gold["kcenter/selected"]
    assert float(gold["kcenter/margin"]) >= 1e-4
    got = mining.kcenter_numpy(emb, k, int(want[0]))
    assert got.tolist() == want.tolist()
    paths = [f"img_{i}.jpg" for i in range(len(emb))]
    state = np.random.get_state()
    chosen = mining.coreset_selection_kcenter(emb, paths, k, seed=seed, device=False)
    after = np.random.get_state()
    assert chosen == [paths[i] for i in want]
    assert state[0] == after[0] and (state[1] == after[1]).all() and state[2:] == after[2:]   # numpy's global state untouched
    # another seed starts elsewhere; seed=None draws from the global state as the reference does
    assert mining.coreset_selection_kcenter(emb[:64], paths[:64], 4, seed=3, device=False)[0] == paths[int(np.random.RandomState(3).randint(64))]
    np.random.seed(11)
    first = mining.coreset_selection_kcenter(emb[:64], paths[:64], 4, device=False)[0]
    assert first == paths[int(np.random.RandomState(11).randint(64))]


def test_coreset_selection_edge_cases(pkg, capsys):
    from unina_yolo_dla_amd import mining
    emb = np.arange(12, dtype=np.float32).reshape(4, 3)
    paths = list("abcd")
    assert mining.coreset_selection_kcenter(emb, paths, 9, seed=0, device=False) == paths     # target_size > n: all paths
    assert "WARNING" in capsys.readouterr().out
    with pytest.raises(ValueError):
        mining.coreset_selection_kcenter(np.zeros((0, 3), np.float32), [], 2, device=False)
    assert sorted(mining.coreset_selection_kcenter(emb, paths, 4, seed=0, device=False)) == paths
    # lowest index wins ties: rows 1 and 2 are equally far from row 0
    tie = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0]], dtype=np.float32)
    assert mining.kcenter_numpy(tie, 2, 0).tolist() == [0, 1]
    with pytest.raises(ValueError):
        mining.compute_difficulty_scores(None, [], [], mode="kmeans")


@pytest.fixture(scope="module")
def lib(pkg):
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    return engine.load_library()


def test_header_declares_and_library_exports_mining_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "unina_mi355.h")).read()
    assert re.search(r"#define\s+UNINA_MINE_SCORES\s+8\b", hdr)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym), sym
    from unina_yolo_dla_amd import engine
    assert set(NEW_SYMBOLS) <= set(engine.ABI_SYMBOLS)


def test_mining_entry_points_reject_bad_arguments_without_a_device(lib):
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert lib.unina_mine(None, None, p, p, None) == ERR_ARG
    assert lib.unina_mine_async(None, None, p, p, None) == ERR_ARG
    assert lib.unina_mine_heads_async(None, p, None) == ERR_ARG
    assert lib.unina_embedding_dim(None) == -ERR_ARG
    fake = 0x10000   # never dereferenced: the argument checks come first
    kc = lib.unina_kcenter
    assert kc(None, 8, 4, 2, 0, fake, None, None) == ERR_ARG          # null embeddings
    assert kc(fake, 8, 4, 2, 0, None, None, None) == ERR_ARG          # null selection
    assert kc(fake, 8, 4, 9, 0, fake, None, None) == ERR_ARG          # k > n
    assert kc(fake, 8, 4, 0, 0, fake, None, None) == ERR_ARG          # k < 1
    assert kc(fake, 8, 4, 2, 8, fake, None, None) == ERR_ARG          # first_index out of range
    assert kc(fake, 8, 4, 2, -1, fake, None, None) == ERR_ARG
    assert kc(fake + 4, 8, 4, 2, 0, fake, None, None) == ERR_ARG      # misaligned embeddings
    assert kc(fake, 0, 4, 0, 0, fake, None, None) == ERR_ARG          # empty set


def test_engine_file_records_the_embedded_models_width(pkg):
    """A base_channels=16 model is embedded at width 32: the header's last word tells the engine the model's own width, so
    the embedding reports 8 * 16 = 128 channels, not 256."""
    import struct
    from unina_yolo_dla_amd import export
    for bc, want in ((16, 16), (32, 0)):
        g = pkg.graph.Graph(base_channels=bc, in_h=64, in_w=64)
        blob = export.EngineBuilder(pkg.synth.make_state_dict(7, g), g).tobytes()
        assert struct.unpack_from("<I", blob, 72)[0] == want
        assert blob[76:128] == b"\0" * 52


class StubEngine:
    """Stands in for engine.Engine in the command's body: scores from the frame's mean, a 4-float embedding."""
    width, height, device = 32, 32, 0

    def mine(self, frame, embed=True):
        m = float(np.asarray(frame.cpu() if hasattr(frame, "cpu") else frame).mean())
        s = np.full(8, m, dtype=np.float32)
        s[7] = 1 - m
        return s, (np.array([m, 2 * m, 0, 1], dtype=np.float32) if embed else None)


def test_cli_writes_the_reference_schema(pkg, tmp_path, monkeypatch, capsys):
    from unina_yolo_dla_amd import mine, mining
    monkeypatch.setattr(mining, "_device_frame", lambda engine, frame: frame)
    data = tmp_path / "data"
    data.mkdir()
    for i, v in enumerate((0.25, 0.75)):
        np.save(data / f"frame{i}.npy", np.full((3, 32, 32), v, dtype=np.float32))
    (data / "notes.txt").write_text("not an image")
    out, cs = tmp_path / "difficulty_map.json", tmp_path / "coreset.json"
    args = mine.parser().parse_args(["--engine", "m.une", "--data", str(data), "--output", str(out), "--coreset", "2",
                                     "--coreset-output", str(cs)])
    args.device_kcenter = False
    scores = mine.run(StubEngine(), args)
    text = out.read_text()
    got = json.loads(text)
    assert got == scores and text == json.dumps(scores, indent=2)
    assert sorted(got) == sorted(str(data / f"frame{i}.npy") for i in range(2))
    assert all(isinstance(v, float) for v in got.values())
    assert got[str(data / "frame1.npy")] == pytest.approx(0.75)
    assert sorted(json.loads(cs.read_text())) == sorted(got)
    printed = capsys.readouterr().out
    assert "Top 5 Most Uncertain Images" in printed and printed.index("frame1.npy: 0.7500") < printed.index("frame0.npy: 0.2500")
    # --limit and mode loc_var
    args = mine.parser().parse_args(["--engine", "m.une", "--data", str(data), "--output", str(out), "--limit", "1", "--mode", "loc_var"])
    assert list(mine.run(StubEngine(), args).values()) == [pytest.approx(0.75)]
    with pytest.raises(ValueError):
        mine.load_frame(str(data / "frame0.npy"), 64, 64)


def test_letterbox_geometry_and_pil_loader(tmp_path):
    from unina_yolo_dla_amd import mine
    assert mine.letterbox_geometry(1280, 720, 640, 640) == (640, 360, 0, 140)
    assert mine.letterbox_geometry(720, 1280, 640, 640) == (360, 640, 140, 0)
    assert mine.letterbox_geometry(640, 640, 640, 640) == (640, 640, 0, 0)
    assert mine.letterbox_geometry(100, 50, 64, 48) == (64, 32, 0, 8)
    Image = pytest.importorskip("PIL.Image")
    img = np.zeros((36, 64, 3), dtype=np.uint8)
    img[..., 0] = 255
    Image.fromarray(img).save(tmp_path / "red.png")
    x = mine.load_frame(str(tmp_path / "red.png"), 64, 64)
    assert x.shape == (3, 64, 64) and x.dtype == np.float32
    assert np.allclose(x[:, 0, 0], 114 / 255) and np.allclose(x[:, 32, 32], [1, 0, 0]) and np.allclose(x[:, 63, 63], 114 / 255)
