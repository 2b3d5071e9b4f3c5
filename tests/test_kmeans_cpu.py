"""CPU tests of the k-means coreset's host side (mining.py): the float64 twins, the k-means++ start, the selection loop and
the reference's recorded selections (tests/golden/kmeans_blobs.npz, made by tests/golden/make_golden_kmeans.py, which runs
the reference's coreset_selection_kmeans). The device kernels: tests/test_gpu_kmeans.py."""
import numpy as np
import pytest

from conftest import load_golden


@pytest.fixture(scope="module")
def blobs():
    return load_golden("kmeans_blobs.npz")


def blob_cases(blobs):
    return [str(t) for t in blobs["cases"]]


def blob_case(blobs, tag):
    K, m, dim, data_seed, seed = (int(v) for v in blobs[f"{tag}/params"])
    data = blobs[f"{tag}/data"]
    assert data.shape == (K * m, dim) and data.dtype == np.float32
    return data, K, seed, blobs[f"{tag}/centre_rows"], blobs[f"{tag}/ref_selected"]


def overlapping(n=600, dim=64, seed=11):
    """The k-center fixture's generator: relu(N(0.16, 0.24^2)), no cluster structure."""
    return np.maximum(np.random.RandomState(seed).normal(0.16, 0.24, size=(n, dim)), 0).astype(np.float32)


def shared_nearest_case():
    """Two centroids whose nearest row is row 2; row 4 is the second centroid's second-nearest."""
    emb = np.array([[10, 0, 0, 0], [0, 10, 0, 0], [1, 1, 0, 0], [0, 0, 10, 0], [1.5, 1, 0, 0], [0, 0, 0, 10]], dtype=np.float32)
    cen = np.array([[1, 1.1, 0, 0], [1.2, 1, 0, 0], [0, 0, 9, 0]], dtype=np.float32)
    return emb, cen, [2, 4, 3]


def test_fixture_selection_equals_the_reference_set(pkg, blobs):
    from unina_yolo_dla_amd import mining
    assert len(blob_cases(blobs)) == 3
    for tag in blob_cases(blobs):
        data, K, seed, centre_rows, ref_sel = blob_case(blobs, tag)
        assert sorted(ref_sel.tolist()) == centre_rows.tolist()          # what the fixture script asserted of the reference
        paths = [f"img_{i}" for i in range(len(data))]
        got = mining.coreset_selection_kmeans(data, paths, K, seed=seed, device=False)
        assert len(got) == K and sorted(got) == sorted(paths[i] for i in ref_sel), tag
        assert sorted(mining.coreset_selection(data, paths, K, method="kmeans", seed=seed, device=False)) == sorted(got)


def test_edge_cases_and_dispatcher(pkg):
    from unina_yolo_dla_amd import mining
    emb = np.arange(32, dtype=np.float32).reshape(8, 4)
    paths = [f"p{i}" for i in range(8)]
    assert mining.coreset_selection_kmeans(emb, paths, 9, seed=0, device=False) == paths           # target_size > n: all paths
    with pytest.raises(ValueError, match="empty dataset"):
        mining.coreset_selection_kmeans(np.zeros((0, 4), np.float32), [], 2, device=False)
    assert sorted(mining.coreset_selection_kmeans(emb, paths, 8, seed=0, device=False)) == paths   # k == n: every row
    want = mining.coreset_selection_kcenter(emb, paths, 3, seed=1, device=False)
    assert mining.coreset_selection(emb, paths, 3, seed=1, device=False) == want                     # default: kcenter
    assert mining.coreset_selection(emb, paths, 3, method="kcenter", seed=1, device=False) == want
    with pytest.raises(ValueError):
        mining.coreset_selection(emb, paths, 3, method="spectral", device=False)


def test_nearest_rows_numpy_gives_a_taken_row_to_nobody_else(pkg):
    from unina_yolo_dla_amd import mining
    emb, cen, want = shared_nearest_case()
    d = np.linalg.norm(emb[:, None] - cen[None], axis=2)
    assert d[:, 0].argmin() == 2 and d[:, 1].argmin() == 2 and np.argsort(d[:, 1])[1] == 4   # the case is what it claims
    assert mining.nearest_rows_numpy(emb, cen).tolist() == want
    # exact tie: the lowest index
    tie = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float32)
    assert mining.nearest_rows_numpy(tie, np.zeros((2, 4), np.float32)).tolist() == [0, 1]


def test_kmeans_numpy_duplicate_init_leaves_the_higher_cluster_empty(pkg):
    from unina_yolo_dla_amd import mining
    emb = overlapping(40, 8)
    emb[7] = emb[3]
    cen, labels, hist, iters, converged = mining.kmeans_numpy(emb, 3, [3, 7, 20], 1)
    assert iters == 1 and not converged and len(hist) == 1
    assert (labels != 1).all() and labels[3] == 0 and labels[7] == 0       # the lowest index wins the exact tie
    assert cen[1].tolist() == emb[7].astype(np.float64).tolist()           # no members: the centroid is kept
    assert np.allclose(cen[0], emb[labels == 0].astype(np.float64).mean(axis=0), rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        mining.kmeans_numpy(emb, 3, [3, 7, 40], 1)


def test_kmeans_numpy_inertia_falls_and_convergence_is_a_fixed_point(pkg):
    from unina_yolo_dla_amd import mining
    emb = overlapping()
    init = mining.kmeans_pp_init(emb, 20, 0)
    cen, labels, hist, iters, converged = mining.kmeans_numpy(emb, 20, init, 200)
    assert converged and 2 <= iters < 200 and len(hist) == iters
    assert (np.diff(hist) <= 1e-12 * hist[:-1]).all(), hist
    assert hist[0] > hist[-1] * 1.01                                        # and it did fall
    assert hist[-1] == pytest.approx(((emb.astype(np.float64) - cen[labels]) ** 2).sum(), rel=1e-12)
    c2, l2, h2, it2, conv2 = mining.kmeans_numpy(emb, 20, None, 5, centroids=cen)
    assert conv2 and it2 == 2 and (l2 == labels).all() and np.array_equal(c2, cen) and h2[0] == h2[1] == hist[-1]
    # a run cut short reports what it did
    c3, l3, h3, it3, conv3 = mining.kmeans_numpy(emb, 20, init, 3)
    assert it3 == 3 and not conv3 and h3.tolist() == hist[:3].tolist()


def test_kmeans_pp_init_is_reproducible_and_leaves_the_global_rng_alone(pkg):
    from unina_yolo_dla_amd import mining
    emb = overlapping(200, 16)
    np.random.seed(99)
    before = np.random.get_state()
    a = mining.kmeans_pp_init(emb, 12, 4)
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]
    assert a.tolist() == mining.kmeans_pp_init(emb, 12, 4).tolist()
    assert a.tolist() != mining.kmeans_pp_init(emb, 12, 5).tolist()
    assert len(set(a.tolist())) == 12 and a.min() >= 0 and a.max() < 200
    assert a[0] == np.random.RandomState(4).randint(200)
    # all rows equal: distinct indices still
    assert sorted(mining.kmeans_pp_init(np.ones((5, 4), np.float32), 5, 0).tolist()) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        mining.kmeans_pp_init(emb, 201, 0)


def test_cli_parser_defaults_to_kcenter_and_names_kmeans_in_the_json(pkg, tmp_path, monkeypatch):
    import json
    from unina_yolo_dla_amd import mine, mining
    from test_mining_cpu import StubEngine
    base = ["--engine", "m.une", "--data", "d"]
    assert mine.parser().parse_args(base).coreset_method == "kcenter"
    assert mine.parser().parse_args(base + ["--coreset-method", "kmeans"]).coreset_method == "kmeans"
    with pytest.raises(SystemExit):
        mine.parser().parse_args(base + ["--coreset-method", "spectral"])
    monkeypatch.setattr(mining, "_device_frame", lambda engine, frame: frame)
    data = tmp_path / "data"
    data.mkdir()
    for i, v in enumerate((0.1, 0.5, 0.9)):
        np.save(data / f"frame{i}.npy", np.full((3, 32, 32), v, dtype=np.float32))
    out, cs = tmp_path / "difficulty_map.json", tmp_path / "coreset.json"
    args = mine.parser().parse_args(["--engine", "m.une", "--data", str(data), "--output", str(out), "--coreset", "2",
                                     "--coreset-output", str(cs), "--coreset-method", "kmeans"])
    args.device_kcenter = False
    mine.run(StubEngine(), args)
    got = json.loads(cs.read_text())
    assert got["method"] == "kmeans" and len(got["paths"]) == 2 and set(got["paths"]) <= {str(data / f"frame{i}.npy") for i in range(3)}


def test_kmeans_entry_points_reject_bad_arguments_without_a_device(pkg):
    """Every UNINA_ERR_ARG case of the header: the checks come before the first HIP call, so no pointer is dereferenced."""
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    lib = engine.load_library()
    ERR_ARG, fake = 4, 0x10000
    good = dict(emb=fake, n=8, dim=4, k=2, init=fake, max_iter=3, cen=fake, lab=fake, hist=fake, it=fake, ws=fake)

    def km(**kw):
        a = dict(good, **kw)
        return lib.unina_kmeans(a["emb"], a["n"], a["dim"], a["k"], a["init"], a["max_iter"], a["cen"], a["lab"], a["hist"], a["it"], a["ws"], None)

    for bad in (dict(emb=None), dict(cen=None), dict(lab=None), dict(it=None), dict(emb=fake + 4), dict(cen=fake + 8), dict(ws=fake + 8),
                dict(hist=fake + 4), dict(lab=fake + 2), dict(init=fake + 1), dict(dim=6), dict(dim=0), dict(k=0), dict(k=9), dict(max_iter=0),
                dict(n=0, k=0)):
        assert km(**bad) == ERR_ARG, bad
    nr = lib.unina_nearest_rows
    assert nr(None, 8, 4, fake, 2, fake, None, None) == ERR_ARG
    assert nr(fake, 8, 4, None, 2, fake, None, None) == ERR_ARG
    assert nr(fake, 8, 4, fake, 2, None, None, None) == ERR_ARG
    assert nr(fake + 4, 8, 4, fake, 2, fake, None, None) == ERR_ARG
    assert nr(fake, 8, 4, fake + 4, 2, fake, None, None) == ERR_ARG
    assert nr(fake, 8, 6, fake, 2, fake, None, None) == ERR_ARG
    assert nr(fake, 8, 4, fake, 0, fake, None, None) == ERR_ARG
    assert nr(fake, 8, 4, fake, 9, fake, None, None) == ERR_ARG
    assert lib.unina_kmeans_workspace_bytes(8, 6, 2) == 0 and lib.unina_kmeans_workspace_bytes(8, 4, 9) == 0
    ws = lib.unina_kmeans_workspace_bytes(100000, 256, 1000)
    assert ws % 16 == 0 and 4000 < ws < (1 << 20)
