"""GPU tests of the k-means coreset (csrc/kmeans.hip behind unina_kmeans / unina_nearest_rows), through the C ABI.

Every bound here is derived, none is fitted to the kernels: u = 2^-24, gamma(m) = m u / (1 - m u) (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1). The f32-input MFMA is a d-ordered fmaf chain, so <x, c> over `dim` terms carries at
most gamma(dim) sum|x c|; |c|^2 (fmaf chains + a 6-level tree) and the final fmaf(-2, dot, |c|^2) add two more roundings:
the score |c_j|^2 - 2 <x_i, c_j> is within tol(i, j) / 2 of its exact value with
    tol(i, j) = 2 gamma(dim + 2) (2 sum_d |x_id c_jd| + sum_d c_jd^2),
and a label can differ from the float64 arg-min only by a centroid whose distance is within tol(i, label) + tol(i, best).
The bounds restated, and the slack measured under them once a GPU run is made: profiles/r04/kmeans_bound.txt."""

import numpy as np
import pytest

from conftest import load_golden
from kmeans_cases import one_step_case
from test_kmeans_cpu import blob_case, blob_cases, overlapping, shared_nearest_case
from test_mining_cpu import kcenter_data

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CONVERGED = 1 << 30
ERR_ARG = 4
SHAPES = [(1, 4, 1), (37, 24, 5), (300, 256, 48), (1000, 40, 130), (257, 8, 257)]


def gamma(m):
    return m * U / (1.0 - m * U)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def blobs():
    return load_golden("kmeans_blobs.npz")


@pytest.fixture(scope="module")
def overlap():
    """(600, 64) overlapping data and a 20-row k-means++ start, shared by the loop tests (never written to)."""
    from unina_yolo_dla_amd import mining
    emb = overlapping()
    return emb, mining.kmeans_pp_init(emb, 20, 0)


def raw_kmeans(torch, emb, k, max_iter, init_rows=None, centroids=None, workspace=True, history=True):
    """unina_kmeans itself: (centroids, labels, history [max_iter], raw d_iters) as host arrays, nothing trimmed.
    history=False passes d_inertia_history = NULL and returns None in its place."""
    from unina_yolo_dla_amd import engine
    L = engine.load_library()
    # (np.array: a copy, the constructed cases are read-only arrays)
    x = emb if isinstance(emb, torch.Tensor) else torch.from_numpy(np.array(emb, dtype=np.float32, order="C")).cuda()
    n, d = x.shape
    init = None if init_rows is None else torch.from_numpy(np.asarray(init_rows, dtype=np.int32)).cuda()
    cen = torch.zeros((k, d), dtype=torch.float32, device="cuda") if centroids is None else \
        torch.from_numpy(np.array(centroids, dtype=np.float32, order="C")).cuda()
    labels = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    hist = torch.full((max_iter,), 3.0, dtype=torch.float64, device="cuda") if history else None
    iters = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.unina_kmeans_workspace_bytes(n, d, k), dtype=torch.uint8, device="cuda") if workspace else None
    rc = L.unina_kmeans(x.data_ptr(), n, d, k, None if init is None else init.data_ptr(), max_iter, cen.data_ptr(), labels.data_ptr(),
                        None if hist is None else hist.data_ptr(), iters.data_ptr(), None if ws is None else ws.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return cen.cpu().numpy(), labels.cpu().numpy(), None if hist is None else hist.cpu().numpy(), int(iters.cpu()[0])


def check_one_step(torch, emb, start, what=None):
    """max_iter = 1 from given centroids, every stage against float64 on the device's own inputs: labels (tol above),
    centroids (a sequential fp32 sum of `count` terms and one division: gamma(count + 1) * mean_members |x| per channel),
    inertia (double on the device: 1e-6 relative). Prints the slack under each bound; returns the device's labels."""
    (n, dim), k = emb.shape, len(start)
    cen, labels, hist, iters = raw_kmeans(torch, emb, k, 1, centroids=start)
    assert iters == 1 and labels.min() >= 0 and labels.max() < k
    x, c = emb.astype(np.float64), start.astype(np.float64)
    d2 = np.stack([((x - cj) ** 2).sum(axis=1) for cj in c], axis=1)
    tol = 2.0 * gamma(dim + 2) * (2.0 * (np.abs(x) @ np.abs(c).T) + (c * c).sum(axis=1)[None, :])
    rows = np.arange(n)
    best = d2.argmin(axis=1)
    allowed = tol[rows, labels] + tol[rows, best]
    excess = d2[rows, labels] - d2[rows, best]
    what = f"({n},{dim},{k})" if what is None else f"{what} ({n},{dim},{k})"
    print(f"{what} labels: {int((labels != best).sum())} differ from the float64 arg-min; "
          f"worst excess / allowed {float((excess / allowed).max()):.3g}")
    assert (excess <= allowed).all(), (n, dim, k, float((excess / allowed).max()))
    gap = d2 - d2[rows, best][:, None] - tol - tol[rows, best][:, None]      # > 0: centroid j cannot win row i
    gap[rows, best] = np.inf
    sure = (gap > 0).all(axis=1)
    assert (labels[sure] == best[sure]).all()
    assert sure.mean() > 0.9, sure.mean()                          # the equality check covers the data
    # centroid update from the DEVICE's labels
    counts = np.bincount(labels, minlength=k)
    worst = 0.0
    for j in range(k):
        if counts[j] == 0:
            assert cen[j].tobytes() == start[j].tobytes(), j
            continue
        members = x[labels == j]
        bound = gamma(counts[j] + 1) * np.abs(members).mean(axis=0)
        err = np.abs(cen[j].astype(np.float64) - members.mean(axis=0))
        assert (err <= bound).all(), (j, counts[j], float(err.max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    want = float(((x - cen.astype(np.float64)[labels]) ** 2).sum())
    rel = abs(hist[0] - want) / max(want, 1e-300)
    print(f"{what} centroids: worst error / bound {worst:.3g}; inertia: relative error {rel:.3g} (bound 1e-6)")
    assert rel <= 1e-6, (hist[0], want)
    return labels


@pytest.mark.parametrize("n,dim,k", SHAPES)
def test_one_step_against_float64(pkg, torch_cuda, n, dim, k):
    check_one_step(torch_cuda, *one_step_case(n, dim, k))


def test_exact_ties_and_empty_clusters(pkg, torch_cuda):
    """Identical start centroids at indices that meet in every place the arg-min is combined -- 0 / 4: the two lane halves
    of one accumulator tile; 1 / 33: two tiles of a chunk; 2 / 129: two chunks -- the lowest index takes every member, the
    other cluster counts 0 and its centroid keeps its bits."""
    rng = np.random.RandomState(8)
    n, dim, k = 400, 12, 130
    emb = np.maximum(rng.normal(0.16, 0.24, size=(n, dim)), 0).astype(np.float32)
    init = rng.permutation(n)[:k]
    for low, high in ((0, 4), (1, 33), (2, 129)):
        emb[init[high]] = emb[init[low]]
    cen, labels, hist, iters = raw_kmeans(torch_cuda, emb, k, 1, init_rows=init)
    counts = np.bincount(labels, minlength=k)
    for low, high in ((0, 4), (1, 33), (2, 129)):
        assert counts[high] == 0 and counts[low] >= 2, (low, high, counts[low], counts[high])
        assert labels[init[high]] == low and labels[init[low]] == low
        assert cen[high].tobytes() == emb[init[high]].tobytes()
    # the start rows are their own nearest centroid (distance 0 against >> tol): the float64 arg-min, lowest index on ties
    x = emb.astype(np.float64)
    want = np.stack([((x - cj) ** 2).sum(axis=1) for cj in x[init]], axis=1).argmin(axis=1)
    assert (labels[init] == want[init]).all()
    # two clusters, one start: everything belongs to cluster 0
    two = np.maximum(rng.normal(0.16, 0.24, size=(70, 8)), 0).astype(np.float32)
    two[1] = two[0]
    cen, labels, _, _ = raw_kmeans(torch_cuda, two, 2, 1, init_rows=[0, 1])
    assert (labels == 0).all() and cen[1].tobytes() == two[1].tobytes()
    np.testing.assert_allclose(cen[0], two.astype(np.float64).mean(axis=0), rtol=gamma(71), atol=0)


def test_one_call_equals_chained_calls_and_two_runs_agree(pkg, torch_cuda, overlap):
    emb, init = overlap
    x = torch_cuda.from_numpy(emb).cuda()
    T = 4
    cen, labels, hist, iters = raw_kmeans(torch_cuda, x, 20, T, init_rows=init)
    assert iters == T                                                        # (not converged yet: overlapping data)
    again = raw_kmeans(torch_cuda, x, 20, T, init_rows=init, workspace=False)   # and with the call's own workspace
    assert cen.tobytes() == again[0].tobytes() and labels.tobytes() == again[1].tobytes() and hist.tobytes() == again[2].tobytes()
    assert iters == again[3]
    c, chain_hist, chain_iters = None, [], 0
    for t in range(T):
        c, lab, h, it = raw_kmeans(torch_cuda, x, 20, 1, init_rows=init if t == 0 else None, centroids=c)
        chain_hist.append(h[0])
        chain_iters += it
    assert c.tobytes() == cen.tobytes() and lab.tobytes() == labels.tobytes()
    assert np.asarray(chain_hist).tobytes() == hist.tobytes() and chain_iters == iters


def test_loop_converges_and_later_iterations_do_nothing(pkg, torch_cuda, overlap):
    from unina_yolo_dla_amd import engine
    emb, init = overlap
    x = torch_cuda.from_numpy(emb).cuda()
    max_iter = 100
    cen, labels, hist, iters = raw_kmeans(torch_cuda, x, 20, max_iter, init_rows=init)
    assert iters & CONVERGED
    done = iters & (CONVERGED - 1)
    assert 2 <= done < max_iter
    assert np.isfinite(hist[:done]).all() and np.isnan(hist[done:]).all()     # not executed: never written after the NaN fill
    assert (np.diff(hist[:done]) <= 1e-6 * hist[:done - 1]).all(), hist[:done]
    assert hist[done - 1] < hist[0]
    print(f"overlapping (600,64,20): converged after {done} iterations, inertia {hist[0]:.6g} -> {hist[done - 1]:.6g}")
    # the state is a fixed point, and the last executed iteration changed nothing: one more step from it gives the same bytes
    c1, l1, h1, it1 = raw_kmeans(torch_cuda, x, 20, 1, centroids=cen)
    assert c1.tobytes() == cen.tobytes() and l1.tobytes() == labels.tobytes() and h1[0] == hist[done - 1]
    assert hist[done - 1] == hist[done - 2]
    # a loop cut before that is the same trajectory
    c3, l3, h3, it3 = raw_kmeans(torch_cuda, x, 20, done - 1, init_rows=init)
    assert it3 == done - 1 and h3.tobytes() == hist[:done - 1].tobytes()
    # the Python entry trims the history and splits the flag
    pc, pl, ph, pit, pconv = engine.kmeans(x, 20, init_rows=init, max_iter=max_iter)
    assert pconv and pit == done and ph.tobytes() == hist[:done].tobytes() and pc.tobytes() == cen.tobytes()
    assert pl.dtype == np.int64 and (pl == labels).all()


def test_blob_fixture_labels_equal_the_float64_twin(pkg, torch_cuda, blobs):
    """Decision margins of the fixture are > 1e-3 relative at convergence and larger on the way (the starts are blob rows),
    far above tol: the device must walk the float64 trajectory label for label."""
    from unina_yolo_dla_amd import engine, mining
    for tag in blob_cases(blobs):
        data, K, seed, centre_rows, ref_sel = blob_case(blobs, tag)
        init = mining.kmeans_pp_init(data, K, seed)
        wc, wl, wh, wit, wconv = mining.kmeans_numpy(data, K, init, 100)
        cen, labels, hist, iters, conv = engine.kmeans(data, K, init_rows=init, max_iter=100)
        assert conv and wconv and iters == wit, (tag, iters, wit)
        assert (labels == wl).all(), tag
        np.testing.assert_allclose(hist, wh, rtol=1e-5)
        np.testing.assert_allclose(cen, wc, rtol=0, atol=gamma(len(data) + 1) * np.abs(data).max())
        # selection on the device = the reference's loop on the same centroids
        assert engine.nearest_rows(data, cen).tolist() == mining.nearest_rows_numpy(data, cen).tolist()


def test_nearest_rows_gives_a_taken_row_to_nobody_else(pkg, torch_cuda):
    from unina_yolo_dla_amd import engine
    emb, cen, want = shared_nearest_case()
    assert engine.nearest_rows(emb, cen).tolist() == want
    assert engine.nearest_rows(torch_cuda.from_numpy(emb).cuda(), torch_cuda.from_numpy(cen).cuda()).tolist() == want
    tie = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float32)
    assert engine.nearest_rows(tie, np.zeros((2, 4), np.float32)).tolist() == [0, 1]
    assert engine.nearest_rows(tie, tie).tolist() == [0, 1, 2]                 # k == n


def test_end_to_end_selects_the_reference_set(pkg, torch_cuda, blobs):
    from unina_yolo_dla_amd import mining
    for tag in blob_cases(blobs):
        data, K, seed, centre_rows, ref_sel = blob_case(blobs, tag)
        paths = [f"img_{i}" for i in range(len(data))]
        got = mining.coreset_selection_kmeans(data, paths, K, seed=seed, device=True)
        assert len(got) == K and sorted(got) == sorted(paths[i] for i in ref_sel), tag
    gold = load_golden("mining_seed1234.npz")
    emb, k, seed = kcenter_data(gold)
    paths = [str(i) for i in range(len(emb))]
    assert mining.coreset_selection(emb, paths, k, method="kcenter", seed=seed) == [paths[i] for i in gold["kcenter/selected"]]


def test_argument_errors_and_bad_init_row(pkg, torch_cuda):
    from unina_yolo_dla_amd import engine
    L = engine.load_library()
    torch = torch_cuda
    n, d, k = 40, 8, 3
    x = torch.from_numpy(overlapping(n, d)).cuda()
    cen = torch.full((k, d), 7.0, dtype=torch.float32, device="cuda")
    labels = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    hist = torch.full((4,), 3.0, dtype=torch.float64, device="cuda")
    iters = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    init = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    ws = torch.empty(L.unina_kmeans_workspace_bytes(n, d, k), dtype=torch.uint8, device="cuda")
    sel = torch.zeros(k, dtype=torch.int32, device="cuda")
    X, CEN, LAB, HIST, IT, INIT, WS, SEL = (t.data_ptr() for t in (x, cen, labels, hist, iters, init, ws, sel))

    def km(emb=X, n=n, dim=d, k=k, init=INIT, max_iter=4, cen=CEN, lab=LAB, hist=HIST, it=IT, ws=WS):
        return L.unina_kmeans(emb, n, dim, k, init, max_iter, cen, lab, hist, it, ws, None)

    for bad in (dict(emb=None), dict(cen=None), dict(lab=None), dict(it=None), dict(emb=X + 4), dict(cen=CEN + 4), dict(ws=WS + 8),
                dict(hist=HIST + 4), dict(dim=6), dict(k=0), dict(k=n + 1), dict(max_iter=0), dict(n=0)):
        assert km(**bad) == ERR_ARG, bad
    assert L.unina_kmeans_workspace_bytes(n, 6, k) == 0 and L.unina_kmeans_workspace_bytes(n, d, n + 1) == 0

    def nr(emb=X, n=n, dim=d, cen=CEN, k=k, sel=SEL, ws=None):
        return L.unina_nearest_rows(emb, n, dim, cen, k, sel, ws, None)

    for bad in (dict(emb=None), dict(cen=None), dict(sel=None), dict(emb=X + 4), dict(cen=CEN + 8), dict(dim=6), dict(k=0), dict(k=n + 1)):
        assert nr(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert float(cen.min()) == 7.0 and int(labels.max()) == -5 and int(iters[0]) == -9   # refused calls wrote nothing
    # an init row outside [0, n): found on the device, reported through d_iters, outputs untouched, no fault
    for rows in ([0, n, 2], [0, 1, -1]):
        init.copy_(torch.tensor(rows, dtype=torch.int32))
        iters.fill_(-9)
        assert km() == 0
        torch.cuda.synchronize()
        assert int(iters[0]) == -1
        assert float(cen.min()) == 7.0 and float(cen.max()) == 7.0 and int(labels.min()) == -5 and int(labels.max()) == -5
        assert float(hist.min()) == 3.0 and float(hist.max()) == 3.0
    with pytest.raises(engine.EngineError, match="init row"):
        engine.kmeans(x, k, init_rows=[0, n, 2], max_iter=2)
    # and a good call on the same buffers afterwards works
    init.copy_(torch.tensor([0, 1, 2], dtype=torch.int32))
    assert km() == 0
    torch.cuda.synchronize()
    assert int(iters[0]) > 0 and int(labels.min()) >= 0 and int(labels.max()) < k
