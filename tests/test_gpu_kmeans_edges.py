"""The Lloyd loop at its kernels' edges (-m gpu): the constructed cases of tests/kmeans_cases.py through unina_kmeans
(csrc/kmeans.hip), and the `stream=` argument of the selection wrappers. What the cases contain, and that a kernel which skips
the edge cannot pass them, is proved on the CPU by tests/test_kmeans_cases_cpu.py.

Which edge a case drives:
    one step    dim 260 / 512: the second trip of the lane loops of kmeans_norms_kernel and kmeans_inertia_kernel, the second
                channel block of kmeans_update_kernel, a padded K step behind eight full ones; n 2081: the second trip of
                kmeans_finish_kernel; n 32805: the inertia's block cap; k 31 .. 33 and 127 .. 129: the last MFMA tile and the
                last chunk of kmeans_assign_kernel; n 127 .. 129 and 255 .. 257: its row guard and the update's label scan
    planted     tail260 / tail512 (the answer only behind channel 256), last_centroid(k) (every index the nearest of a sure
                row), offset32 (the cancellation in |c|^2 - 2 <x, c>)
    ties        the lower index in lane half 1, on a tile seam, on a chunk seam
    loop        convergence exactly in the max_iter-th iteration, one before, one behind; no history; a centroid that is empty
                in every iteration
    non-finite  the rule of include/unina_mi355.h, three iterations against the twin
    streams     engine.kmeans / nearest_rows / kcenter on a side stream while the current stream is busy
No tolerance is new: one step is held by test_gpu_kmeans.check_one_step (labels under tol, centroids under gamma(count + 1) *
mean|x|, inertia 1e-6 relative), everything else is equality. Measured slack: profiles/r04/kmeans_edges_bound.txt."""
import numpy as np
import pytest

import kmeans_cases as kc
from test_gpu_kmeans import CONVERGED, check_one_step, raw_kmeans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("n,dim,k", kc.ONE_STEP_SHAPES)
def test_one_step_at_the_edges_against_float64(pkg, torch_cuda, n, dim, k):
    check_one_step(torch_cuda, *kc.one_step_case(n, dim, k))


PLANTED = {"tail260": kc.tail260, "tail512": kc.tail512, "offset32": kc.offset32}
PLANTED.update({f"last_centroid({k})": (lambda k=k: kc.last_centroid(k)) for k in kc.LAST_KS})


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_cases_against_float64_and_the_plant(pkg, torch_cuda, name):
    emb, start, plant = PLANTED[name]()
    labels = check_one_step(torch_cuda, emb, start, what=name)
    assert (labels == plant).all(), (name, np.flatnonzero(labels != plant)[:8], labels[labels != plant][:8])


def test_exact_ties_in_both_lane_halves_and_on_the_seams(pkg, torch_cuda):
    """The lower index takes every member whichever lane half, tile or chunk it sits in; the higher cluster counts 0 and its
    centroid keeps its start bits."""
    emb, init = kc.tie_case()
    cen, labels, hist, iters = raw_kmeans(torch_cuda, emb, kc.TIE_K, 1, init_rows=init)
    assert iters == 1
    counts = np.bincount(labels, minlength=kc.TIE_K)
    for low, high in kc.TIE_PAIRS:
        assert counts[high] == 0 and counts[low] >= 2, (low, high, counts[low], counts[high])
        assert labels[init[high]] == low and labels[init[low]] == low, (low, high)
        assert cen[high].tobytes() == emb[init[high]].tobytes(), (low, high)
    # a start row is its own nearest centroid (distance 0 against >> tol): the float64 arg-min, lowest index on ties
    x = emb.astype(np.float64)
    want = np.stack([((x - cj) ** 2).sum(axis=1) for cj in x[init]], axis=1).argmin(axis=1)
    assert (labels[init] == want[init]).all()


def test_convergence_in_the_last_iteration_one_before_and_one_behind(pkg, torch_cuda):
    emb, init, (wc, wl, wh, T, wconv) = kc.loop_case()
    assert wconv and T >= 4
    x = torch_cuda.tensor(emb, device="cuda")
    cen, labels, hist, iters = raw_kmeans(torch_cuda, x, kc.LOOP_K, T, init_rows=init)
    assert iters == T | CONVERGED, (iters & (CONVERGED - 1), T)              # the flag set by the very last finish kernel
    assert hist.shape == (T,) and np.isfinite(hist).all()
    assert (labels == wl).all()
    want = float(((emb.astype(np.float64) - cen.astype(np.float64)[labels]) ** 2).sum())
    assert abs(hist[-1] - want) <= 1e-6 * want and hist[-1] == hist[-2]
    # one more iteration enqueued: nothing behind the flag runs
    c2, l2, h2, it2 = raw_kmeans(torch_cuda, x, kc.LOOP_K, T + 1, init_rows=init)
    assert it2 == iters and c2.tobytes() == cen.tobytes() and l2.tobytes() == labels.tobytes()
    assert h2[:T].tobytes() == hist.tobytes() and np.isnan(h2[T])
    # one fewer: the same trajectory, and no bit
    c3, l3, h3, it3 = raw_kmeans(torch_cuda, x, kc.LOOP_K, T - 1, init_rows=init)
    assert it3 == T - 1 and h3.tobytes() == hist[:T - 1].tobytes()
    # d_inertia_history = NULL
    for max_iter, (c, l, it) in ((T, (cen, labels, iters)), (T + 1, (c2, l2, it2)), (T - 1, (c3, l3, it3))):
        cn, ln, hn, itn = raw_kmeans(torch_cuda, x, kc.LOOP_K, max_iter, init_rows=init, history=False)
        assert hn is None and itn == it and cn.tobytes() == c.tobytes() and ln.tobytes() == l.tobytes(), max_iter


def test_a_centroid_far_from_all_data_keeps_its_bits_through_the_loop(pkg, torch_cuda):
    emb, start, (wc, wl, wh, T, wconv) = kc.far_case()
    cen, labels, hist, iters = raw_kmeans(torch_cuda, emb, kc.LOOP_K, T, centroids=start)
    assert iters == T | CONVERGED
    assert cen[kc.FAR_INDEX].tobytes() == start[kc.FAR_INDEX].tobytes()
    assert (labels != kc.FAR_INDEX).all() and (labels == wl).all()
    others = np.arange(kc.LOOP_K) != kc.FAR_INDEX
    assert (np.bincount(labels, minlength=kc.LOOP_K)[others] > 0).all()      # (it is the only empty one)


def test_nonfinite_values_follow_the_rule_of_the_header(pkg, torch_cuda):
    """A NaN score never wins; a row all of whose scores are NaN or +inf takes label 0; nothing is validated. Labels and
    d_iters equal the twin's after one, two and three iterations; the history is NaN where the twin's is."""
    from unina_yolo_dla_amd import mining
    emb, init = kc.nonfinite()
    for t in range(1, kc.NONFINITE_ITERS + 1):
        wc, wl, wh, wit, wconv = mining.kmeans_numpy(emb, 3, init, t)
        cen, labels, hist, iters = raw_kmeans(torch_cuda, emb, 3, t, init_rows=init)
        assert iters == wit | (CONVERGED if wconv else 0), (t, iters, wit, wconv)
        assert (labels == wl).all(), (t, labels, wl)
        done = wit
        assert np.array_equal(np.isnan(hist[:done]), np.isnan(wh)), (t, hist, wh)
        fin = ~np.isnan(wh)
        assert (np.abs(hist[:done][fin] - wh[fin]) <= 1e-6 * np.abs(wh[fin])).all()
        assert np.isnan(hist[done:]).all()
        assert np.array_equal(np.isnan(cen), np.isnan(wc)) and np.array_equal(np.isinf(cen), np.isinf(wc)), t
        print(f"non-finite, {t} iterations: cluster sizes {np.bincount(labels, minlength=3).tolist()}, history {hist.tolist()}")


def keep_busy(torch, big, fills):
    """Ordinary fills of `big` on the current stream and an event behind them; the caller asserts it has not fired yet."""
    for i in range(fills):
        big.fill_(float(i))
    ev = torch.cuda.Event()
    ev.record()
    return ev


def test_side_stream_waits_for_the_current_streams_initialisation(pkg, torch_cuda):
    """engine.kmeans / nearest_rows / kcenter create and initialise their tensors (zeros, the clone of the start centroids) on
    the current stream and launch on `stream`. With the current stream busy those initialisations land late: unordered, the
    kernels read the centroids before the clone and the zero fills wipe what they wrote. The side-stream results must be
    the default-stream bytes."""
    from unina_yolo_dla_amd import engine
    torch = torch_cuda
    emb, init, _ = kc.loop_case()
    k = kc.LOOP_K
    x = torch.tensor(emb, device="cuda")
    start = torch.tensor(emb[init], device="cuda")
    want = engine.kmeans(x, k, centroids=start, max_iter=4)
    cen = torch.from_numpy(want[0]).cuda()
    want_rows = engine.nearest_rows(x, cen)
    want_kc = engine.kcenter(x, k, 3)
    assert len(set(want_rows.tolist())) == k and len(set(want_kc.tolist())) == k      # (not the zeros of an unwritten result)
    side = torch.cuda.Stream()
    big = torch.empty(128 << 20, dtype=torch.float32, device="cuda")        # 512 MiB a fill: 300 fills are some tens of ms
    fills = 300
    torch.cuda.synchronize()

    ev = keep_busy(torch, big, fills)
    assert not ev.query()                                                    # the current stream is still busy at the call
    got = engine.kmeans(x, k, centroids=start, max_iter=4, stream=side)
    assert got[3] == want[3] and got[4] == want[4], (got[3], want[3])
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert start.cpu().numpy().tobytes() == emb[init].tobytes()              # the caller's start matrix is not written

    ev = keep_busy(torch, big, fills)
    assert not ev.query()
    got = engine.kmeans(x, k, init_rows=init, max_iter=4, stream=side.cuda_stream)    # a raw handle
    assert got[3] == want[3] and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()

    ev = keep_busy(torch, big, fills)
    assert not ev.query()
    assert engine.nearest_rows(x, cen, stream=side).tolist() == want_rows.tolist()

    ev = keep_busy(torch, big, fills)
    assert not ev.query()
    assert engine.kcenter(x, k, 3, stream=side).tolist() == want_kc.tolist()
    torch.cuda.synchronize()
