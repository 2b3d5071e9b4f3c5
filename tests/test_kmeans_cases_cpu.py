"""What the constructed cases of tests/kmeans_cases.py contain, proved on the float64 twin without a device: every plant is
invisible to a kernel that skips the edge it sits behind, and visible to one that does not."""
import numpy as np
import pytest

import kmeans_cases as kc


def twin_labels(pkg, emb, start):
    from unina_yolo_dla_amd import mining
    return mining.kmeans_numpy(emb, len(start), None, 1, centroids=start)[1]


@pytest.mark.parametrize("case", [kc.tail260, kc.tail512], ids=["tail260", "tail512"])
def test_tail_cases_carry_their_signal_only_behind_channel_256(pkg, case):
    emb, start, plant = case()
    k = len(start)
    head = kc.LANE_TRIP
    assert (emb[:, :head] == emb[0, :head]).all() and (start[:, :head] == emb[0, :head]).all()
    assert (twin_labels(pkg, *without_tail(case)) == 0).all()                # no tail: k equal centroids, the lowest index
    assert (twin_labels(pkg, emb, start) == plant).all() and (np.bincount(plant) > 0).all()
    d2, tol, best, sure = kc.one_step_reference(emb, start)
    assert (best == plant).all() and sure.all()
    # each kernel's lost tail, one at a time, in float64
    x, c = emb.astype(np.float64), start.astype(np.float64)
    full_dot, head_dot = x @ c.T, x[:, :head] @ c[:, :head].T
    full_norm, head_norm = (c * c).sum(axis=1), (c[:, :head] ** 2).sum(axis=1)
    assert ((head_norm[None] - 2.0 * full_dot).argmin(axis=1) == k - 1).all()          # norms: the longest centroid takes all
    assert ((full_norm[None] - 2.0 * head_dot).argmin(axis=1) == 0).all()              # assign: the shortest centroid takes all
    # update: the start's tail is 10 000 centroid bounds at least from the members' mean
    for j in range(k):
        members = x[plant == j]
        bound = kc.gamma(len(members) + 1) * np.abs(members).mean(axis=0)
        assert (np.abs(c[j] - members.mean(axis=0))[head:] > 1e4 * bound[head:]).all()
    # inertia: the tail is all of it but the rounding of the head's fp32 mean
    mean = np.stack([x[plant == j].mean(axis=0) for j in range(k)])
    diff = (x - mean[plant]) ** 2
    assert diff[:, head:].sum() > 0.999999 * diff.sum() and diff[:, head:].sum() > 1e-3


def without_tail(case):
    emb, start, _ = kc.without_tail(case())
    return emb, start


@pytest.mark.parametrize("k", kc.LAST_KS)
def test_last_centroid_cases_lose_a_label_with_the_last_centroid(pkg, k):
    emb, start, plant = kc.last_centroid(k)
    assert (kc.MFMA_TILE - 1 in kc.LAST_KS) and (kc.TILE_C + 1 in kc.LAST_KS)
    labels = twin_labels(pkg, emb, start)
    assert (labels == plant).all() and (np.bincount(labels, minlength=k) >= 1).all()
    short = twin_labels(pkg, emb, start[:k - 1])
    assert (short != labels).sum() >= 1 and (short[labels != k - 1] == labels[labels != k - 1]).all()


def test_offset32_cancels_and_stays_sure(pkg):
    emb, start, plant = kc.offset32()
    d2, tol, best, sure = kc.one_step_reference(emb, start)
    assert sure.all() and (best == plant).all() and (twin_labels(pkg, emb, start) == plant).all()
    c = start.astype(np.float64)
    scores = (c * c).sum(axis=1)[None] - 2.0 * emb.astype(np.float64) @ c.T
    spread = np.sort(scores, axis=1)
    assert 5e4 < np.abs(scores).min() and np.abs(scores).max() < 8e4
    assert (spread[:, 1] - spread[:, 0]).min() < 1e-3 * np.abs(scores).min()           # the decision is in the last 1e-3 of a score
    assert (spread[:, 1] - spread[:, 0]).min() > 4.0 * tol.max()                       # (d2 gap = score gap) and still sure


@pytest.mark.parametrize("n,dim,k", kc.ONE_STEP_SHAPES)
def test_one_step_shapes_are_sure_and_leave_no_cluster_empty(pkg, n, dim, k):
    emb, start = kc.one_step_case(n, dim, k)
    d2, tol, best, sure = kc.one_step_reference(emb, start)
    assert sure.mean() > 0.9, sure.mean()
    assert (np.bincount(best, minlength=k) > 0).all()
    assert (best == twin_labels(pkg, emb, start))[sure].all()


def test_one_step_shapes_reach_the_branches_they_name():
    shapes = set(kc.ONE_STEP_SHAPES)
    assert any(kc.LANE_TRIP < dim < kc.LANE_TRIP + kc.TILE_D and dim % kc.TILE_D for _, dim, _ in shapes)    # 260
    assert any(dim >= 2 * kc.LANE_TRIP for _, dim, _ in shapes)
    assert any(4 * ((n + 31) // 32) > kc.BLOCK for n, _, _ in shapes if n < 32768)
    assert any((n + 31) // 32 > kc.INERTIA_MAX_BLOCKS for n, _, _ in shapes)
    for edge, axis in ((kc.MFMA_TILE, 2), (kc.TILE_C, 2), (kc.TILE_R, 0), (kc.BLOCK, 0)):
        assert {edge - 1, edge, edge + 1} <= {s[axis] for s in shapes}, (edge, axis)


def test_tie_pairs_tie_bit_for_bit_and_sit_where_they_say(pkg):
    emb, init = kc.tie_case()
    x = emb.astype(np.float64)
    c = x[init]
    scores = (c * c).sum(axis=1)[None] - 2.0 * x @ c.T
    used = [i for pair in kc.TIE_PAIRS for i in pair]
    assert len(set(used)) == len(used)
    for low, high in kc.TIE_PAIRS:
        assert low < high and c[low].tobytes() == c[high].tobytes()
        assert scores[:, low].tobytes() == scores[:, high].tobytes()
    # a duplicated start row's nearest centroid is the pair (distance 0), so the tie decides a label
    labels = twin_labels(pkg, emb, emb[init])
    for low, high in kc.TIE_PAIRS:
        assert labels[init[low]] == low and labels[init[high]] == low and (labels != high).all()
    half = lambda j: (j % kc.MFMA_TILE >> 2) & 1
    tile = lambda j: j // kc.MFMA_TILE
    chunk = lambda j: j // kc.TILE_C
    where = {pair: (half(pair[0]), half(pair[1]), tile(pair[0]) == tile(pair[1]), chunk(pair[0]) == chunk(pair[1])) for pair in kc.TIE_PAIRS}
    assert where[0, 4] == (0, 1, True, True) and where[3, 7] == (0, 1, True, True)
    assert where[5, 8] == (1, 0, True, True)                                 # the lower index in lane half 1
    assert where[1, 33][2:] == (False, True) and where[2, 129][3] is False
    assert where[31, 32] == (1, 0, False, True) and where[63, 64] == (1, 0, False, True)
    assert where[127, 128] == (1, 0, False, False)


def test_loop_case_takes_several_iterations_and_every_decision_is_clear(pkg):
    emb, init, (cen, labels, hist, iters, converged) = kc.loop_case()
    assert emb.shape == (kc.LOOP_K * kc.LOOP_ROWS_PER_BLOB, kc.LOOP_DIM) and converged
    assert iters >= 4 and len(hist) == iters, iters                         # iters - 1 can still not report convergence early
    assert (np.diff(hist) <= 0).all() and hist[-1] == hist[-2]
    assert kc.trajectory_margin(emb, emb[init], iters) > kc.LOOP_MARGIN
    # cut one short: the same trajectory, not converged
    from unina_yolo_dla_amd import mining
    c1, l1, h1, it1, conv1 = mining.kmeans_numpy(emb, kc.LOOP_K, init, iters - 1)
    assert it1 == iters - 1 and not conv1 and h1.tolist() == hist[:-1].tolist() and (l1 == labels).all()


def test_far_centroid_is_empty_in_every_iteration(pkg):
    emb, start, (cen, labels, hist, iters, converged) = kc.far_case()
    assert converged and iters >= 3
    c = start.astype(np.float64)
    for _ in range(iters):
        c, lab, _ = kc.step64(emb, c)
        assert (lab != kc.FAR_INDEX).all()
    assert (lab == labels).all() and cen[kc.FAR_INDEX].tolist() == start[kc.FAR_INDEX].astype(np.float64).tolist()
    assert kc.trajectory_margin(emb, start, iters) > kc.LOOP_MARGIN


def test_nonfinite_case_follows_the_rule_in_every_iteration(pkg):
    """The rule of include/unina_mi355.h: a NaN score never wins; a row all of whose scores are NaN or +inf takes label 0."""
    emb, init = kc.nonfinite()
    assert emb.shape == (40, 8) and np.isnan(emb[kc.NAN_ROW]).sum() == 1 and np.isinf(emb[kc.INF_ROW]).sum() == 1
    assert np.isfinite(np.delete(emb, [kc.NAN_ROW, kc.INF_ROW], axis=0)).all()
    c = emb[init].astype(np.float64)
    seen = []
    for t in range(kc.NONFINITE_ITERS):
        want = kc.rule_labels(emb, c)
        c, labels, inertia = kc.step64(emb, c)
        assert (labels == want).all(), (t, labels, want)
        assert labels[kc.NAN_ROW] == 0 and np.isnan(inertia)
        seen.append(labels)
    assert np.isnan(c[0]).any()
    # iteration 2 is where numpy's plain arg-min (the first NaN) and the rule part: nobody but the NaN row stays in cluster 0
    assert (seen[0] == 0).sum() > 1 and (seen[1] == 0).sum() == 1 and seen[1][kc.NAN_ROW] == 0
    from unina_yolo_dla_amd import mining
    whole = mining.kmeans_numpy(emb, 3, init, kc.NONFINITE_ITERS)
    assert (whole[1] == seen[-1]).all() and whole[3] == kc.NONFINITE_ITERS and np.isnan(whole[2]).all()
