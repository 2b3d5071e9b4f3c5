#!/usr/bin/env python3
"""Generates tests/golden/kmeans_blobs.npz by running the REFERENCE's coreset_selection_kmeans in the dev container.

    python tests/golden/make_golden_kmeans.py        (needs /root/reference and scikit-learn; never runs on the GPU box)

The reference clusters with scikit-learn's MiniBatchKMeans, whose trajectory and RNG stream this build does not reproduce
(it runs full-batch Lloyd from k-means++ starts). What can be pinned is the SELECTED SET on data where the answer does not
depend on the trajectory: K well-separated blobs, each ONE exact centre row plus m - 1 rows on a shell of radius 0.5 around
it (so the blob's mean is close to the centre row and no other row is), centres max(N(0, 4^2), 0), rows permuted, everything
from np.random.RandomState(data_seed). Any clustering that finds the blobs selects exactly the centre rows.

For every committed case the script ASSERTS (and stops with "choose another seed" otherwise) that
  * the reference's selection is the set of centre rows;
  * this repository's coreset_selection_kmeans(..., device=False) returns the same set;
  * at convergence every row's best and second-best centroid distance differ by more than 1e-3 relative (so fp32 kernels
    must reproduce the float64 labels).
Written per case: params (K, m, dim, data_seed, seed), the data (fp32), the centre-row indices, the reference's selection.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/unina_yolo_dla")
sys.modules.setdefault("cv2", types.ModuleType("cv2"))   # active_learning.py imports it for the augmenter only

import numpy as np  # noqa: E402

import active_learning as ref_al  # noqa: E402  (the reference)
from unina_yolo_dla_amd import mining  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 5
CASES = [(16, 24, 32, 3), (48, 20, 256, 3), (7, 9, 24, 4)]   # (K, m, dim, data_seed)
MARGIN = 1e-3


def blobs(K, m, dim, data_seed):
    """(data [K*m, dim] fp32, centre-row indices [K]): see the module docstring."""
    rng = np.random.RandomState(data_seed)
    centres = np.maximum(rng.normal(0.0, 4.0, size=(K, dim)), 0)
    rows, is_centre = [], []
    for c in centres:
        shell = rng.normal(size=(m - 1, dim))
        shell *= 0.5 / np.linalg.norm(shell, axis=1, keepdims=True)
        rows.append(np.vstack([c[None], c[None] + shell]))
        is_centre += [True] + [False] * (m - 1)
    perm = rng.permutation(K * m)
    data = np.vstack(rows)[perm].astype(np.float32)
    return data, np.flatnonzero(np.asarray(is_centre)[perm])


def case(K, m, dim, data_seed):
    data, centre_rows = blobs(K, m, dim, data_seed)
    paths = [str(i) for i in range(len(data))]
    tag = f"K{K}_m{m}_d{dim}_s{data_seed}"
    ref_sel = np.array([int(p) for p in ref_al.coreset_selection_kmeans(data, paths, K, seed=SEED)], dtype=np.int64)
    assert sorted(ref_sel.tolist()) == centre_rows.tolist(), f"{tag}: the reference does not select the centre rows, choose another seed"
    ours = [int(p) for p in mining.coreset_selection_kmeans(data, paths, K, seed=SEED, device=False)]
    assert sorted(ours) == centre_rows.tolist(), f"{tag}: this build's float64 path does not select the centre rows, choose another seed"
    # decision margins at convergence of the kept run (the one coreset_selection_kmeans keeps)
    best = None
    for i in range(3):
        run = mining.kmeans_numpy(data, K, mining.kmeans_pp_init(data, K, SEED + i), 100)
        if best is None or run[2][-1] < best[2][-1]:
            best = run
    cen, labels, hist, iters, converged = best
    assert converged, f"{tag}: not converged, choose another seed"
    d = np.sort(np.linalg.norm(data.astype(np.float64)[:, None, :] - cen[None], axis=2), axis=1)
    margin = float(((d[:, 1] - d[:, 0]) / d[:, 1]).min()) if K > 1 else np.inf
    assert margin > MARGIN, f"{tag}: decision margin {margin:.3g} <= {MARGIN}, choose another seed"
    print(f"{tag}: n {len(data)}, {iters} iterations, inertia {hist[-1]:.6g}, smallest relative margin {margin:.3g}")
    return tag, {"params": np.array([K, m, dim, data_seed, SEED]), "data": data, "centre_rows": centre_rows, "ref_selected": ref_sel}


def main():
    blob = {}
    tags = []
    for c in CASES:
        tag, items = case(*c)
        tags.append(tag)
        for name, v in items.items():
            blob[f"{tag}/{name}"] = v
    blob["cases"] = np.array(tags)
    out = os.path.join(GOLD, "kmeans_blobs.npz")
    np.savez_compressed(out, **blob)
    print("done", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
