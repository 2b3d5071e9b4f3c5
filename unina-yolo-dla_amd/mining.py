"""The reference's active-learning "mining" roles (active_learning.py) on top of the engine's mining calls.

Same names and return types as the reference:

  compute_difficulty_scores ...... ActiveLearner.compute_difficulty_scores   active_learning.py:234-305
  query_uncertain_samples ........ ActiveLearner.query_uncertain_samples     active_learning.py:307-331
  extract_backbone_embeddings .... extract_backbone_embeddings               active_learning.py:31-99
  coreset_selection_kcenter ...... coreset_selection_kcenter                 active_learning.py:104-163
  coreset_selection_kmeans ....... coreset_selection_kmeans                  active_learning.py:166-211
  coreset_selection .............. ActiveLearner.coreset_selection           active_learning.py:327-360

The GPU work is hand-written HIP behind the C ABI (csrc/mining.hip: ``unina_mine`` / ``unina_kcenter``; csrc/kmeans.hip:
``unina_kmeans`` / ``unina_nearest_rows``). The pure-numpy twins ``difficulty_from_heads``, ``kcenter_numpy``,
``kmeans_numpy`` and ``nearest_rows_numpy`` restate the arithmetic; they are what the CPU tests pin to the reference's
recorded results and they run without a GPU. The kmeans variant clusters by full-batch Lloyd from k-means++ starts (the
reference's MiniBatchKMeans trajectory cannot be reproduced: DESIGN.md 9b); its selection loop is the reference's.
Not covered: the copy-paste augmenter, graph (B) models (no ``.backbone``).
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

MODES = ("entropy", "loc_var")
CLS_NAMES = ("p2_cls", "p3_cls", "p4_cls")


def difficulty_from_heads(heads) -> np.ndarray:
    """The 8 scores of include/unina_mi355.h (UNINA_MINE_SCORES) from raw cls logits, in fp32 numpy, in the reference's
    order of operations (active_learning.py:287-301). `heads`: {"p2_cls": [C,H,W], ...} or a sequence of the three cls planes."""
    planes = [heads[n] for n in CLS_NAMES] if isinstance(heads, dict) else list(heads)
    out = np.zeros(8, dtype=np.float32)
    one, eps = np.float32(1.0), np.float32(1e-10)
    for i, x in enumerate(planes):
        x = np.asarray(x, dtype=np.float32)
        p = one / (one + np.exp(-x))
        ent = -(p * np.log(p + eps) + (one - p) * np.log(one - p + eps))
        out[i] = ent.max()
        conf = p.max(axis=0)
        out[3 + i] = (one - np.abs(conf - np.float32(0.5)) * np.float32(2.0)).max()
    out[6] = out[0:3].max()
    out[7] = out[3:6].max()
    return out


def _score_index(mode: str) -> int:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")
    return 6 + MODES.index(mode)


def _device_frame(engine, frame):
    import torch
    if isinstance(frame, torch.Tensor):
        t = frame
    else:
        t = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32))
    if t.dim() == 3:
        t = t[None]
    return t.to(torch.device("cuda", engine.device), dtype=torch.float32).contiguous()


def compute_difficulty_scores(engine, frames: Iterable, paths: Sequence[str], mode: str = "entropy") -> Dict[str, float]:
    """{path: score} for `frames` ([3,H,W] / [1,3,H,W] fp32 arrays or tensors, already pre-processed), one engine call each."""
    k = _score_index(mode)
    scores: Dict[str, float] = {}
    for frame, path in zip(frames, paths):
        s, _ = engine.mine(_device_frame(engine, frame), embed=False)
        scores[path] = float(s[k])
    return scores


def query_uncertain_samples(engine, frames: Iterable, paths: Sequence[str], top_k: int = 100, mode: str = "entropy") -> List[str]:
    """The `top_k` paths with the highest score, descending (active_learning.py:324-331)."""
    scores = compute_difficulty_scores(engine, frames, paths, mode)
    ranked = sorted(scores.items(), key=lambda kv: kv[1], reverse=True)
    return [p for p, _ in ranked[:top_k]]


def extract_backbone_embeddings(engine, frames: Iterable, paths: Sequence[str]) -> Tuple[np.ndarray, List[str]]:
    """(embeddings [N,D] fp32, paths): the global average pool of the backbone's P4 map per frame."""
    embs, out_paths = [], []
    for frame, path in zip(frames, paths):
        _, e = engine.mine(_device_frame(engine, frame), embed=True)
        embs.append(e)
        out_paths.append(path)
    if not embs:
        raise ValueError("FATAL: Dataloader is empty. Cannot extract embeddings.")
    return np.vstack(embs), out_paths


def mine_frames(engine, frames: Iterable, paths: Sequence[str]):
    """One pass for both results: (scores [N,8] fp32, embeddings [N,D] fp32, paths)."""
    sc, embs, out_paths = [], [], []
    for frame, path in zip(frames, paths):
        s, e = engine.mine(_device_frame(engine, frame), embed=True)
        sc.append(s)
        embs.append(e)
        out_paths.append(path)
    if not sc:
        raise ValueError("FATAL: Dataloader is empty. Cannot extract embeddings.")
    return np.vstack(sc), np.vstack(embs), out_paths


def kcenter_numpy(embeddings: np.ndarray, k: int, first_index: int) -> np.ndarray:
    """The reference's loop (active_learning.py:143-161) with the start index given: `k` indices in selection order."""
    embeddings = np.asarray(embeddings)
    n = embeddings.shape[0]
    if not (0 <= first_index < n) or not (1 <= k <= n):
        raise ValueError("need 0 <= first_index < n and 1 <= k <= n")
    selected = [int(first_index)]
    min_distances = np.full(n, np.inf)
    for _ in range(k - 1):
        d = np.linalg.norm(embeddings - embeddings[selected[-1]], axis=1)
        min_distances = np.minimum(min_distances, d)
        min_distances[selected] = -1
        selected.append(int(np.argmax(min_distances)))
    return np.asarray(selected, dtype=np.int64)


def coreset_selection_kcenter(embeddings: np.ndarray, paths: Sequence[str], target_size: int, seed: Optional[int] = None,
                              device: Optional[bool] = None) -> List[str]:
    """K-center greedy selection of `target_size` paths. The first index is drawn as the reference draws it
    (``np.random.seed(seed); np.random.randint(n)``, which equals ``RandomState(seed).randint(n)``) without touching numpy's
    global state; with seed=None it is drawn from the global state, as in the reference. `device`: True = the GPU kernel
    (unina_kcenter), False = numpy, None = the GPU when one is visible."""
    n = embeddings.shape[0]
    if n == 0:
        raise ValueError("FATAL: Cannot perform Coreset Selection on empty dataset.")
    if target_size > n:
        print(f"WARNING: target_size ({target_size}) > n_samples ({n}). Returning all.")
        return list(paths)
    first = int(np.random.RandomState(seed).randint(n)) if seed is not None else int(np.random.randint(n))
    if target_size < 1:
        return [paths[first]]   # the reference's loop runs zero times and returns the start point
    if device is None:
        try:
            import torch
            device = torch.cuda.is_available()
        except ImportError:
            device = False
    if device:
        from .engine import kcenter
        sel = kcenter(embeddings, target_size, first)
    else:
        sel = kcenter_numpy(embeddings, target_size, first)
    return [paths[int(i)] for i in sel]


# ---- the kmeans coreset variant ---------------------------------------------------------------------------------------
def kmeans_pp_init(embeddings: np.ndarray, k: int, seed: Optional[int]) -> np.ndarray:
    """k-means++ start (Arthur & Vassilvitskii 2007): `k` distinct row indices, the first uniform, each next one drawn with
    probability proportional to the squared distance to the nearest row chosen so far. float64, O(n k dim), all draws from
    ``np.random.RandomState(seed)``: numpy's global state is not touched. When every remaining row coincides with a chosen
    one, the lowest unchosen index is taken."""
    x = np.asarray(embeddings, dtype=np.float64)
    n = x.shape[0]
    if not 1 <= k <= n:
        raise ValueError("need 1 <= k <= n")
    rng = np.random.RandomState(seed)
    rows = [int(rng.randint(n))]
    d2 = ((x - x[rows[0]]) ** 2).sum(axis=1)
    d2[rows[0]] = 0.0
    for _ in range(1, k):
        total = d2.sum()
        if total > 0:
            nxt = int(np.searchsorted(np.cumsum(d2), rng.random_sample() * total, side="right"))
            nxt = min(nxt, n - 1)
            if d2[nxt] == 0:                                    # (rounding at the end of the cumulative sum)
                nxt = int(np.argmax(d2))
        else:
            chosen = np.zeros(n, dtype=bool)
            chosen[rows] = True
            nxt = int(np.argmin(chosen))
        rows.append(nxt)
        d2 = np.minimum(d2, ((x - x[nxt]) ** 2).sum(axis=1))
        d2[nxt] = 0.0
    return np.asarray(rows, dtype=np.int64)


def kmeans_numpy(embeddings: np.ndarray, k: int, init_rows=None, max_iter: int = 100, centroids=None):
    """float64 twin of the device loop (csrc/kmeans.hip), same rules, same outputs. Per iteration: label = argmin_j
    |c_j|^2 - 2 <x, c_j> (lowest index on ties); c_j = mean of its members, a cluster without members keeps its centroid;
    inertia = sum (x - c_label)^2 with the new centroids. An iteration whose assignment changes no label is completed and
    is the last; labels are compared from the second iteration on. Non-finite values are not validated and follow the
    device's rule (include/unina_mi355.h): a NaN score never wins, and a row all of whose scores are NaN or +inf takes
    label 0. Returns (centroids, labels, inertia_history [iters], iters, converged)."""
    x = np.asarray(embeddings, dtype=np.float64)
    n = x.shape[0]
    if (init_rows is None) == (centroids is None):
        raise ValueError("give the start as init_rows or as centroids, not both")
    if init_rows is not None:
        init_rows = np.asarray(init_rows, dtype=np.int64).reshape(-1)
        if init_rows.min() < 0 or init_rows.max() >= n:
            raise ValueError(f"an init row lies outside [0, {n})")
        c = x[init_rows].copy()
    else:
        c = np.array(centroids, dtype=np.float64)
    if c.shape != (k, x.shape[1]) or not 1 <= k <= n or max_iter < 1:
        raise ValueError("need k start centroids, 1 <= k <= n and max_iter >= 1")
    labels = np.full(n, -1, dtype=np.int64)
    history: List[float] = []
    converged = False
    def nearest(block):
        scores = cn - 2.0 * (block @ c.T)
        return np.argmin(np.where(np.isnan(scores), np.inf, scores), axis=1)   # the device's strict <: a NaN never wins

    for _ in range(max_iter):
        with np.errstate(invalid="ignore", over="ignore"):                     # (non-finite data is not an error here)
            cn = (c * c).sum(axis=1)[None, :]
            new = np.concatenate([nearest(x[r:r + 8192]) for r in range(0, n, 8192)])   # (row blocks: memory)
            changed = int((new != labels).sum())
            labels = new
            order = np.argsort(labels, kind="stable")
            counts = np.bincount(labels, minlength=k)
            starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
            live = counts > 0
            sums = np.add.reduceat(x[order], starts[live], axis=0)
            c[live] = sums / counts[live][:, None]
            history.append(float(((x - c[labels]) ** 2).sum()))
        if changed == 0:
            converged = True
            break
    return c, labels, np.asarray(history, dtype=np.float64), len(history), converged


def nearest_rows_numpy(embeddings: np.ndarray, centroids: np.ndarray) -> np.ndarray:
    """The reference's selection loop (active_learning.py:203-209): one row index per centroid, in centroid order."""
    embeddings = np.asarray(embeddings)
    selected: List[int] = []
    for centroid in np.asarray(centroids):
        distances = np.linalg.norm(embeddings - centroid, axis=1)
        distances[selected] = np.inf
        selected.append(int(np.argmin(distances)))
    return np.asarray(selected, dtype=np.int64)


def coreset_selection_kmeans(embeddings: np.ndarray, paths: Sequence[str], target_size: int, seed: Optional[int] = None,
                             device: Optional[bool] = None, n_init: int = 3, max_iter: int = 100) -> List[str]:
    """The paths nearest to `target_size` k-means centroids. `n_init` Lloyd runs from k-means++ starts (seeds `seed`,
    `seed + 1`, ...; seed=None draws fresh entropy per start); the run with the lowest final inertia is kept, the first one
    on a tie; then the reference's selection loop. `device`: True = the GPU kernels (unina_kmeans / unina_nearest_rows),
    False = numpy, None = the GPU when one is visible."""
    n = embeddings.shape[0]
    if n == 0:
        raise ValueError("FATAL: Cannot perform Coreset Selection on empty dataset.")
    if target_size > n:
        return list(paths)
    if target_size < 1 or n_init < 1:
        raise ValueError("need target_size >= 1 and n_init >= 1")
    if device is None:
        try:
            import torch
            device = torch.cuda.is_available()
        except ImportError:
            device = False
    host = np.asarray(embeddings)
    if device:
        import torch
        from . import engine
        data = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).cuda()   # one upload for every start
        fit, pick = engine.kmeans, engine.nearest_rows
    else:
        data, fit, pick = host, kmeans_numpy, nearest_rows_numpy
    best, best_inertia = None, np.inf
    for i in range(n_init):
        init = kmeans_pp_init(host, target_size, None if seed is None else seed + i)
        cen, _, hist, _, _ = fit(data, target_size, init_rows=init, max_iter=max_iter)
        if best is None or hist[-1] < best_inertia:
            best, best_inertia = cen, hist[-1]
    return [paths[int(i)] for i in pick(data, best)]


def coreset_selection(embeddings: np.ndarray, paths: Sequence[str], target_size: int, method: str = "kcenter",
                      seed: Optional[int] = None, device: Optional[bool] = None) -> List[str]:
    """The dispatcher of ActiveLearner.coreset_selection (active_learning.py:352-359) on given embeddings. An unknown
    method is an error here (the reference runs k-center for anything that is not "kmeans")."""
    if method == "kmeans":
        return coreset_selection_kmeans(embeddings, paths, target_size, seed=seed, device=device)
    if method == "kcenter":
        return coreset_selection_kcenter(embeddings, paths, target_size, seed=seed, device=device)
    raise ValueError('method must be "kcenter" or "kmeans"')
