"""The reference's active-learning "mining" roles (active_learning.py) on top of the engine's mining calls.

Same names and return types as the reference:

  compute_difficulty_scores ...... ActiveLearner.compute_difficulty_scores   active_learning.py:234-305
  query_uncertain_samples ........ ActiveLearner.query_uncertain_samples     active_learning.py:307-331
  extract_backbone_embeddings .... extract_backbone_embeddings               active_learning.py:31-99
  coreset_selection_kcenter ...... coreset_selection_kcenter                 active_learning.py:104-163

The GPU work is hand-written HIP behind the C ABI (csrc/mining.hip: ``unina_mine`` / ``unina_kcenter``). The pure-numpy
twins ``difficulty_from_heads`` and ``kcenter_numpy`` restate the reference's arithmetic; they are what the CPU tests pin
to the reference's recorded results and they run without a GPU. Not covered: the kmeans coreset variant
(active_learning.py:166-211, scikit-learn), the copy-paste augmenter, graph (B) models (no ``.backbone``).
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
