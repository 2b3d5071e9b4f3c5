#!/usr/bin/env python3
"""Generates tests/golden/mining_seed1234.npz by running the REFERENCE's active-learning code in the dev container.

    python tests/golden/make_golden_mining.py        (needs /root/reference; never runs on the GPU box)

What is pinned, and by what (all data, no code):
  * frames ......... the reference model (model.py, seed-7 synthetic weights) under ActiveLearner.compute_difficulty_scores
                     (modes "entropy" and "loc_var") and extract_backbone_embeddings, fed a list of {"images", "paths"}
                     dicts as the data loader. Twelve 640x640 frames, seeds 1234..1245; frame 3 is multiplied by 0 and
                     frame 5 by 0.25: on a full-contrast synthetic frame some logit among 134 400 is ~0 and the entropy
                     score saturates at ln 2, so only the attenuated frames tell a correct kernel from a constant. Two 64x64.
  * per level ...... the same expressions (active_learning.py:287-301) per head, in fp32 and in float64.
  * head cases ..... synthetic logits away from zero (all <= -2, one planted extremum per level), num_classes 1, 4, 20,
                     at the head shapes of a 64x64 engine; scored by compute_difficulty_scores through a stub model.
  * k-center ....... relu(N(0.16, 0.24^2)) [2048, 256], target_size 32, seed 2 -> coreset_selection_kcenter's selection.
                     Asserts that at every step the best and second-best min-distance differ by >= 1e-4 relative.
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
import torch  # noqa: E402

import active_learning as ref_al  # noqa: E402  (the reference)
import model as ref_model  # noqa: E402
import unina_yolo_dla_amd as u  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED = 7
SEEDS = list(range(1234, 1246))
ATTENUATE = {3: 0.0, 5: 0.25}


def frames(h, w, seeds, att):
    out = []
    for i, s in enumerate(seeds):
        x = u.rng.frame(s, h, w)
        if i in att:
            x = (x * np.float32(att[i])).astype(np.float32)
        out.append(x)
    return out


def ref_net(sd, g):
    m = ref_model.UNINA_YOLO_DLA(g.num_classes, g.base_channels, g.lite_p2).eval()
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and all("num_batches_tracked" in k for k in res.missing_keys), res
    return m


def per_level(cls_planes, dtype):
    """active_learning.py:287-301 per head, in `dtype`: (entropy[3], loc_var[3])."""
    ent, loc = [], []
    for c in cls_planes:
        probs = torch.sigmoid(torch.as_tensor(c).to(dtype))
        e = -(probs * torch.log(probs + 1e-10) + (1 - probs) * torch.log(1 - probs + 1e-10))
        ent.append(e.max().item())
        conf = probs.max(dim=0)[0]
        loc.append((1.0 - (torch.abs(conf - 0.5) * 2.0)).max().item())
    return np.array(ent, dtype=np.float64), np.array(loc, dtype=np.float64)


def scores_row(ent, loc):
    return np.concatenate([ent, loc, [ent.max(), loc.max()]])


class StubModel(torch.nn.Module):
    """Returns given head tensors: lets compute_difficulty_scores score synthetic logits."""

    def __init__(self, planes):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.planes = planes

    def forward(self, images):
        return [(torch.as_tensor(c)[None], torch.zeros(1, 4, *c.shape[1:])) for c in self.planes]


def mine_set(m, xs, tag):
    paths = [f"{tag}_{i}" for i in range(len(xs))]
    loader = [{"images": torch.from_numpy(x), "paths": [p]} for x, p in zip(xs, paths)]
    learner = ref_al.ActiveLearner(m, gold_set_path=".")
    ent = learner.compute_difficulty_scores(loader, mode="entropy")
    loc = learner.compute_difficulty_scores(loader, mode="loc_var")
    emb, got_paths = ref_al.extract_backbone_embeddings(m, loader, device="cpu")
    assert got_paths == paths
    s32, s64 = [], []
    for x, p in zip(xs, paths):
        with torch.no_grad():
            out = m(torch.from_numpy(x))
        cls = [o[0][0] for o in out]
        r32, r64 = scores_row(*per_level(cls, torch.float32)), scores_row(*per_level(cls, torch.float64))
        assert np.float32(r32[6]) == np.float32(ent[p]) and np.float32(r32[7]) == np.float32(loc[p]), (p, r32, ent[p], loc[p])
        s32.append(r32.astype(np.float32))
        s64.append(r64)
    return np.stack(s32), np.stack(s64), emb.astype(np.float32)


def head_cases():
    """name -> (three cls planes at the head shapes of a 64x64 engine)."""
    rng = np.random.RandomState(4321)
    shapes = [(16, 16), (8, 8), (4, 4)]
    cases = {}
    for nc in (1, 4, 20):
        planes = [(-2.0 - 6.0 * rng.rand(nc, h, w)).astype(np.float32) for h, w in shapes]
        for lvl, (pl, val) in enumerate(zip(planes, (-1.25, -0.75, -1.0))):   # one planted extremum per level, known cell
            pl[nc - 1, pl.shape[1] // 2, (3 * lvl + 1) % pl.shape[2]] = np.float32(val)
        cases[f"nc{nc}"] = planes
    planes = [(-2.0 - 6.0 * rng.rand(4, h, w)).astype(np.float32) for h, w in shapes]
    planes[2][1, 3, 2] = np.float32(0.4)                                       # the extremum in P4 only, positive logit
    cases["nc4_p4only"] = planes
    planes = [(-9.0 + 18.0 * rng.rand(4, h, w)).astype(np.float32) for h, w in shapes]   # both signs, confident cells
    planes = [np.where(np.abs(p) < 1.0, np.float32(3.0), p).astype(np.float32) for p in planes]
    cases["nc4_mixed"] = planes
    return cases


def kcenter_case():
    rng = np.random.RandomState(2)
    emb = np.maximum(rng.normal(0.16, 0.24, size=(2048, 256)), 0).astype(np.float32)
    paths = [str(i) for i in range(len(emb))]
    sel = [int(p) for p in ref_al.coreset_selection_kcenter(emb, paths, 32, seed=2)]
    # replay: the decision margin at every step
    md = np.full(len(emb), np.inf)
    worst = np.inf
    chosen = [sel[0]]
    for t in range(1, 32):
        md = np.minimum(md, np.linalg.norm(emb - emb[chosen[-1]], axis=1))
        md[chosen] = -1
        top = np.sort(md)[-2:]
        worst = min(worst, (top[1] - top[0]) / top[1])
        assert int(np.argmax(md)) == sel[t]
        chosen.append(sel[t])
    assert worst >= 1e-4, f"k-center fixture: decision margin {worst:.3g} < 1e-4, choose another seed"
    print(f"k-center: first {sel[0]}, smallest relative margin {worst:.3g}")
    return np.array(sel, dtype=np.int64), worst


def main():
    torch.set_num_threads(8)
    blob = {}
    g640 = u.graph.Graph()
    sd = u.synth.make_state_dict(WEIGHT_SEED, g640)
    s32, s64, emb = mine_set(ref_net(sd, g640), frames(640, 640, SEEDS, ATTENUATE), "f640")
    blob["f640/seeds"], blob["f640/scores32"], blob["f640/scores64"], blob["f640/embed"] = np.array(SEEDS), s32, s64, emb
    blob["f640/attenuate_idx"] = np.array(sorted(ATTENUATE))
    blob["f640/attenuate_mul"] = np.array([ATTENUATE[i] for i in sorted(ATTENUATE)], dtype=np.float32)
    print("640 entropy:", s32[:, 6], "\n640 loc_var:", s32[:, 7])
    g64 = u.graph.Graph(in_h=64, in_w=64)
    s32, s64, emb = mine_set(ref_net(sd, g64), frames(64, 64, SEEDS[:2], {}), "f64")
    blob["f64/seeds"], blob["f64/scores32"], blob["f64/scores64"], blob["f64/embed"] = np.array(SEEDS[:2]), s32, s64, emb
    for name, planes in head_cases().items():
        learner = ref_al.ActiveLearner(StubModel(planes), gold_set_path=".")
        loader = [{"images": torch.zeros(1, 3, 64, 64), "paths": ["x"]}]
        r32, r64 = scores_row(*per_level(planes, torch.float32)), scores_row(*per_level(planes, torch.float64))
        assert np.float32(learner.compute_difficulty_scores(loader, mode="entropy")["x"]) == np.float32(r32[6])
        assert np.float32(learner.compute_difficulty_scores(loader, mode="loc_var")["x"]) == np.float32(r32[7])
        for lvl, pl in enumerate(planes):
            blob[f"heads/{name}/p{lvl + 2}_cls"] = pl
        blob[f"heads/{name}/scores32"], blob[f"heads/{name}/scores64"] = r32.astype(np.float32), r64
        print(name, r32)
    sel, margin = kcenter_case()
    blob["kcenter/selected"], blob["kcenter/margin"] = sel, np.array(margin)
    blob["kcenter/params"] = np.array([2, 2048, 256, 32, 2])   # data seed, n, dim, target_size, selection seed
    np.savez_compressed(os.path.join(GOLD, "mining_seed1234.npz"), **blob)
    print("done", os.path.getsize(os.path.join(GOLD, "mining_seed1234.npz")), "bytes")


if __name__ == "__main__":
    main()
