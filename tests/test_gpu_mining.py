"""GPU tests of the data-mining path (csrc/mining.hip behind unina_mine* / unina_kcenter), through the C ABI.

Reference results: tests/golden/mining_seed1234.npz (tests/golden/make_golden_mining.py runs the reference's
active_learning.py). Measured deviations and the bounds derived from them: profiles/r04/mining_parity.txt."""
import numpy as np
import pytest

from conftest import load_golden
from test_mining_cpu import assert_scores, head_case_names, kcenter_data

pytestmark = pytest.mark.gpu

P4_BUFFER = "neck.cat_pan2"     # graph (A): backbone.stage3_c3k2.cv3 writes its LAST 8 * base_channels channels ([p3_down | p4])

# fp32 / STRICT engines against the reference's recorded scores and embeddings of the twelve frames: 4 x the worst
# deviation measured on an MI355X (profiles/r04/mining_parity.txt: scores 7.15e-6 (fp32) / 6.56e-6 (STRICT), embeddings
# 4.77e-7 / 8.94e-7): room for another box and another summation order.
SCORE_TOL = 4 * 7.15e-6
EMBED_TOL = 4 * 8.94e-7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def gold():
    return load_golden("mining_seed1234.npz")


def make_engine(pkg, sd7, precision, size=(640, 640), num_classes=4, sd=None):
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine, calibrate_amax
    g = pkg.graph.Graph(num_classes=num_classes, in_h=size[0], in_w=size[1])
    sd = sd7 if sd is None else sd
    if precision == "int8":
        amax = calibrate_amax(sd, g, [pkg.rng.frame(5000 + i, size[0], size[1]) for i in range(2)])
        return Engine.from_state_dict(sd, g, precision=export.INT8, amax=amax)
    prec = {"fp16": export.FP16, "strict": export.STRICT, "fp32": export.FP32}[precision]
    return Engine.from_state_dict(sd, g, precision=prec)


def fixture_frames(pkg, gold):
    xs = []
    att = dict(zip(gold["f640/attenuate_idx"].tolist(), gold["f640/attenuate_mul"].tolist()))
    for i, s in enumerate(gold["f640/seeds"]):
        x = pkg.rng.frame(int(s), 640, 640)
        if i in att:
            x = (x * np.float32(att[i])).astype(np.float32)
        xs.append(x)
    return xs


@pytest.mark.parametrize("nc", [1, 4, 20])
def test_mine_heads_matches_reference_on_head_cases(pkg, torch_cuda, gold, nc):
    """Heads-only entry on bound synthetic logits: all 8 values, bound max(8 ulp, 4 x |ref32 - ref64|).
    Observed worst deviation on an MI355X: 6e-8 (one ulp)."""
    g = pkg.graph.Graph(num_classes=nc, in_h=64, in_w=64)
    from unina_yolo_dla_amd.engine import Engine
    e = Engine.from_state_dict(pkg.synth.make_state_dict(7, g), g)
    try:
        for name in [n for n in head_case_names(gold) if gold[f"heads/{n}/p2_cls"].shape[0] == nc]:
            for lvl in (2, 3, 4):
                e.outputs[f"p{lvl}_cls"].copy_(torch_cuda.from_numpy(gold[f"heads/{name}/p{lvl}_cls"])[None])
            got = e.mine_heads()
            assert_scores(got, gold[f"heads/{name}/scores32"], gold[f"heads/{name}/scores64"], f"gpu {name}")
    finally:
        e.close()


@pytest.mark.parametrize("precision", ["fp16", "strict", "fp32", "int8"])
@pytest.mark.parametrize("size", [(640, 640), (96, 160)])
def test_mine_equals_enqueue_plus_mine_heads_and_pools_the_p4_buffer(pkg, sd7, torch_cuda, precision, size):
    """mine() scores are BIT-equal to enqueue + mine_heads on the same handle; the embedding equals the float64 mean of the
    P4 slice as unina_debug_read_buffer decodes it, within the fp32 summation bound of H*W <= 1600 terms
    (rtol 1600 * 2^-24 ~ 1e-4, atol 1e-6). Every activation storage, fusion on and off, square and rectangular."""
    e = make_engine(pkg, sd7, precision, size)
    try:
        x = torch_cuda.from_numpy(pkg.rng.frame(1236, size[0], size[1])).cuda()
        d = e.embedding_dim
        assert d == 256
        for fuse in (True, False):
            e.set_fusion(fuse)
            scores, emb = e.mine(x)
            e.forward(x)
            again = e.mine_heads()
            assert scores.tobytes() == again.tobytes(), (precision, size, fuse, scores, again)
            assert np.isfinite(scores).all() and (scores >= 0).all() and scores[6] == scores[:3].max() and scores[7] == scores[3:6].max()
            buf = e.read_buffer(P4_BUFFER)
            want = buf[buf.shape[0] - d:].astype(np.float64).mean(axis=(1, 2))
            print(f"{precision} {size} fuse={fuse}: worst |embed - mean(buffer)| {np.abs(emb - want).max():.3g}")
            np.testing.assert_allclose(emb, want, rtol=1600 * 2.0 ** -24, atol=1e-6)
            assert emb.max() > 1e-2      # a live tensor, not an unwritten buffer
            s2, none = e.mine(x, embed=False)
            assert none is None and s2.tobytes() == scores.tobytes()
    finally:
        e.close()


@pytest.mark.parametrize("precision", ["fp32", "strict"])
def test_mine_matches_reference_on_twelve_frames(pkg, sd7, torch_cuda, gold, precision):
    """Scores and embeddings of the fp32 and STRICT engines against the reference's; the ranking of the frames by loc_var
    score is the reference's wherever two reference scores differ by more than twice the tolerance."""
    e = make_engine(pkg, sd7, precision)
    try:
        got_s, got_e = [], []
        for x in fixture_frames(pkg, gold):
            s, emb = e.mine(torch_cuda.from_numpy(x).cuda())
            got_s.append(s)
            got_e.append(emb)
        got_s, got_e = np.stack(got_s), np.stack(got_e)
        ref_s, ref_e = gold["f640/scores32"], gold["f640/embed"]
        ds, de = np.abs(got_s.astype(np.float64) - ref_s).max(), np.abs(got_e.astype(np.float64) - ref_e).max()
        print(f"{precision}: worst |score - reference| {ds:.3g} (bound {SCORE_TOL:.3g}), worst |embedding - reference| {de:.3g} (bound {EMBED_TOL:.3g})")
        assert ds <= SCORE_TOL, (precision, ds)
        assert de <= EMBED_TOL, (precision, de)
        # the attenuated frames are below ln 2 by far more than the tolerance: a constant would not pass
        assert abs(got_s[3, 6] - 0.68507) < 1e-4 and abs(got_s[5, 6] - 0.69022) < 1e-4
        loc_ref, loc_got = ref_s[:, 7], got_s[:, 7]
        for i in range(12):
            for j in range(12):
                if loc_ref[i] - loc_ref[j] > 2 * SCORE_TOL:
                    assert loc_got[i] > loc_got[j], (i, j, loc_ref[i], loc_ref[j], loc_got[i], loc_got[j])
    finally:
        e.close()


def test_mine_is_deterministic_and_leaves_the_frame_path_alone(pkg, sd7, torch_cuda):
    from unina_yolo_dla_amd.engine import Engine
    e = Engine.from_state_dict(sd7)
    try:
        x = torch_cuda.from_numpy(pkg.rng.frame(1234, 640, 640)).cuda()
        y = torch_cuda.from_numpy(pkg.rng.frame(1240, 640, 640)).cuda()
        before = e.infer(x, conf_thr=0.25)
        s1, e1 = e.mine(x)
        e.mine(y)
        s2, e2 = e.mine(x)
        assert s1.tobytes() == s2.tobytes() and e1.tobytes() == e2.tobytes()
        after = e.infer(x, conf_thr=0.25)
        assert len(before) > 0 and before.tobytes() == after.tobytes()
        # asynchronous form into rows of caller-owned matrices
        S = torch_cuda.zeros((3, 8), dtype=torch_cuda.float32, device="cuda")
        E = torch_cuda.zeros((3, e.embedding_dim), dtype=torch_cuda.float32, device="cuda")
        e.mine_async(x, S[1], E[1])
        torch_cuda.cuda.synchronize()
        assert S[1].cpu().numpy().tobytes() == s1.tobytes() and E[1].cpu().numpy().tobytes() == e1.tobytes()
        assert float(S[0].abs().sum()) == 0 and float(E[2].abs().sum()) == 0
    finally:
        e.close()


def test_graph_b_engine_scores_but_does_not_embed(pkg, torch_cuda):
    from unina_yolo_dla_amd.engine import Engine, EngineError
    g = pkg.graph.Graph(in_h=64, in_w=64, variant="B")
    e = Engine.from_state_dict(pkg.synth.make_state_dict(7, g), g)
    try:
        assert e.L.unina_embedding_dim(e.h) == -6
        x = torch_cuda.from_numpy(pkg.rng.frame(1234, 64, 64)).cuda()
        with pytest.raises(EngineError):
            e.mine(x)
        s, _ = e.mine(x, embed=False)
        assert np.isfinite(s).all() and s[6] > 0
    finally:
        e.close()


def test_narrow_model_reports_its_own_channels(pkg, torch_cuda):
    """base_channels=16 is embedded at width 32: the embedding has the model's 128 channels."""
    from unina_yolo_dla_amd.engine import Engine
    g = pkg.graph.Graph(base_channels=16, in_h=64, in_w=64)
    e = Engine.from_state_dict(pkg.synth.make_state_dict(7, g), g)
    try:
        assert e.embedding_dim == 128
        x = torch_cuda.from_numpy(pkg.rng.frame(1234, 64, 64)).cuda()
        _, emb = e.mine(x)
        buf = e.read_buffer(P4_BUFFER)
        p4 = buf[buf.shape[0] - 256:]
        assert np.abs(p4[128:]).max() == 0
        np.testing.assert_allclose(emb, p4[:128].astype(np.float64).mean(axis=(1, 2)), rtol=1600 * 2.0 ** -24, atol=1e-6)
    finally:
        e.close()


def test_kcenter_reproduces_reference_selection(pkg, torch_cuda, gold):
    """The fixture's decision margin is >= 1e-4 at every step; two fp32 sums of 256 non-negative terms in any order differ
    by at most 2 * 256 * 2^-24 ~ 3e-5 relative, so the GPU must pick the reference's 32 indices in order."""
    from unina_yolo_dla_amd import engine, mining
    emb, k, seed = kcenter_data(gold)
    want = gold["kcenter/selected"]
    got = engine.kcenter(emb, k, int(want[0]))
    assert got.tolist() == want.tolist()
    paths = [str(i) for i in range(len(emb))]
    assert mining.coreset_selection_kcenter(emb, paths, k, seed=seed, device=True) == [paths[i] for i in want]
    # exact ties: the lowest index wins; a dimension that is no multiple of 4 takes the scalar path
    tie = np.zeros((70, 6), dtype=np.float32)
    tie[1:, 0] = 1.0
    assert engine.kcenter(tie, 3, 0).tolist() == [0, 1, 2]
    rnd = np.random.RandomState(5).rand(300, 37).astype(np.float32)
    assert engine.kcenter(rnd, 20, 7).tolist() == mining.kcenter_numpy(rnd.astype(np.float64), 20, 7).tolist()
    assert engine.kcenter(rnd, 1, 9).tolist() == [9]


def test_kcenter_large_set_by_property(pkg, torch_cuda):
    """N = 65 536, D = 256, k = 256, independent of tie-breaking and of the code under test: replaying the GPU's selection in
    float64 numpy, every pick's min-distance to the earlier picks is >= (1 - 1e-4) x the maximum over all rows at that step."""
    from unina_yolo_dla_amd import engine
    n, d, k, first = 65536, 256, 256, 4242
    emb = np.maximum(np.random.RandomState(17).normal(0.16, 0.24, size=(n, d)), 0).astype(np.float32)
    sel = engine.kcenter(emb, k, first)
    assert sel[0] == first and len(set(sel.tolist())) == k and sel.min() >= 0 and sel.max() < n
    e64 = emb.astype(np.float64)
    sq = (e64 * e64).sum(axis=1)
    md = np.full(n, np.inf)
    worst = np.inf
    for t in range(1, k):
        last = e64[sel[t - 1]]
        dist = np.sqrt(np.maximum(sq + sq[sel[t - 1]] - 2.0 * (e64 @ last), 0.0))   # float64: the expanded form is exact enough here
        md = np.minimum(md, dist)
        md[sel[:t]] = -1
        best = md.max()
        worst = min(worst, md[sel[t]] / best)
        assert md[sel[t]] >= (1 - 1e-4) * best, (t, int(sel[t]), md[sel[t]], best)
    print(f"large k-center: smallest pick / best ratio {worst:.9f}")
