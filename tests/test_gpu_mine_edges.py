"""The data-mining path at its structural edges (-m gpu): the constructed cases of tests/mine_cases.py through csrc/mining.hip and
the nearest_* kernels of csrc/kmeans.hip. What the cases are and why they cannot pass with a plant ignored is proved on the CPU
by tests/test_mine_cases_cpu.py.

Which edge a case drives:
    scores      the partial last workgroup of a level, the level boundaries of the packed grid (blk0) with and without slack,
                every wave of block_max, class planes 0 and nc - 1, the second trip of mine_finish_kernel's strided loop
                (1024x1040: P2 is 260 workgroups); saturating logits; one NaN logit (numpy's max, the definition, keeps it)
    pool        P4 pixel counts on and beside a strip boundary of gap_embed_kernel (32 pixels at 256 channels, 64 at 128), every
                activation storage, fusion on and off, against the float64 mean of the engine's own buffer
    selection   exact ties at each level of the arg-max / arg-min combine (a thread's strided loop, lanes, waves, the serial
                pass), n beside the 1024-thread workgroup, dim beside one trip of the lane loops, scalar and float4 paths
No tolerance is new: scores are held to test_mining_cpu.score_bound, the pool to gamma(hw + 2) * mean|x| (derived in
mine_cases.pool_bound), selections index for index."""
import time

import numpy as np
import pytest

import mine_cases as mc
from test_mining_cpu import score_bound

pytestmark = pytest.mark.gpu

P4_BUFFER = "neck.cat_pan2"     # graph (A): backbone.stage3_c3k2.cv3 writes its last 256 channels


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engines(pkg, torch_cuda):
    """(size, nc) -> Engine, created on first use from the seed-7 synthetic weights (only the cls output tensors are used)."""
    from unina_yolo_dla_amd.engine import Engine
    made = {}

    def get(size, nc):
        if (size, nc) not in made:
            g = pkg.graph.Graph(num_classes=nc, in_h=size[0], in_w=size[1])
            made[size, nc] = Engine.from_state_dict(pkg.synth.make_state_dict(7, g), g)
        return made[size, nc]

    yield get
    for e in made.values():
        e.close()


def run_scores(torch, e, planes):
    for lvl, x in zip((2, 3, 4), planes):
        e.outputs[f"p{lvl}_cls"].copy_(torch.from_numpy(x)[None])
    return e.mine_heads()


def check_scores(got, planes, what):
    """NaN positions first, then every finite value under score_bound. Returns the worst |got - twin32| / bound."""
    t32, t64 = mc.twins(planes)
    assert np.array_equal(np.isnan(got), np.isnan(t32)), (what, got, t32)
    ok = ~np.isnan(t32)
    assert np.isfinite(got[ok]).all(), (what, got)
    dev = np.abs(got[ok].astype(np.float64) - t32[ok].astype(np.float64))
    bound = score_bound(t32[ok], t64[ok])
    assert (dev <= bound).all(), (what, got, t32, dev, bound)
    return float((dev / bound).max())


def sweep(torch, e, size, nc, big=False):
    worst = 0.0
    ids = mc.score_case_ids(size, nc, big)
    for role, k, plane in ids:
        planes, _ = mc.score_case(size, nc, role, k, plane, big=big)
        worst = max(worst, check_scores(run_scores(torch, e, planes), planes, (size, nc, role, k, plane)))
    print(f"{size} nc={nc}: {len(ids)} cases, worst |score - twin| / bound {worst:.3g}")


@pytest.mark.parametrize("nc", mc.CLASS_COUNTS)
@pytest.mark.parametrize("size", mc.SCORE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scores_at_the_structural_edges(pkg, engines, torch_cuda, size, nc):
    """Every role x position x plane of mine_cases.score_case_ids: all 8 values under max(8 ulp, 4 x |twin32 - twin64|)."""
    sweep(torch_cuda, engines(size, nc), size, nc)


def test_scores_past_one_trip_of_the_finish_loop(pkg, engines, torch_cuda):
    """1024x1040, nc = 4: P2 has 260 workgroups, so threads 0..3 of mine_finish_kernel take a second trip; plants in P2
    workgroups 0, 255, 256 and 259. Nothing is forwarded at this size."""
    t0 = time.perf_counter()
    e = engines(mc.BIG_SIZE, mc.BIG_NC)
    print(f"engine at {mc.BIG_SIZE}: built and loaded in {time.perf_counter() - t0:.2f} s")
    sweep(torch_cuda, e, mc.BIG_SIZE, mc.BIG_NC, big=True)


@pytest.mark.parametrize("value", mc.SPECIALS)
def test_saturating_logits_give_the_twins_finite_scores(pkg, engines, torch_cuda, value):
    size, nc = (16, 272), 4
    for level in range(3):
        planes = mc.special_case(size, nc, level, value)
        got = run_scores(torch_cuda, engines(size, nc), planes)
        assert np.isfinite(got).all(), (value, level, got)
        check_scores(got, planes, (value, level))


@pytest.mark.parametrize("size,nc", [((16, 272), 4), ((80, 112), 7), ((16, 16), 1)], ids=["16x272-nc4", "80x112-nc7", "16x16-nc1"])
def test_one_nan_logit_makes_its_level_and_both_totals_nan(pkg, engines, torch_cuda, size, nc):
    """One NaN in one class of one cell (first cell, last cell, first cell of the last workgroup; plane 0 and nc - 1): that
    level's two scores and scores[6], scores[7] are NaN, as numpy's max gives them; the other two levels keep their values."""
    e = engines(size, nc)
    for level, cells in enumerate(mc.cells_of(size)):
        for pos in mc.nan_positions(cells):
            for plane in mc.planes_of(nc):
                planes = mc.nan_case(size, nc, level, pos, plane)
                got = run_scores(torch_cuda, e, planes)
                want = np.zeros(8, bool)
                want[[level, 3 + level, 6, 7]] = True
                assert np.array_equal(np.isnan(got), want), (level, pos, plane, got)
                check_scores(got, planes, (level, pos, plane))


def test_one_engine_through_a_sequence_keeps_nothing(pkg, engines, torch_cuda):
    """High scores, then the background alone, then plants in P4 only: every call returns its own scores (nothing survives in
    score_partial), and two runs of one case give identical bytes."""
    size, nc = (80, 112), 4
    e = engines(size, nc)
    high = mc.score_case(size, nc, "ent", 0, 0)[0]
    p4_only = mc.score_case(size, nc, "ent", 0, nc - 1, levels=(2,))[0]
    seq = [high, mc.background(size, nc), p4_only, high, p4_only, mc.background(size, nc)]
    got = []
    for i, planes in enumerate(seq):
        got.append(run_scores(torch_cuda, e, planes))
        check_scores(got[-1], planes, f"sequence {i}")
    assert got[0].tobytes() == got[3].tobytes() and got[2].tobytes() == got[4].tobytes() and got[1].tobytes() == got[5].tobytes()
    assert got[1][6] < 0.02 and got[2][0] < 0.02 and got[2][2] > 0.6
    again = run_scores(torch_cuda, e, seq[-1])
    assert again.tobytes() == got[5].tobytes()


# ---- pooled embedding ------------------------------------------------------------------------------------------------
def pool_params():
    out = []
    for bc, sizes in ((32, mc.POOL_SIZES_256), (16, mc.POOL_SIZES_128)):
        for s in sizes:
            precisions = ("fp16", "strict", "fp32", "int8") if bc == 32 and s in mc.POOL_ALL_PRECISIONS else ("fp16",)
            out += [pytest.param(bc, s, p, id=f"{8 * bc}ch-{s[0]}x{s[1]}-{mc.p4_pixels(s)}px-{p}") for p in precisions]
    return out


def pool_engine(pkg, bc, size, precision):
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine, calibrate_amax
    g = pkg.graph.Graph(base_channels=bc, in_h=size[0], in_w=size[1])
    sd = pkg.synth.make_state_dict(7, g)
    if precision == "int8":
        amax = calibrate_amax(sd, g, [pkg.rng.frame(5000 + i, size[0], size[1]) for i in range(2)])
        return Engine.from_state_dict(sd, g, precision=export.INT8, amax=amax)
    return Engine.from_state_dict(sd, g, precision={"fp16": export.FP16, "strict": export.STRICT, "fp32": export.FP32}[precision])


@pytest.mark.parametrize("bc,size,precision", pool_params())
def test_pool_at_strip_edges(pkg, torch_cuda, bc, size, precision):
    """Real forward of frame seed 1236 (chosen on the CPU oracle, tests/test_mine_cases_cpu.py). Per channel,
    |embedding - float64 mean of the read-back P4 slice| <= gamma(hw + 2) * mean|x|; on the same buffer, dropping any one pixel
    from the mean moves a channel by more than 100 such bounds, so a pool that loses a pixel at a strip edge cannot pass. At one
    pixel the fp16 and fp32 embedding is the buffer, bit for bit."""
    e = pool_engine(pkg, bc, size, precision)
    try:
        d, hw = e.embedding_dim, mc.p4_pixels(size)
        assert d == 8 * bc
        x = torch_cuda.from_numpy(pkg.rng.frame(mc.POOL_SEED, size[0], size[1])).cuda()
        for fuse in (True, False):
            e.set_fusion(fuse)
            _, emb = e.mine(x)
            buf = e.read_buffer(P4_BUFFER)
            p4 = buf[buf.shape[0] - 256:][:d].reshape(d, -1)
            assert p4.shape == (d, hw) and np.isfinite(p4).all() and np.abs(p4).max() > 1e-2
            x64 = p4.astype(np.float64)
            bound = mc.pool_bound(x64)
            dev = np.abs(emb.astype(np.float64) - x64.mean(axis=1))
            live = bound > 0
            factor = mc.drop_one_ratio(x64).min() if hw > 1 else float("nan")
            print(f"{8 * bc}ch {size} {precision} fuse={fuse}: {hw} px, worst |emb - mean| / bound "
                  f"{(dev[live] / bound[live]).max():.3g}, smallest drop-one factor {factor:.3g}")
            assert (dev <= bound).all(), (fuse, int(np.argmax(dev - bound)), dev.max())
            if hw > 1:
                assert factor > 100.0
            elif precision in ("fp16", "fp32"):
                assert emb.tobytes() == np.ascontiguousarray(p4[:, 0], dtype=np.float32).tobytes()
    finally:
        e.close()


# ---- selection loops -------------------------------------------------------------------------------------------------
def device_rows(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()      # (a copy: the cached rows are read-only)


@pytest.mark.parametrize("n", mc.KC_N)
def test_kcenter_on_integer_rows_equals_numpy_index_for_index(pkg, torch_cuda, n):
    """Integers in {0..3}: every distance is exact in any summation order, equal distances are exact ties, so the lowest
    index must win at every level of the combine. dim 1 .. 260: the scalar and the float4 path, beside one trip of each."""
    from unina_yolo_dla_amd import engine, mining
    for dim in mc.KC_DIM:
        dev = device_rows(torch_cuda, mc.integer_rows(n, dim))
        for x, k, first in mc.kcenter_cases(n, dim):
            want = mining.kcenter_numpy(x, k, first)
            got = engine.kcenter(dev, k, first)
            assert got.tolist() == want.tolist(), (n, dim, k, first, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("dim", mc.LADDER_DIM)
def test_kcenter_tie_ladder(pkg, torch_cuda, dim):
    """Equal rows at 3, 4, 67, 1027 and 2051 among zero rows (then without 3, without 3 and 4, ...): the tie is met in one
    thread's strided loop (i, i + 1024, i + 2048), between lanes, between waves and in the serial pass."""
    from unina_yolo_dla_amd import engine, mining
    for x, k, first in mc.kcenter_ladder_cases(dim):
        want = mining.kcenter_numpy(x, k, first)
        got = engine.kcenter(x, k, first)
        assert got.tolist() == want.tolist(), (dim, want, got)


@pytest.mark.parametrize("n", mc.NR_N)
def test_nearest_rows_on_integer_rows_equals_numpy_index_for_index(pkg, torch_cuda, n):
    """Centroids equal to duplicated data rows, given more often than the row exists: a row taken by one centroid goes to
    nobody else, and each tie goes to the lowest index left."""
    from unina_yolo_dla_amd import engine, mining
    for dim in mc.NR_DIM:
        x, c = mc.nearest_case(n, dim)
        want = mining.nearest_rows_numpy(x, c)
        got = engine.nearest_rows(device_rows(torch_cuda, x), c)
        assert got.tolist() == want.tolist(), (n, dim, want, got)


@pytest.mark.parametrize("dim", mc.NR_LADDER_DIM)
def test_nearest_rows_tie_ladder(pkg, torch_cuda, dim):
    from unina_yolo_dla_amd import engine
    x, c = mc.nearest_ladder_case(dim)
    got = engine.nearest_rows(x, c)
    assert got.tolist() == list(mc.LADDER_ROWS) + [0], (dim, got)
