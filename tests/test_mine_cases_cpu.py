"""Keeps tests/mine_cases.py honest, on the CPU: every constructed mining case is recomputed with the numpy twins and must sit
where it says -- each planted score far from the background's and from the other levels', a witness cell whose removal moves
the score, special logits finite and one NaN spreading exactly as far as the twin says; the pool's frame loses the bound by a
factor of 100 when any one pixel is dropped; every selection case is decided identically in fp32, float64 and with the channels
permuted, and holds a step with an exact tie at the top and one without. A case that drifts fails here, before
tests/test_gpu_mine_edges.py runs it against the kernels."""
import numpy as np
import pytest

import mine_cases as mc
from test_mining_cpu import score_bound

FAR = 1000.0          # a planted score is this many bounds away from what a kernel that ignored the plant would report


def all_score_engines():
    return [(s, nc, False) for s in mc.SCORE_SIZES for nc in mc.CLASS_COUNTS] + [(mc.BIG_SIZE, mc.BIG_NC, True)]


def test_sizes_are_the_structural_edges():
    assert [mc.cells_of(s) for s in mc.SCORE_SIZES] == [(16, 4, 1), (272, 68, 17), (560, 140, 35), (1024, 256, 64)]
    c = mc.cells_of(mc.BIG_SIZE)
    assert c == (66560, 16640, 4160) and c[0] // mc.BLOCK == 260 and c[0] % mc.BLOCK == 0
    assert mc.positions(272) == [0, 63, 64, 255, 256, 271] and mc.positions(560) == [0, 63, 64, 255, 256, 512, 559]
    assert mc.positions(1) == [0] and mc.positions(256) == [0, 63, 64, 255] and mc.positions(1024) == [0, 63, 64, 255, 256, 768, 1023]
    assert {p // mc.BLOCK for p in mc.big_positions(c[0])} == {0, 255, 256, 259}
    for cells in (4, 16, 17, 35, 64, 68, 140, 256, 272, 560, 1024, 4160, 16640, 66560):
        for p in mc.positions(cells):
            q = mc.partner(p, cells)
            assert q != p and 0 <= q < cells
            assert cells <= mc.WAVE or q // mc.WAVE != p // mc.WAVE
            assert cells <= mc.BLOCK or q // mc.BLOCK != p // mc.BLOCK
    assert [mc.p4_pixels(s) for s in mc.POOL_SIZES_256] == [1, 3, 32, 33, 35, 64, 65]
    assert [mc.p4_pixels(s) for s in mc.POOL_SIZES_128] == [63, 64, 65]
    assert [mc.p4_pixels(s) for s in mc.POOL_ALL_PRECISIONS] == [1, 32, 33, 65]


@pytest.mark.parametrize("size,nc,big", all_score_engines(), ids=lambda v: str(v).replace(" ", ""))
def test_every_planted_score_is_far_from_background_and_from_the_other_levels(pkg, size, nc, big):
    """Per case: the six level scores sit >= 1000 bounds from the background's scores and pairwise >= 1000 bounds apart, and
    putting the witness cell back to background moves its score by >= 1000 bounds (roles "loc" and "ent_alone"; the entropy of
    role "ent" is carried by two cells, which is why the other two roles exist). Smallest margin seen over all cases: 5.9e5
    bounds against the background (the +2.0 class's loc_var of role "ent_alone"; 1.2e6 for the other roles), bound <= 4.8e-7."""
    bg32, _ = mc.twins(mc.background(size, nc))
    assert abs(bg32[0] - 0.0173) < 1e-4 and abs(bg32[3] - 0.0049) < 1e-4
    ids = mc.score_case_ids(size, nc, big)
    assert len(ids) >= (1 if nc == 1 else 6)
    worst, worst_bound, seen = np.inf, 0.0, [set(), set(), set()]
    for role, k, plane in ids:
        planes, where = mc.score_case(size, nc, role, k, plane, big=big)
        t32, t64 = mc.twins(planes)
        bound = score_bound(t32, t64)
        worst_bound = max(worst_bound, bound.max())
        assert np.isfinite(t32).all()
        far = np.abs(t32.astype(np.float64) - bg32) / bound
        worst = min(worst, far.min())
        assert (far >= FAR).all(), (role, k, plane, t32, bound)
        for a in range(3):
            for b in range(a + 1, 3):
                for o in (0, 3) if role != "ent_alone" or nc == 1 else (0,):      # (alone, every level's loc_var is the +2.0 class's)
                    assert abs(float(t32[o + a]) - float(t32[o + b])) >= FAR * max(bound[o + a], bound[o + b]), (role, k, plane, t32)
        assert t32[6] == t32[0] and t32[7] == t32[3]                                   # v_0 carries both totals
        for l in range(3):
            seen[l].add(where[l]["ent" if role != "loc" else "loc"])
            flat = planes[l].reshape(nc, -1)
            if nc >= 2 and flat.shape[1] > mc.WAVE and role != "ent_alone":
                assert where[l]["ent"] // mc.WAVE != where[l]["loc"] // mc.WAVE
            witness = [("loc", 3)] if role == "loc" else [("ent", 0), ("loc", 3)] if role == "ent_alone" else []
            for which, o in witness:
                cut = [p.copy() for p in planes]
                cut[l].reshape(nc, -1)[:, where[l][which]] = mc.BG
                c32, _ = mc.twins(cut)
                assert abs(float(c32[o + l]) - float(t32[o + l])) >= FAR * bound[o + l], (role, k, plane, l, which)
    cells = mc.cells_of(size)
    for l in range(3):
        want = set(mc.big_positions(cells[l]) if big and l == 0 else mc.positions(cells[l]))
        assert seen[l] == want, (l, seen[l], want)
    print(f"{size} nc={nc}: {len(ids)} cases, smallest margin {worst:.3g} bounds, largest bound {worst_bound:.3g}")
    assert worst_bound <= 4.8e-7


@pytest.mark.parametrize("value", mc.SPECIALS)
def test_saturating_logits_give_finite_scores(pkg, value):
    """A level wholly at +-88, +-104, +-1e30, +-inf: the twin gives +-0 or 1.4e-37, the bound (4e-10) comes from the float64
    evaluation; the other two levels keep their plants."""
    for level in range(3):
        planes = mc.special_case((16, 272), 4, level, value)
        t32, t64 = mc.twins(planes)
        assert np.isfinite(t32).all() and np.isfinite(t64).all()
        assert abs(t32[level]) <= 2e-37 and abs(t32[3 + level]) <= 2e-37
        b = score_bound(t32, t64)
        assert b[level] <= 4.1e-10 and b[3 + level] <= 4.1e-10
        ref, _ = mc.twins(mc.score_case((16, 272), 4, "ent", 0, 0)[0])
        others = [i for i in range(6) if i % 3 != level]
        assert t32[others].tobytes() == ref[others].tobytes()


@pytest.mark.parametrize("size,nc", [((16, 272), 4), ((80, 112), 7), ((16, 16), 1)])
def test_one_nan_spreads_to_its_level_and_both_totals_only(pkg, size, nc):
    ref, _ = mc.twins(mc.score_case(size, nc, "ent", 0, 0)[0])
    for level, cells in enumerate(mc.cells_of(size)):
        for pos in mc.nan_positions(cells):
            for plane in mc.planes_of(nc):
                t32, t64 = mc.twins(mc.nan_case(size, nc, level, pos, plane))
                want = np.zeros(8, bool)
                want[[level, 3 + level, 6, 7]] = True
                assert np.array_equal(np.isnan(t32), want) and np.array_equal(np.isnan(t64), want), (level, pos, plane, t32)
                assert t32[~want].tobytes() == ref[~want].tobytes()


# ---- pooled embedding ------------------------------------------------------------------------------------------------
def oracle_p4(pkg, oracle_mod, bc, size):
    g = pkg.graph.Graph(base_channels=bc, in_h=size[0], in_w=size[1])
    osd = oracle_mod.StateDict(pkg.synth.make_state_dict(7, g))
    try:
        ref = oracle_mod.forward(osd, pkg.rng.frame(mc.POOL_SEED, size[0], size[1]), base_channels=bc, keep_all=True)
    finally:
        osd.close()
    p4 = ref["backbone.stage3_c3k2.cv3"]
    assert p4.shape == (8 * bc, size[0] // 16, size[1] // 16)
    return p4.reshape(p4.shape[0], -1).astype(np.float64)


@pytest.mark.parametrize("bc,size", [(32, s) for s in mc.POOL_SIZES_256] + [(16, s) for s in mc.POOL_SIZES_128],
                         ids=lambda v: str(v).replace(" ", ""))
def test_pool_frame_loses_the_bound_when_any_pixel_is_dropped(pkg, oracle_mod, bc, size):
    """Frame seed 1236 on the CPU oracle's P4 map: dropping any ONE pixel from the float64 mean moves at least one channel by
    more than 100 bounds (gamma(hw + 2) * mean|x|). Smallest factor over the pixels of a size, seed 1236:
    256 channels: 3 px 3.4e6, 32 px 4.8e4, 33 px 5.0e4, 35 px 3.5e4, 64 px 9.7e3, 65 px 9.1e3
    128 channels: 63 px 8.3e3, 64 px 5.8e3, 65 px 6.1e3
    (one pixel: nothing to drop; there the fp16 and fp32 embedding is the buffer, bit for bit)."""
    x = oracle_p4(pkg, oracle_mod, bc, size)
    hw = mc.p4_pixels(size)
    assert x.shape == (8 * bc, hw) and np.abs(x).max() > 1e-2
    if hw == 1:
        return
    r = mc.drop_one_ratio(x)
    print(f"bc={bc} {size}: {hw} pixels, smallest drop-one factor {r.min():.3g}")
    assert r.shape == (hw,) and r.min() > 100.0


def test_pool_bound_is_the_derived_one():
    x = np.arange(12, dtype=np.float64).reshape(2, 6) - 4.0
    u = 2.0 ** -24
    assert np.allclose(mc.pool_bound(x), 8 * u / (1 - 8 * u) * np.abs(x).mean(axis=1), rtol=1e-15)
    r = mc.drop_one_ratio(x)
    j = 2
    moved = np.abs(np.delete(x, j, axis=1).mean(axis=1) - x.mean(axis=1))
    assert np.isclose(r[j], (moved / mc.pool_bound(x)).max(), rtol=1e-12)


# ---- selection loops -------------------------------------------------------------------------------------------------
def perm_of(dim):
    return np.random.RandomState(dim).permutation(dim)


@pytest.mark.parametrize("n", mc.KC_N)
def test_kcenter_cases_are_exact_and_hold_a_tie_and_a_clear_step(pkg, n):
    from unina_yolo_dla_amd import mining
    for dim in mc.KC_DIM:
        x = mc.integer_rows(n, dim)
        assert x.shape == (n, dim) and set(np.unique(x)) <= {0.0, 1.0, 2.0, 3.0}
        if n >= 4:
            assert np.array_equal(x[n // 2], x[1]) and np.array_equal(x[n - 1], x[0])
        for emb, k, first in mc.kcenter_cases(n, dim):
            want = mining.kcenter_numpy(emb, k, first)
            s64, tied = mc.kcenter_trace(emb, k, first)
            s32, t32 = mc.kcenter_trace(emb, k, first, dtype=np.float32)
            sp, tp = mc.kcenter_trace(emb, k, first, perm=perm_of(dim))
            assert want.tolist() == s64.tolist() == s32.tolist() == sp.tolist(), (n, dim, k, first)
            assert tied.tolist() == t32.tolist() == tp.tolist()
            if n >= 8:
                assert tied.any(), (n, dim, k, first)
                if mc.clear_step_possible(n, dim):
                    assert (~tied).any(), (n, dim, k, first)
    ks = {(k, first) for _, k, first in mc.kcenter_cases(n, 4)}
    assert ks == {(k, f) for k in ({min(n, 40), n} if n <= 65 else {40}) for f in {0, n - 1}}


@pytest.mark.parametrize("dim", mc.LADDER_DIM)
def test_kcenter_ladder_meets_its_ties_at_every_level_of_the_combine(pkg, dim):
    from unina_yolo_dla_amd import mining
    r = mc.LADDER_ROWS
    assert r[1] == r[0] + 1 and r[2] == r[0] + mc.WAVE and r[3] == r[0] + mc.ARG_BLOCK and r[4] == r[0] + 2 * mc.ARG_BLOCK
    assert mc.LADDER_N > r[4] and mc.LADDER_N > 2 * mc.ARG_BLOCK
    for i, (x, k, first) in enumerate(mc.kcenter_ladder_cases(dim)):
        assert sorted(np.flatnonzero(x.any(axis=1)).tolist()) == list(r[i:])
        want = mining.kcenter_numpy(x, k, first)
        sel, tied = mc.kcenter_trace(x, k, first, dtype=np.float32)
        assert want.tolist() == sel.tolist() and tied.all()
        rest = [j for j in range(mc.LADDER_N) if j not in (0, r[i])][:k - 2]
        assert sel.tolist() == [0, r[i]] + rest


@pytest.mark.parametrize("n", mc.NR_N)
def test_nearest_cases_are_exact_and_hold_a_tie_and_a_clear_step(pkg, n):
    from unina_yolo_dla_amd import mining
    for dim in mc.NR_DIM:
        x, c = mc.nearest_case(n, dim)
        assert c.shape == ((n if n <= 9 else 12), dim) and set(np.unique(c)) <= {0.0, 1.0, 2.0, 3.0}
        want = mining.nearest_rows_numpy(x, c)
        s64, tied = mc.nearest_trace(x, c)
        s32, t32 = mc.nearest_trace(x, c, dtype=np.float32)
        sp, tp = mc.nearest_trace(x, c, perm=perm_of(dim))
        assert want.tolist() == s64.tolist() == s32.tolist() == sp.tolist(), (n, dim)
        assert tied.tolist() == t32.tolist() == tp.tolist()
        assert len(set(want.tolist())) == len(want)
        if n >= 8:
            assert tied.any() and want[0] == 0 and want[2] == 1, (n, dim, want)
            if dim >= 63:       # (at 4 channels the grid has 256 points: rows 0 and 1 have other copies too)
                assert want[1] == n - 1 and n // 2 in want and want[c.shape[0] // 2] not in (0, n - 1), (n, dim, want)
            if mc.clear_step_possible(n, dim):
                assert (~tied).any(), (n, dim)


@pytest.mark.parametrize("dim", mc.NR_LADDER_DIM)
def test_nearest_ladder_walks_the_tied_rows_in_index_order(pkg, dim):
    from unina_yolo_dla_amd import mining
    x, c = mc.nearest_ladder_case(dim)
    want = mining.nearest_rows_numpy(x, c)
    sel, tied = mc.nearest_trace(x, c, dtype=np.float32)
    assert want.tolist() == sel.tolist() == list(mc.LADDER_ROWS) + [0]
    assert tied.tolist() == [True] * 4 + [False, True]
