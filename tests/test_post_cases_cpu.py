"""Keeps tests/post_cases.py honest, on the CPU: every constructed post-process case is recomputed with numpy's float32 sigmoid
and the oracle, and must sit in the regime it declares (candidate count; S / cnt / want / distinct keys of the cut bin; levels of
the key-range split; share of suppressed candidates; the exact kept set of chains and pair edges). A case that drifts out of its
regime fails here, before tests/test_gpu_post_edges.py ever runs it against the kernel."""
import numpy as np
import pytest

import post_cases as pc

F = np.float32


def decode_np(heads, conf_thr):
    """conf (float32), class, pass mask per enumeration index: the decode's first-max-wins argmax from (0.0, -1)"""
    confs, classes = [], []
    for l in range(3):
        s = pc.sigmoid32(heads[2 * l]).reshape(heads[2 * l].shape[0], -1)
        best = np.full(s.shape[1], -1)
        mx = np.zeros(s.shape[1], F)
        for c in range(s.shape[0]):
            m = s[c] > mx                    # (NaN compares false)
            mx = np.where(m, s[c], mx)
            best = np.where(m, c, best)
        confs.append(mx)
        classes.append(best)
    conf, cls = np.concatenate(confs), np.concatenate(classes)
    return conf, cls, conf >= F(conf_thr)


def bits(x):
    return int(np.asarray(x, F).view(np.uint32))


def take_from_top(hist, want):
    """the bin that holds the want-th element counted from the top: (bin, wanted from it, its count)"""
    acc = 0
    for b in range(len(hist) - 1, -1, -1):
        if acc + hist[b] >= want:
            return b, want - acc, int(hist[b])
        acc += hist[b]
    raise AssertionError("fewer elements than wanted")


def cut_model(conf):
    """post_nms_kernel's overflow branch on the passing confidences: histogram bin T, then the key-range split loop"""
    keys = conf.view(np.uint32).astype(np.int64)
    bins = np.minimum((conf * F(pc.BINS)).astype(np.int64), pc.BINS - 1)
    T, want, cnt = take_from_top(np.bincount(bins, minlength=pc.BINS), pc.MAX_DET)
    out = {"T": T, "S": pc.MAX_DET - want, "cnt": cnt, "want": want, "distinct": len(np.unique(keys[bins == T]))}
    klo = bits(F(T) / F(pc.BINS))
    khi = 0x3F800001 if T == pc.BINS - 1 else bits(F(T + 1) / F(pc.BINS))
    levels = 0
    out.update(klo0=klo, khi0=khi, wdt0=None)          # bin T's key range, and the width of its first split if there is one
    while cnt > pc.MEM_CAP and khi - klo > 1:
        wdt = (khi - klo + pc.BINS - 1) // pc.BINS
        if levels == 0:
            out["wdt0"] = wdt
        m = keys[(keys >= klo) & (keys < khi)]
        b, want, cnt = take_from_top(np.bincount((m - klo) // wdt, minlength=pc.BINS), want)
        nlo = klo + b * wdt
        khi, klo = min(nlo + wdt, khi), nlo
        levels += 1
    out.update(levels=levels, eidx_split=cnt > pc.MEM_CAP, frac=None)
    return out, bins, keys


def box_of(heads, grids, e):
    """the decode's box of enumeration index e (q = 0), in its float32 arithmetic"""
    l = int(pc.level_of(grids, e))
    off = sum(gh * gw for gh, gw in grids[:l])
    y, x = divmod(e - off, grids[l][1])
    fs = F(pc.STRIDES[l])
    xc, yc = (F(x) + F(0.5)) * fs, (F(y) + F(0.5)) * fs
    r = heads[2 * l + 1][:, y, x]
    return F(xc - r[0] * fs), F(yc - r[1] * fs), F(xc + r[2] * fs), F(yc + r[3] * fs)


def test_ladder_gap_and_floor():
    s = pc.sigmoid32(pc.LADDER).astype(np.float64)
    assert np.all(pc.LADDER.astype(np.float64) == 3.0 - np.arange(1400) / 256.0)      # exact in float32
    assert np.min(-np.diff(s)) >= 1e-4 and s.min() > 0.07
    # exp in float64 agrees: the gap is a property of the logits, not of one expf
    s64 = 1.0 / (1.0 + np.exp(-pc.LADDER.astype(np.float64)))
    assert np.abs(s - s64).max() < 2e-7


@pytest.mark.parametrize("name", list(pc.CASES))
def test_case_sits_in_its_declared_regime(name, oracle_mod):
    grids, nc = pc.ENGINES[pc.engine_of(name)]
    heads, conf_thr, iou_thr, q, ex = pc.build(name, grids, nc)
    assert [h.shape for h in heads] == [(c, gh, gw) for gh, gw in grids for c in (nc, 4)]
    assert all(h.dtype == np.float32 and h.flags.c_contiguous for h in heads)
    conf, cls, ok = decode_np(heads, conf_thr)
    assert int(ok.sum()) == ex["total"], (int(ok.sum()), ex["total"])
    want, ncand = oracle_mod.postprocess(heads, conf_thr, iou_thr, q)
    assert ncand == ex["total"]
    n = min(ncand, pc.MAX_DET)
    assert np.all(np.diff(want["confidence"]) <= 0)
    if "kept" in ex:
        assert len(want) == ex["kept"], (len(want), ex["kept"])
    if "share" in ex:
        share = 1.0 - len(want) / n
        assert ex["share"][0] <= share <= ex["share"][1], share
    if "kept_e" in ex:
        assert q == 0.0 and len(want) == len(ex["kept_e"])
        boxes = np.array([box_of(heads, grids, e) for e in ex["kept_e"]], F).reshape(-1, 4)
        got = np.stack([want[f] for f in ("x1", "y1", "x2", "y2")], axis=1) if len(want) else np.zeros((0, 4), F)
        assert np.array_equal(got, boxes)
    if ex.get("alternating"):          # confidence falls along every row: exactly the even columns survive
        assert sorted(ex["kept_e"]) == [y * grids[0][1] + x for y in range(pc.CHAIN_ROWS) for x in range(0, pc.CHAIN_COLS, 2)]
    if "all_class" in ex:
        assert np.all(want["class_id"] == ex["all_class"]) and np.all(want["confidence"] == F(ex["all_conf"]))
    if "first_conf_one" in ex:
        k = ex["first_conf_one"]
        assert np.all(want["confidence"][:k] == F(1.0)) and np.all(want["confidence"][k:] < F(1.0))
    if "cut" in ex and grids == pc.GRIDS_96x160:     # confidence 0.0 (and 9e-14): exact values at the bottom of bin 0
        model, _, _ = cut_model(conf[ok])
        assert {f: model[f] for f in ex["cut"]} == ex["cut"], model
    if "T" in ex:
        assert ncand > pc.MAX_DET
        model, bins, keys = cut_model(conf[ok])
        for f in ("T", "S", "cnt", "want", "distinct", "levels", "eidx_split"):
            assert model[f] == ex[f], (f, model[f], ex[f])
        # every confidence of the cut bin at least a quarter bin from both of its edges (1.0 itself is the last bin's upper end)
        c = conf[ok][bins == ex["T"]].astype(np.float64) * pc.BINS - ex["T"]
        c = c[conf[ok][bins == ex["T"]] < F(1.0)]
        assert c.min() >= 0.25 - 1e-3 and c.max() <= 0.75 + 1e-3, (c.min(), c.max())
        # ... and no other candidate within a quarter bin of the cut bin
        others = conf[ok][bins != ex["T"]].astype(np.float64) * pc.BINS
        assert np.all((others < ex["T"] - 0.25) | (others > ex["T"] + 1.25))
        if ex["tied"]:                 # ties are broken by enumeration index ACROSS the levels: each tied population spans P2, P3, P4
            e = np.flatnonzero(ok)[bins == ex["T"]]
            for k in np.unique(keys[bins == ex["T"]]):
                assert set(pc.level_of(grids, e[keys[bins == ex["T"]] == k]).tolist()) == {0, 1, 2}, k


def test_cut_table_covers_the_listed_regimes():
    names = set(pc.CUT_NAMES)
    for cnt, wants in ((1023, (1, 2, 1022, 1023)), (1024, (1, 2, 1023, 1024)), (1025, (1, 2, 1024)), (1026, (1, 2)), (5000, (1, 2))):
        for w in wants:
            for k in ("1key", "2keys", "manykeys"):
                assert f"cut-bin2048-cnt={cnt}-want={w}-{k}" in names
    levels = {n: pc.CASES[n][1]["levels"] for n in names}
    assert {0, 1, 2, 3} <= set(levels.values())
    assert any(pc.CASES[n][1]["eidx_split"] for n in names) and not all(pc.CASES[n][1]["eidx_split"] for n in names)


def test_count_sweep_sits_on_the_tile_and_block_edges():
    """nw = ceil(n / 64) changes at 64 / 128 / 512 / 1024, the last arriver's second candidate (tid + 512) starts at 513, the
    overflow branch at 1025"""
    assert set(pc.COUNTS) >= {0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1260}
    for n in pc.COUNTS:
        heads, conf_thr, iou_thr, q, ex = pc.build(f"n={n}-disjoint")
        _, _, ok = decode_np(heads, conf_thr)
        e = np.flatnonzero(ok)
        assert len(e) == n
        if n >= 63:                     # scattered: candidates on all three levels and in many 256-cell launch-1 workgroups
            assert set(pc.level_of(pc.GRIDS_96x160, e).tolist()) == {0, 1, 2} and len(set((e // 256).tolist())) >= 4


def test_iou_half_pair_flips_between_the_two_thresholds(oracle_mod):
    heads, conf_thr, iou_eq, q, _ = pc.build("pair-iou_eq")
    assert iou_eq == 0.5 and F(pc.IOU_HALF_BELOW) < F(0.5) and float(F(pc.IOU_HALF_BELOW)) == pc.IOU_HALF_BELOW
    both, _ = oracle_mod.postprocess(heads, conf_thr, 0.5, q)
    one, _ = oracle_mod.postprocess(heads, conf_thr, pc.IOU_HALF_BELOW, q)
    assert len(both) == 2 and len(one) == 1
    a, b = both[0], both[1]
    assert (a["x1"], a["y1"], a["x2"], a["y2"]) == (34.0, 34.0, 50.0, 50.0) and (b["x1"], b["y1"], b["x2"], b["y2"]) == (34.0, 34.0, 50.0, 42.0)
    assert F(128.0) / (F(256.0) + F(1e-6)) == F(0.5)      # the 1e-6 is absorbed


def test_sequence_cases_build_on_the_640_grids(oracle_mod):
    for name in pc.SEQUENCE:
        heads, conf_thr, iou_thr, q, ex = pc.build(name, pc.GRIDS_640, 4)
        _, ncand = oracle_mod.postprocess(heads, conf_thr, iou_thr, q)
        assert ncand == ex["total"], name
    counts = [pc.build(n, pc.GRIDS_640, 4)[4]["total"] for n in pc.SEQUENCE]
    assert max(counts) == 33600 and min(counts) == 0
