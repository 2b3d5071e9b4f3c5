"""Constructed post-process frames (plain numpy, no GPU): every case puts decode + top-1024 cut + NMS into ONE named regime of
csrc/postprocess.hip and is built so that the comparison with the oracle is exact -- order included.

    build(name, grids, num_classes) -> (heads, conf_thr, iou_thr, q, expect)

heads: the six planar float32 arrays in graph.OUTPUT_NAMES order. grids: ((gh, gw),) * 3 for P2, P3, P4 (strides 4, 8, 16).
expect: what the case DECLARES about itself (tests/test_post_cases_cpu.py recomputes every entry with numpy and the oracle):
    total       cells that pass conf_thr
    share       (lo, hi): fraction of min(total, 1024) that the NMS suppresses           (suppressing cases)
    kept_e      enumeration indices of the kept records, in output order                 (chains, pair edges)
    T, S, cnt, want, distinct, levels, eidx_split                                         (cut cases, see cut_case)
    cut         the same seven for the conf_thr = 0 frames, whose cut bin holds exact zeros (no bin-placement claim)
    tied        the case holds exact confidence ties scattered over the frame (run-to-run test)

Two ingredients keep the order decidable although GPU expf and glibc expf may differ by an ulp:
  * the confidence LADDER: logits 3 - k/256 (exact in float32), k < 1400. Adjacent sigmoids differ by >= 1.7e-4, the smallest
    is 0.078: an ulp (6e-8) cannot reorder two candidates or move one across conf_thr = 0.05. Exact ties = identical logits.
  * BINNED confidences: a confidence aimed at bin T of the kernel's 4096-bin histogram is the float32 logit of a point at least
    a quarter bin (6e-5) from both edges of the bin.
Background cells: every class logit -30 (sigmoid 9e-14), reg 0.2 -- a box of 0.4 cells that suppresses nothing.
"""
import numpy as np

F = np.float32
STRIDES = (4, 8, 16)
GRIDS_96x160 = ((24, 40), (12, 20), (6, 10))        # 1260 cells, non-square
GRIDS_640 = ((160, 160), (80, 80), (40, 40))        # 33 600 cells
MAX_DET = 1024                                       # kMaxDet
MEM_CAP = 1024                                       # kMemCap: members of the cut bin that are ranked exactly
BINS = 4096                                          # kBins
BG_LOGIT, BG_REG = -30.0, 0.2
LADDER = (F(3) - np.arange(1400, dtype=F) / F(256)).astype(F)
CHAIN_REG = (2.0, 0.4, 2.0, 0.4)                     # P2: 16 px wide, 3.2 px tall; neighbours 4 px apart: IoU 12/20, next 8/24
CHAIN_ROWS, CHAIN_COLS = 24, 40


def sigmoid32(x):
    """The decode's sigmoid in float32 arithmetic (numpy's expf; within an ulp of glibc's and the GPU's)."""
    x = np.asarray(x, F)
    with np.errstate(over="ignore", invalid="ignore"):
        return (F(1) / (F(1) + np.exp(-x))).astype(F)


def logit_of(conf):
    """float32 logit whose sigmoid is `conf` (float64 inverse, rounded once)."""
    c = np.asarray(conf, np.float64)
    return np.log(c / (1.0 - c)).astype(F)


def binned_logits(T, d):
    """d logits whose confidences sit in bin T between 0.25 and 0.75 of the bin, evenly spaced (d = 1: the middle)."""
    pos = np.full(1, 0.5) if d == 1 else 0.25 + 0.5 * np.arange(d) / (d - 1)
    return logit_of((T + pos) / BINS)


class Frame:
    def __init__(self, grids, nc, bg=BG_LOGIT):
        self.grids, self.nc = tuple(tuple(g) for g in grids), nc
        self.cls = [np.full((nc, gh, gw), bg, F) for gh, gw in self.grids]
        self.reg = [np.full((4, gh, gw), BG_REG, F) for gh, gw in self.grids]
        self.off = np.concatenate([[0], np.cumsum([gh * gw for gh, gw in self.grids])])
        self.ncells = int(self.off[3])

    def e_of(self, level, y, x):
        """enumeration index (P2 -> P3 -> P4, row-major) of a cell"""
        return int(self.off[level]) + y * self.grids[level][1] + x

    def put(self, e, cls, logit, reg=None):
        """cells e (enumeration indices): class `cls` gets `logit`, the other classes keep the background; optional (l, t, r, b)"""
        e = np.atleast_1d(np.asarray(e, np.int64))
        cls = np.broadcast_to(np.asarray(cls, np.int64), e.shape)
        logit = np.broadcast_to(np.asarray(logit, F), e.shape)
        if reg is not None:
            reg = np.broadcast_to(np.asarray(reg, F), e.shape + (4,))
        for l in range(3):
            m = (e >= self.off[l]) & (e < self.off[l + 1])
            i = e[m] - self.off[l]
            self.cls[l].reshape(self.nc, -1)[cls[m], i] = logit[m]
            if reg is not None:
                self.reg[l].reshape(4, -1)[:, i] = reg[m].T

    def put_all_classes(self, e, logit):
        e = np.atleast_1d(np.asarray(e, np.int64))
        for l in range(3):
            m = (e >= self.off[l]) & (e < self.off[l + 1])
            self.cls[l].reshape(self.nc, -1)[:, e[m] - self.off[l]] = F(logit)

    def heads(self):
        return [a for l in range(3) for a in (self.cls[l], self.reg[l])]


def scatter(ncells, seed):
    """fixed-seed permutation of every cell of the three levels: consecutive picks land in many launch-1 workgroups"""
    return np.random.default_rng(seed).permutation(ncells)


def level_of(grids, e):
    off = np.concatenate([[0], np.cumsum([gh * gw for gh, gw in grids])])
    return np.searchsorted(off, np.asarray(e), side="right") - 1


# ---------------------------------------------------------------------------------------------------- count sweep
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1260)   # nw = ceil(n / 64), kTN = 512, kMaxDet


def overlap_scale(n, ncells):
    """Box half-size multiplier of the suppressing variant: reg is uniform in 1..3 cells times this. A frame whose every cell
    is a candidate (n = 1260) has one candidate per cell and the plain 1..3 cells do; a sparser scatter has its candidates
    sqrt(ncells / n) cells apart on average, and the boxes grow by that factor so that a box still covers the same number of
    same-class neighbours (the oracle then suppresses 32-39 % at every n of the sweep)."""
    return max(1.0, float(np.sqrt(ncells / max(n, 1))))


def count_case(grids, nc, n, overlap):
    fr = Frame(grids, nc)
    assert n <= fr.ncells and n <= len(LADDER)
    rng = np.random.default_rng(1000 + n)
    cells = scatter(fr.ncells, 17)[:n]
    ranks = rng.permutation(n)                        # confidence order unrelated to the enumeration order
    cls = rng.integers(0, min(nc, 4), n)
    reg = None
    if overlap:
        reg = (rng.uniform(1.0, 3.0, (n, 4)) * overlap_scale(n, fr.ncells)).astype(F)
    fr.put(cells, cls, LADDER[ranks], reg)
    expect = {"total": n}
    if overlap and n >= 63:
        expect["share"] = (0.2, 0.8)
    if not overlap:
        expect["kept"] = min(n, MAX_DET)
    return fr.heads(), 0.05, 0.45, (0.1 if overlap else 0.0), expect


# ---------------------------------------------------------------------------------------------------- chains
def chain_greedy(conf_rank, cls):
    """Greedy NMS of CHAIN_ROWS x CHAIN_COLS chain cells by the chain's own rule -- a box suppresses its LEFT and RIGHT
    neighbour of the same class and a lower confidence, nothing else; a suppressed box suppresses nothing. conf_rank[y, x] =
    ladder rank (0 = highest). Returns the kept (y, x) in output order (rank ascending)."""
    alive = np.ones(conf_rank.shape, bool)
    order = np.argsort(conf_rank, axis=None, kind="stable")
    kept = []
    for f in order:
        y, x = divmod(int(f), conf_rank.shape[1])
        if not alive[y, x]:
            continue
        kept.append((y, x))
        for xx in (x - 1, x + 1):
            if 0 <= xx < conf_rank.shape[1] and cls[y, xx] == cls[y, x] and conf_rank[y, xx] > conf_rank[y, x]:
                alive[y, xx] = False
    return kept


def chain_ranks(order):
    ys, xs = np.mgrid[0:CHAIN_ROWS, 0:CHAIN_COLS]
    if order == "fall":            # confidence falls along each row: the oracle keeps every other box
        return ys * CHAIN_COLS + xs
    if order == "rr":              # ranks dealt round-robin over the rows: consecutive ranks sit in different rows
        return xs * CHAIN_ROWS + ys
    assert order == "perm"
    return np.random.default_rng(23).permutation(CHAIN_ROWS * CHAIN_COLS).reshape(CHAIN_ROWS, CHAIN_COLS)


def chain_classes(layout, nc):
    ys, xs = np.mgrid[0:CHAIN_ROWS, 0:CHAIN_COLS]
    if layout == "one":            # 960 rows in ONE wave's list (class & 3 == 0)
        return np.zeros_like(xs)
    if layout == "byrow":          # four waves, 240 rows each
        return ys % 4
    assert layout == "c1c5" and nc >= 6
    # classes 1 and 5 share a scan wave (1 & 3 == 5 & 3). Interleaved in PAIRS (1 1 5 5 1 1 ...): inside a pair the neighbour
    # is suppressed, across a pair boundary the neighbour has the other class and must survive. (Interleaved singly, no pair
    # of equal class would overlap at all and a wave that mixed the two classes up could not be told from a correct one.)
    return np.where((xs // 2) % 2 == 0, 1, 5)


def chain_case(grids, nc, order, layout):
    fr = Frame(grids, nc)
    assert grids[0][0] >= CHAIN_ROWS and grids[0][1] >= CHAIN_COLS
    ranks, cls = chain_ranks(order), chain_classes(layout, nc)
    ys, xs = np.mgrid[0:CHAIN_ROWS, 0:CHAIN_COLS]
    e = (ys * grids[0][1] + xs).ravel()
    fr.put(e, cls.ravel(), LADDER[ranks.ravel()], CHAIN_REG)
    kept = chain_greedy(ranks, cls)
    expect = {"total": CHAIN_ROWS * CHAIN_COLS, "kept_e": [y * grids[0][1] + x for y, x in kept]}
    if order in ("fall", "rr") and layout != "c1c5":
        expect["alternating"] = True
    return fr.heads(), 0.05, 0.45, 0.0, expect


# ---------------------------------------------------------------------------------------------------- pair edges
IOU_HALF_BELOW = float(np.nextafter(F(0.5), F(0)))


def pair_case(grids, nc, kind):
    """Box A = [34,50]^2 from P2 cell (x 10, y 10), reg (2,2,2,2). Box B = x [34,50], y [34,42] from P2 cell (x 11, y 10), reg
    (3,2,1,0). Intersection 128, union 256: IoU = 128 / (256 + 1e-6f) = 0.5 exactly in float32."""
    fr = Frame(grids, nc)
    a, b = fr.e_of(0, 10, 10), fr.e_of(0, 10, 11)
    conf_thr, iou_thr = 0.05, 0.45
    la, lb, ca, cb = LADDER[0], LADDER[1], 0, 0
    if kind == "iou_eq":                 # strict >: IoU == threshold suppresses nothing
        iou_thr, kept = 0.5, [a, b]
    elif kind == "iou_below":
        iou_thr, kept = IOU_HALF_BELOW, [a]
    elif kind == "equal_conf":           # strict confidence: neither goes; output in enumeration order
        lb, iou_thr, kept = la, 0.1, [a, b]
    elif kind == "b_higher":             # the later cell has the higher confidence: it comes first and suppresses A
        la, lb, kept = LADDER[1], LADDER[0], [b]
    else:
        assert kind == "other_class"
        cb, kept = 1, [a, b]
    fr.put(a, ca, la, (2, 2, 2, 2))
    fr.put(b, cb, lb, (3, 2, 1, 0))
    return fr.heads(), conf_thr, iou_thr, 0.0, {"total": 2, "kept_e": kept}


def special_case(grids, nc, kind):
    fr = Frame(grids, nc)
    order = scatter(fr.ncells, 29)
    rng = np.random.default_rng(31)
    if kind == "all_m200":               # sigmoid(-200) == 0: best stays -1, conf 0 >= 0 passes. Cut by enumeration index alone.
        fr.put_all_classes(np.arange(fr.ncells), -200.0)
        tot = fr.ncells
        return fr.heads(), 0.0, 0.45, 0.0, {"total": tot, "kept": min(tot, MAX_DET), "all_class": -1, "all_conf": 0.0,
                                            "kept_e": list(range(min(tot, MAX_DET))), "tied": True,
                                            "cut": dict(T=0, S=0, cnt=tot, want=MAX_DET, distinct=1, levels=3, eidx_split=True)}
    if kind == "part_m200":              # 400 cells of class -1 and confidence 0 below a ladder that fills the rest of the frame
        n_m = 400
        lad = order[n_m:]
        assert len(lad) <= len(LADDER)
        fr.put_all_classes(order[:n_m], -200.0)
        fr.put(lad, rng.integers(0, min(nc, 4), len(lad)), LADDER[rng.permutation(len(lad))])
        return fr.heads(), 0.0, 0.45, 0.0, {"total": fr.ncells, "kept": min(fr.ncells, MAX_DET), "tied": True,
                                            "cut": dict(T=0, S=len(lad), cnt=n_m, want=MAX_DET - len(lad), distinct=1, levels=0,
                                                        eidx_split=False)}
    if kind == "m200_bg_ladder":
        # three populations under conf_thr = 0: 100 ladder cells, 60 background cells (9e-14, class 0) and the rest at -200
        # (0.0, class -1). The cut falls among the zeros: bin 0 is split down to ONE key (bit pattern 0) and then by index.
        lad, bg = order[:100], order[100:160]
        fr.put_all_classes(np.setdiff1d(np.arange(fr.ncells), order[:160]), -200.0)
        fr.put(lad, rng.integers(0, min(nc, 4), 100), LADDER[rng.permutation(100)])
        return fr.heads(), 0.0, 0.45, 0.0, {"total": fr.ncells, "kept": min(fr.ncells, MAX_DET), "tied": True,
                                            "cut": dict(T=0, S=100, cnt=fr.ncells - 100, want=MAX_DET - 100, distinct=2, levels=3,
                                                        eidx_split=True)}
    if kind == "nan":
        # a cell whose class logits are all NaN never passes; a NaN beside a real logit loses the argmax to it
        lad = order[:40]
        fr.put(lad, rng.integers(0, min(nc, 4), 40), LADDER[rng.permutation(40)])
        fr.put_all_classes(order[40:50], np.nan)
        fr.put_all_classes(order[50:55], np.nan)
        fr.put(order[50:55], min(nc, 4) - 1, LADDER[100:105])
        return fr.heads(), 0.05, 0.45, 0.0, {"total": 45, "kept": 45}
    assert kind == "inf"
    # +inf -> confidence exactly 1.0 (ties by enumeration index); -inf in every class -> 0.0, never passes 0.05
    ones = np.sort(order[:70])
    fr.put(ones, rng.integers(0, min(nc, 4), 70), np.inf)
    fr.put_all_classes(order[70:80], -np.inf)
    fr.put(order[80:120], rng.integers(0, min(nc, 4), 40), LADDER[rng.permutation(40)])
    return fr.heads(), 0.05, 0.45, 0.0, {"total": 110, "kept": 110, "first_conf_one": 70, "tied": True}


# ---------------------------------------------------------------------------------------------------- cut regimes
def cut_case(grids, nc, T, cnt, want, distinct, n_below, conf_thr, levels, eidx_split, keys="spread", chain=False, ones=0):
    """More than kMaxDet candidates, laid out around ONE histogram bin T:
        S = kMaxDet - want  candidates above bin T (ladder confidences, or none)
        cnt                 members of bin T, `distinct` different confidences dealt round-robin over scattered cells
        n_below             candidates below bin T
    so the kernel must take `want` of the bin's `cnt` members, ties by enumeration index. levels = passes of the
    `while (cnt > kMemCap && khi - klo > 1u)` key-range split; eidx_split = the enumeration-index split (esh / ebin) runs after.
    keys: "spread" = evenly over the middle half of the bin; "cluster" = logits 2^-18 apart (32 confidence ulps) around the
    middle of the bin, so one level of the split cannot separate them; a tuple = those logits."""
    fr = Frame(grids, nc)
    S = MAX_DET - want
    assert 0 <= S and want <= cnt and S + cnt + n_below > MAX_DET
    rng = np.random.default_rng(100 * T + cnt + want + distinct)
    cells = np.arange(fr.ncells)
    chain_e = np.zeros(0, np.int64)
    if chain:   # 5 P2 rows of 60 chain boxes among the candidates ABOVE the bin: suppression after an overflow selection
        ys, xs = np.meshgrid(np.arange(10, 100, 20), np.arange(20, 80), indexing="ij")
        chain_e = (ys * grids[0][1] + xs).ravel()
        assert len(chain_e) <= S
        rows = np.unique(ys)
        cells = cells[~((cells < fr.off[1]) & np.isin(cells // grids[0][1], rows))]   # nothing else in those P2 rows
        fr.put(chain_e, 2, LADDER[np.arange(len(chain_e))], CHAIN_REG)               # confidence falls along each row
    order = cells[np.random.default_rng(41).permutation(len(cells))]
    n_above = S - len(chain_e)
    assert n_above + cnt + n_below <= len(order)
    above, members, below = order[:n_above], order[n_above:n_above + cnt], order[n_above + cnt:n_above + cnt + n_below]
    fr.put(above, rng.integers(0, min(nc, 4), n_above), LADDER[300 + np.arange(n_above) % 400])      # 0.86 .. 0.58
    if isinstance(keys, tuple):
        lg = np.asarray(keys, F)
    elif keys == "cluster":
        lg = (binned_logits(T, 1)[0] + F(2.0 ** -18) * (np.arange(distinct) - distinct // 2)).astype(F)
    else:
        lg = binned_logits(T, distinct)
    assert len(lg) == distinct
    fr.put(members[ones:], rng.integers(0, min(nc, 4), cnt - ones), lg[np.arange(cnt - ones) % distinct])
    fr.put(members[:ones], rng.integers(0, min(nc, 4), ones), 30.0)                                 # exactly 1.0
    if T >= 2048:
        fr.put(below, rng.integers(0, min(nc, 4), n_below), LADDER[800 + np.arange(n_below) % 600])  # 0.47 .. 0.078
    else:
        fr.put(below, rng.integers(0, min(nc, 4), n_below), -9.0)                                    # bin 0
    expect = {"total": S + cnt + n_below, "T": T, "S": S, "cnt": cnt, "want": want, "distinct": distinct + (1 if ones else 0),
              "levels": levels, "eidx_split": eidx_split, "tied": distinct <= 2}
    if chain:
        expect["share"] = (0.1, 0.2)       # 150 of the 1024 selected: every other chain box
    else:
        expect["kept"] = MAX_DET
    return fr.heads(), conf_thr, 0.45, 0.0, expect


def _mid_bin_regime(cnt, distinct):
    """Bin 2048 = [0.5, 0.5 + 2^-12): 4096 keys, so the FIRST level (wdt = 1) already tells every key apart."""
    if cnt <= MEM_CAP:
        return 0, False
    per_key = -(-cnt // distinct)
    return 1, per_key > MEM_CAP


MANY = 256   # "about cnt" distinct keys: the middle half of bin 2048 holds 2048 float32 confidences; 256 of them are 8 ulps apart,
             # the closest at which an ulp of expf on either side can neither merge nor swap two keys


def _cut_table():
    t = {}
    for cnt in (1023, 1024, 1025, 1026, 5000):
        for want in sorted({1, 2, cnt - 1, cnt, MAX_DET}):
            if not (1 <= want <= min(cnt, MAX_DET)):
                continue
            for d, dn in ((1, "1key"), (2, "2keys"), (MANY, "manykeys")):
                lv, es = _mid_bin_regime(cnt, d)
                t[f"cut-bin2048-cnt={cnt}-want={want}-{dn}"] = dict(T=2048, cnt=cnt, want=want, distinct=d, n_below=700,
                                                                    conf_thr=0.05, levels=lv, eidx_split=es)
    # low bins, conf_thr = 1e-5. Bin 0 = keys [0, 0x39800000): 9.6e8 keys, three levels down to one key; bins 1 and 3 hold 2^23
    # and 2^22 keys: two levels.
    t["cut-bin0-all-2keys"] = dict(T=0, cnt=33600, want=1024, distinct=2, n_below=0, conf_thr=1e-5, levels=3, eidx_split=True,
                                   keys=(-9.0, -9.5))
    t["cut-bin0-50keys"] = dict(T=0, cnt=6000, want=724, distinct=50, n_below=0, conf_thr=1e-5, levels=2, eidx_split=False,
                                keys="cluster")
    for T in (1, 3):
        t[f"cut-bin{T}-2keys"] = dict(T=T, cnt=5000, want=724, distinct=2, n_below=2000, conf_thr=1e-5, levels=2, eidx_split=True)
        t[f"cut-bin{T}-50keys"] = dict(T=T, cnt=5000, want=724, distinct=50, n_below=2000, conf_thr=1e-5, levels=2,
                                       eidx_split=False, keys="cluster")
    # the last bin: [4095/4096, 1.0], 4097 keys. 600 cells at exactly 1.0 and two keys below, 3000 cells each: the cut falls in
    # the upper key's 3000 -> two levels (wdt 2, then 1), then the index split
    t["cut-bin4095-2keys-and-ones"] = dict(T=4095, cnt=6600, want=1024, distinct=2, n_below=500, conf_thr=0.05, levels=2,
                                           eidx_split=True, ones=600, keys=tuple(float(v) for v in logit_of(1.0 - np.array([0.75, 0.25]) / BINS)))
    t["cut-bin2048-cnt=1025-want=2-2keys-chain"] = dict(T=2048, cnt=1025, want=2, distinct=2, n_below=700, conf_thr=0.05,
                                                        levels=1, eidx_split=False, chain=True)
    return t


# ---------------------------------------------------------------------------------------------------- registry
# name -> (builder, kwargs, engine). Engines: "s4" = 96x160, 4 classes; "s8" = 96x160, 8 classes; "l4" = 640x640, 4 classes.
CASES = {}
for _n in COUNTS:
    CASES[f"n={_n}-disjoint"] = (count_case, dict(n=_n, overlap=False), "s4")
    CASES[f"n={_n}-overlap"] = (count_case, dict(n=_n, overlap=True), "s4")
for _o in ("fall", "rr", "perm"):
    for _l, _eng in (("one", "s4"), ("byrow", "s4"), ("c1c5", "s8")):
        CASES[f"chain-{_o}-{_l}"] = (chain_case, dict(order=_o, layout=_l), _eng)
for _k in ("iou_eq", "iou_below", "equal_conf", "b_higher", "other_class"):
    CASES[f"pair-{_k}"] = (pair_case, dict(kind=_k), "s4")
for _k in ("all_m200", "part_m200", "m200_bg_ladder", "nan", "inf"):
    CASES[f"special-{_k}"] = (special_case, dict(kind=_k), "s4")
for _name, _kw in _cut_table().items():
    CASES[_name] = (cut_case, _kw, "l4")

ENGINES = {"s4": (GRIDS_96x160, 4), "s8": (GRIDS_96x160, 8), "l4": (GRIDS_640, 4)}
COUNT_NAMES = [n for n in CASES if n.startswith("n=")]
CHAIN_NAMES = [n for n in CASES if n.startswith("chain-")]
PAIR_NAMES = [n for n in CASES if n.startswith(("pair-", "special-"))]
CUT_NAMES = [n for n in CASES if n.startswith("cut-")]
# one engine, wildly different candidate counts back to back (every name is built on the 640 grids there)
SEQUENCE = ["cut-bin0-all-2keys", "n=1-disjoint", "n=0-disjoint", "n=1025-disjoint", "n=64-disjoint",
            "cut-bin2048-cnt=1025-want=2-2keys", "n=0-overlap", "chain-fall-one", "n=1023-overlap"]


def build(name, grids=None, num_classes=None):
    fn, kw, eng = CASES[name]
    g, nc = ENGINES[eng]
    return fn(tuple(grids) if grids is not None else g, num_classes if num_classes is not None else nc, **kw)


def engine_of(name):
    return CASES[name][2]
