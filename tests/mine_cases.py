"""Constructed inputs of the data-mining path (plain numpy, no GPU): difficulty scores, the pooled embedding and the two
selection loops at the structural edges of csrc/mining.hip and the nearest_* kernels of csrc/kmeans.hip.
tests/test_mine_cases_cpu.py proves on the CPU that every case sits where it says; tests/test_gpu_mine_edges.py runs them.

Scores. A score is a maximum over a level, so a case is a flat background (every logit -6: entropy 0.0173, loc_var 0.0049)
and, per level, planted cells that alone carry the level's two maxima:
    the entropy cell   one class at v_l = (0.3, 0.6, 0.9)[level]; for nc >= 2 a second class at +2.0 pulls its loc_var down to 0.24
    the loc_var cell   one class at -v_l, the rest background (loc_var 0.85 / 0.71 / 0.58)
The three levels expect three different values, so a workgroup or a class plane counted into the wrong level shows. Binary
entropy is even in the logit, so the loc_var cell carries the level's entropy too: a case with both cells cannot tell whether
the ENTROPY cell was read. Hence three roles for the cell at the swept position:
    "ent"        the entropy cell at the position, the loc_var cell in another wave             (both maxima, two cells)
    "loc"        the loc_var cell at the position, the entropy cell in another wave             (witness: loc_var)
    "ent_alone"  the entropy cell at the position and no loc_var cell in that level             (witness: both scores)
With nc = 1, or a level of one cell, there is one planted cell (class at v_l) and one role, "ent_alone".
Positions: cells 0, 63, 64, 255, 256, the first cell of the last workgroup and cells - 1 (kMineBlock 256, wave 64), each where
the level has it; the planted class at plane 0 and at plane nc - 1.

Selection. Embeddings are integers in {0, 1, 2, 3}: every fp32 sum of squares is exact in any order, so equal distances are
exact ties and the kernels must return numpy's indices, one for one.
"""
import functools

import numpy as np

F = np.float32
BLOCK, WAVE = 256, 64                     # kMineBlock, kWave
ARG_BLOCK = 1024                          # kKcArgBlock, kNrArgBlock
BG = -6.0
V = (0.3, 0.6, 0.9)
SECOND = 2.0
SCORE_SIZES = ((16, 16), (16, 272), (80, 112), (128, 128))
BIG_SIZE, BIG_NC = (1024, 1040), 4        # P2: 260 workgroups, one past a full trip of mine_finish_kernel's strided loop
CLASS_COUNTS = (1, 4, 7, 80)
SPECIALS = (88.0, -88.0, 104.0, -104.0, 1e30, -1e30, float("inf"), float("-inf"))


def grids_of(size):
    h, w = size
    return tuple((h // s, w // s) for s in (4, 8, 16))


def cells_of(size):
    return tuple(gh * gw for gh, gw in grids_of(size))


# ---- the twin in float64 ---------------------------------------------------------------------------------------------
def difficulty64(planes):
    """mining.difficulty_from_heads, the same lines in float64."""
    out = np.zeros(8, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i, x in enumerate(planes):
            x = np.asarray(x, dtype=np.float64)
            p = 1.0 / (1.0 + np.exp(-x))
            ent = -(p * np.log(p + 1e-10) + (1.0 - p) * np.log(1.0 - p + 1e-10))
            out[i] = ent.max()
            conf = p.max(axis=0)
            out[3 + i] = (1.0 - np.abs(conf - 0.5) * 2.0).max()
    out[6] = out[0:3].max()
    out[7] = out[3:6].max()
    return out


def twins(planes):
    """(fp32 twin, float64 twin) of one case."""
    from unina_yolo_dla_amd import mining
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return mining.difficulty_from_heads(planes), difficulty64(planes)


# ---- score cases -----------------------------------------------------------------------------------------------------
def positions(cells):
    """The swept cells of a level of `cells` cells, ascending, each once."""
    last_wg = (cells - 1) // BLOCK * BLOCK
    return sorted({p for p in (0, 63, 64, 255, 256, last_wg, cells - 1) if 0 <= p < cells})


def big_positions(cells):
    """P2 at BIG_SIZE: the first cell of workgroups 0, 255, 256 and 259, a cell inside each, and the last cell."""
    out = set()
    for wg in (0, 255, 256, 259):
        out.update((wg * BLOCK, wg * BLOCK + 77))
    out.add(cells - 1)
    assert max(out) < cells
    return sorted(out)


def partner(p, cells):
    """A cell other than p, in another wave where the level has more than one wave (and in another workgroup where it has
    more than one); None in a level of one cell."""
    if cells == 1:
        return None
    for q in ((p + BLOCK) % cells, (p + cells - BLOCK) % cells, (p + WAVE) % cells, (p + cells - WAVE) % cells, 0, cells - 1):
        if q != p and q // WAVE != p // WAVE and (cells <= BLOCK or q // BLOCK != p // BLOCK):
            return q
    for q in ((p + WAVE) % cells, (p + cells - WAVE) % cells, 0, cells - 1):
        if q != p and q // WAVE != p // WAVE:
            return q
    assert cells <= WAVE
    return (p + 1) % cells


def background(size, nc):
    return [np.full((nc, gh, gw), BG, F) for gh, gw in grids_of(size)]


def plant(planes, level, role, pos, plane):
    """Plants one level. Returns {"ent": cell or None, "loc": cell or None}: the cells that carry the level's maxima."""
    x = planes[level]
    nc = x.shape[0]
    flat = x.reshape(nc, -1)
    cells = flat.shape[1]
    if nc == 1 or cells == 1:
        role = "ent_alone"
    other = None if role == "ent_alone" else partner(pos, cells)
    ent_cell, loc_cell = (other, pos) if role == "loc" else (pos, other)
    flat[plane, ent_cell] = V[level]
    if nc >= 2:
        flat[(plane + 1) % nc, ent_cell] = SECOND
    if loc_cell is not None:
        flat[plane, loc_cell] = -V[level]
    return {"ent": ent_cell, "loc": loc_cell if loc_cell is not None else ent_cell}


def score_case(size, nc, role, k, plane, levels=(0, 1, 2), big=False):
    """One frame: in every level of `levels`, the role's cell at the level's k-th position (the last one where the level has
    fewer), planted class at `plane`. Returns (planes, where): where[level] = the cells of that level's maxima."""
    planes = background(size, nc)
    where = {}
    for l in levels:
        cells = planes[l][0].size
        pos = big_positions(cells) if big and l == 0 else positions(cells)
        where[l] = plant(planes, l, role, pos[min(k, len(pos) - 1)], plane)
    return planes, where


def roles_of(nc):
    return ("ent_alone",) if nc == 1 else ("ent", "loc", "ent_alone")


def planes_of(nc):
    return (0,) if nc == 1 else (0, nc - 1)


def score_case_ids(size, nc, big=False):
    """(role, k, plane) of every case of one engine: k runs over the longest position list of the three levels."""
    c = cells_of(size)
    depth = max(len(big_positions(c[0])) if big else len(positions(c[0])), len(positions(c[1])), len(positions(c[2])))
    return [(role, k, plane) for role in roles_of(nc) for k in range(depth) for plane in planes_of(nc)]


def special_case(size, nc, level, value):
    """Plants in the two other levels, `level` wholly at `value`."""
    planes, _ = score_case(size, nc, "ent", 0, 0, levels=[l for l in range(3) if l != level])
    planes[level][...] = value
    return planes


def nan_positions(cells):
    """first cell, last cell, first cell of the last workgroup"""
    return sorted({0, cells - 1, (cells - 1) // BLOCK * BLOCK})


def nan_case(size, nc, level, pos, plane):
    """The full "ent" case (plants in all three levels, first position), then one NaN in class `plane` of cell `pos` of `level`."""
    planes, _ = score_case(size, nc, "ent", 0, 0)
    planes[level].reshape(nc, -1)[plane, pos] = np.nan
    return planes


# ---- pooled embedding ------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def gamma(m):
    return m * U / (1.0 - m * U)


# (base_channels, (in_h, in_w)) -> P4 pixels; a strip is 32 pixels at 256 channels and 64 at 128
POOL_SIZES_256 = ((16, 16), (16, 48), (64, 128), (48, 176), (80, 112), (128, 128), (80, 208))
POOL_SIZES_128 = ((112, 144), (128, 128), (80, 208))
POOL_ALL_PRECISIONS = ((16, 16), (64, 128), (48, 176), (80, 208))      # 1, 32, 33, 65 pixels
POOL_SEED = 1236


def p4_pixels(size):
    return (size[0] // 16) * (size[1] // 16)


def pool_bound(x):
    """x: [C, hw] float64, the map as stored. Per channel gamma(hw + 2) * mean|x|: hw - 1 additions in any order, one
    division, one more rounding for the hi + lo add or the code x scale product."""
    return gamma(x.shape[1] + 2) * np.abs(x).mean(axis=1)


def drop_one_ratio(x):
    """For every pixel, the largest over the channels of |mean without that pixel - mean| / bound: a pool that loses a pixel
    misses the bound by this factor at least in one channel. x: [C, hw] float64, hw >= 2."""
    c, hw = x.shape
    mean = x.mean(axis=1)
    without = (x.sum(axis=1)[:, None] - x) / (hw - 1)
    bound = pool_bound(x)
    live = bound > 0
    return (np.abs(without - mean[:, None])[live] / bound[live, None]).max(axis=0)


# ---- selection loops -------------------------------------------------------------------------------------------------
KC_N = (1, 2, 8, 9, 64, 65, 1023, 1024, 1025, 4097)
KC_DIM = (1, 3, 4, 63, 64, 65, 252, 256, 260)
NR_N = (1, 8, 9, 1023, 1024, 1025, 4097)
NR_DIM = (4, 252, 256, 260)
LADDER_ROWS = (3, 4, 67, 1027, 2051)      # one thread (i, i + 1024, i + 2048), the next lane, the next wave
LADDER_N = 2100
LADDER_DIM = (4, 6)                     # k-center: the float4 and the scalar path
NR_LADDER_DIM = (4, 8)                  # nearest rows takes multiples of 4 only


@functools.lru_cache(maxsize=None)
def integer_rows(n, dim):
    """[n, dim] float32 integers in {0..3}; row n//2 = row 1 and row n-1 = row 0 (from 4 rows on). From 63 channels on, row 1
    is 3 - row 0, the far corner: the farthest row from row 0, twice (exact tie, a lower and a higher index)."""
    x = np.random.RandomState(7919 * n + dim).randint(0, 4, size=(n, dim)).astype(F)
    if n >= 4:
        if dim >= 63:
            x[1] = F(3) - x[0]
        x[n // 2] = x[1]
        x[n - 1] = x[0]
    x.setflags(write=False)
    return x


def kcenter_cases(n, dim):
    """[(embeddings, k, first_index)]"""
    x = integer_rows(n, dim)
    ks = sorted({min(n, 40)} | ({n} if n <= 65 else set()))
    return [(x, k, first) for k in ks for first in sorted({0, n - 1})]


def ladder_rows(dim, rows=LADDER_ROWS):
    x = np.zeros((LADDER_N, dim), F)
    x[list(rows)] = (np.arange(dim) % 3 + 1).astype(F)
    return x


def kcenter_ladder_cases(dim):
    """All rows zero but equal rows at LADDER_ROWS[i:], i = 0..3: the first pick is a tie whose lowest index is met in a
    thread's own strided loop, in the next lane, in the next wave, in the serial pass; every later pick is a tie of all rows."""
    return [(ladder_rows(dim, LADDER_ROWS[i:]), 8, 0) for i in range(len(LADDER_ROWS) - 1)]


def nearest_case(n, dim):
    """(embeddings, centroids). Centroids: data rows 0 and 1 (each duplicated in the data) given twice, so the second copy
    must take the duplicate and the rest must keep off both; the others are fresh integer rows."""
    x = integer_rows(n, dim)
    k = n if n <= 9 else min(n, 12)
    c = np.random.RandomState(104729 * n + dim).randint(0, 4, size=(k, dim)).astype(F)
    if n >= 4:
        for j, r in ((0, 0), (1, 0), (2, 1), (k - 1, 1), (k // 2, 0)):
            c[j] = x[r]
    return x, c


def nearest_ladder_case(dim):
    """Six copies of the ladder's row as centroids: the picks walk LADDER_ROWS in order, then row 0."""
    x = ladder_rows(dim)
    return x, np.repeat(x[LADDER_ROWS[0]][None], len(LADDER_ROWS) + 1, axis=0)


def kcenter_trace(x, k, first, dtype=np.float64, perm=None):
    """mining.kcenter_numpy's loop in `dtype` (channels in `perm` order), with the tie record: (selected, tied[k-1]):
    tied[t] = more than one row holds the top distance at step t + 1."""
    x = np.asarray(x, dtype=dtype)
    if perm is not None:
        x = x[:, perm]
    n = x.shape[0]
    sel, tied = [int(first)], []
    md = np.full(n, np.inf)
    for _ in range(k - 1):
        md = np.minimum(md, np.linalg.norm(x - x[sel[-1]], axis=1))
        md[sel] = -1
        sel.append(int(np.argmax(md)))
        tied.append(int((md == md.max()).sum()) > 1)
    return np.asarray(sel, np.int64), np.asarray(tied, bool)


def nearest_trace(x, c, dtype=np.float64, perm=None):
    """mining.nearest_rows_numpy's loop in `dtype`, with the tie record."""
    x, c = np.asarray(x, dtype=dtype), np.asarray(c, dtype=dtype)
    if perm is not None:
        x, c = x[:, perm], c[:, perm]
    sel, tied = [], []
    for cen in c:
        d = np.linalg.norm(x - cen, axis=1).astype(np.float64)
        d[sel] = np.inf
        sel.append(int(np.argmin(d)))
        tied.append(int((d == d.min()).sum()) > 1)
    return np.asarray(sel, np.int64), np.asarray(tied, bool)


def clear_step_possible(n, dim):
    """A step with ONE row at the top can be asked for where the data can be all different: fewer rows than the 4^dim points
    of the integer grid. (Beyond that random rows repeat everywhere and every top is shared.)"""
    return n < 4 ** dim
