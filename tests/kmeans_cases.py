"""Constructed inputs of the Lloyd loop (plain numpy, no GPU): the kernels behind unina_kmeans (csrc/kmeans.hip) at their
structural edges. tests/test_kmeans_cases_cpu.py proves on the CPU that every case sits where it says;
tests/test_gpu_kmeans_edges.py runs them.

The thresholds, by the kernel constant behind each:
    kTileR = 128          rows of a workgroup of kmeans_assign_kernel (32 per wave): the `row < n` guard, the zero rows of stage_tile
    kTileC = 128          centroids of a chunk, 4 MFMA tiles of 32: tiles = min(4, ceil((k - c0) / 32))
    kTileD = 32           channels staged per K step; the last step of a dim that is no multiple of 32 is padded with zeros
    kBlock = 256          the update's label scan (256 entries a step) and its channel blocks (gridDim.y = ceil(dim / 256));
                          the strided loop of kmeans_finish_kernel over 4 * ceil(n / 32) partials
    lane trip = 256       channels: kmeans_norms_kernel and kmeans_inertia_kernel walk d = lane * 4; d < dim; d += 256
    kInertiaMaxBlocks = 1024   workgroups of the inertia, reached for n > 32 768

Random data alone does not prove that a skipped trip or tile shows, so beside the random shapes there are planted cases
whose answer lives only behind the edge (the tail channels, the last centroid), and exact ties whose lower index sits in
each place where the arg-min is combined.
"""
import functools

import numpy as np

F = np.float32
TILE_R = TILE_C = 128                     # kTileR, kTileC
MFMA_TILE = 32                            # centroids of one accumulator tile
TILE_D = 32                               # kTileD
BLOCK = 256                               # kBlock
LANE_TRIP = 256                           # kWave * 4 channels
INERTIA_MAX_BLOCKS = 1024                 # kInertiaMaxBlocks
U = 2.0 ** -24


def gamma(m):
    return m * U / (1.0 - m * U)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- one step, random data -------------------------------------------------------------------------------------------
# (n, dim, k): the smallest shapes that reach each branch
ONE_STEP_SHAPES = (
    (300, 260, 5),       # dim = 256 + 4: second lane trip of one float4, second channel block of four channels, ninth K step of four
    (130, 512, 9),       # two full lane trips, two full channel blocks, 16 K steps
    (2081, 8, 7),        # 4 * ceil(2081 / 32) = 264 partials: the second trip of kmeans_finish_kernel's loop
    (32805, 4, 3),       # ceil(32805 / 32) = 1026 > kInertiaMaxBlocks: waves walk more than 8 rows
    (200, 12, 31), (200, 12, 32), (200, 12, 33),          # beside one MFMA tile of centroids
    (300, 12, 127), (300, 12, 128), (300, 12, 129),       # beside one chunk (kTileC)
    (127, 8, 4), (128, 8, 4), (129, 8, 4),                # beside one workgroup of rows (kTileR)
    (255, 8, 4), (256, 8, 4), (257, 8, 4),                # beside one step of the update's label scan (kBlock)
)


def one_step_case(n, dim, k):
    rng = np.random.RandomState(1000 * n + dim + k)
    emb = np.maximum(rng.normal(0.16, 0.24, size=(n, dim)), 0).astype(np.float32)
    emb[:, : dim // 2] -= np.float32(0.1)                                    # both signs
    start = (emb[rng.permutation(n)[:k]] * np.float32(0.9) + np.float32(0.02)).astype(np.float32)
    return emb, start


def one_step_reference(emb, start):
    """float64 on the fp32 inputs: (d2 [n, k], tol [n, k], best [n], sure [n]). tol(i, j) = 2 gamma(dim + 2) (2 sum|x c| +
    sum c^2) bounds twice the error of the device's score (tests/test_gpu_kmeans.py); a row is sure when no other centroid
    comes within tol(i, j) + tol(i, best) of the best one, and then the device's label must be `best`."""
    x, c = np.asarray(emb, np.float64), np.asarray(start, np.float64)
    n, dim = x.shape
    d2 = np.stack([((x - cj) ** 2).sum(axis=1) for cj in c], axis=1)
    tol = 2.0 * gamma(dim + 2) * (2.0 * (np.abs(x) @ np.abs(c).T) + (c * c).sum(axis=1)[None, :])
    rows = np.arange(n)
    best = d2.argmin(axis=1)
    gap = d2 - d2[rows, best][:, None] - tol - tol[rows, best][:, None]      # > 0: centroid j cannot win row i
    gap[rows, best] = np.inf
    return d2, tol, best, (gap > 0).all(axis=1)


# ---- planted cases: (emb, start, plant) ------------------------------------------------------------------------------
def tail_case(dim, n=300, k=4, head=LANE_TRIP):
    """Channels [0, head) are one fixed vector in every row and every start centroid; the clusters differ only in channels
    [head, dim): cluster j sits at (j + 1) / 2 * pattern there, rows at noise 0.03 around it, row i in cluster i % k. The
    centres are collinear and of different lengths on purpose: without the tail of |c|^2 every row goes to the LONGEST
    centroid (the largest dot product), without the tail of <x, c> to the SHORTEST (the smallest norm), and without the tail
    of the update the centroids keep the start's tail, which is 0.9 of the centre's."""
    rng = np.random.RandomState(dim)
    tail = dim - head
    fixed = rng.normal(0.16, 0.24, size=head).astype(F)
    pattern = rng.uniform(0.5, 1.0, size=tail) * (2.0 / np.sqrt(tail))       # |pattern| about 1.5 whatever the tail's length
    centres = 0.5 * (np.arange(k)[:, None] + 1) * pattern[None, :]
    plant = np.arange(n) % k
    emb = np.empty((n, dim), F)
    emb[:, :head] = fixed
    emb[:, head:] = (centres[plant] + rng.normal(0, 0.03 / np.sqrt(tail), size=(n, tail))).astype(F)
    start = np.empty((k, dim), F)
    start[:, :head] = fixed
    start[:, head:] = (0.9 * centres).astype(F)
    return emb, start, plant


@functools.lru_cache(maxsize=None)
def tail260():
    """dim = 260: the signal is the ONE float4 of the second lane trip, the four channels of the second channel block and of
    the ninth K step."""
    return frozen(*tail_case(260))


@functools.lru_cache(maxsize=None)
def tail512():
    """dim = 512: the signal is the whole second lane trip / channel block and K steps 8 .. 15."""
    return frozen(*tail_case(512))


def without_tail(case, head=LANE_TRIP):
    """The case with the tail channels zeroed in rows and start: every centroid is the same vector."""
    emb, start, plant = (a.copy() for a in case)
    emb[:, head:] = 0
    start[:, head:] = 0
    return emb, start, plant


LAST_KS = tuple(sorted({k for _, _, k in ONE_STEP_SHAPES}))                   # 3, 4, 5, 7, 9, 31, 32, 33, 127, 128, 129


@functools.lru_cache(maxsize=None)
def last_centroid(k):
    """k centres N(0, 1) in 12 channels, rows at noise 0.05 around centre i % k, the start 0.02 off the centres: every
    centroid index, the last one included, is the float64 arg-min of at least one sure row (asserted here), so a tile or a
    chunk that is skipped, or a `c0 + jl < k` guard off by one, loses labels."""
    n, dim = (200 if k <= 33 else 300), 12
    rng = np.random.RandomState(7000 + k)
    centres = rng.normal(0, 1, size=(k, dim))
    plant = np.arange(n) % k
    emb = (centres[plant] + rng.normal(0, 0.05, size=(n, dim))).astype(F)
    start = (centres + rng.normal(0, 0.02, size=(k, dim))).astype(F)
    _, _, best, sure = one_step_reference(emb, start)
    assert (best == plant).all()
    assert (np.bincount(best[sure], minlength=k) >= 1).all(), k
    return frozen(emb, start, plant)


@functools.lru_cache(maxsize=None)
def offset32():
    """300 x 64 blobs, k = 20, centres N(0, 1), noise 0.3, everything shifted by +32: |c|^2 and 2 <x, c> are about 6.5e4 each
    and differ between centroids by a few units to a few hundred, the cancellation in |c|^2 - 2 <x, c> that the bound's
    sum|x c| term pays for. Every row is sure and the float64 arg-min is the plant (asserted here)."""
    n, dim, k = 300, 64, 20
    rng = np.random.RandomState(32)
    centres = rng.normal(0, 1, size=(k, dim))
    plant = np.arange(n) % k
    emb = (centres[plant] + rng.normal(0, 0.3, size=(n, dim)) + 32.0).astype(F)
    start = (centres + 32.0).astype(F)
    _, _, best, sure = one_step_reference(emb, start)
    assert (best == plant).all() and sure.all()
    return frozen(emb, start, plant)


# ---- exact ties ------------------------------------------------------------------------------------------------------
# (low, high) start rows made identical. Where the two meet in kmeans_assign_kernel (centroid jl of a tile sits in lane half
# h = (jl >> 2) & 1, register (jl & 3) + 4 * (jl >> 3)):
TIE_PAIRS = (
    (0, 4),        # one tile, low in half 0, high in half 1: the half exchange, `oj < best_j` false
    (1, 33),       # two tiles of a chunk
    (2, 129),      # two chunks
    (3, 7),        # half 0 / half 1 once more, the last register of the first group
    (5, 8),        # low in half 1, high in half 0: the OTHER branch of the half exchange (ob == best && oj < best_j)
    (31, 32),      # the seam of two tiles; 31 is in half 1
    (63, 64),      # the next seam
    (127, 128),    # the seam of two chunks; 127 is in half 1
)
TIE_N, TIE_DIM, TIE_K = 400, 12, 130


@functools.lru_cache(maxsize=None)
def tie_case():
    """(emb, init_rows): relu-normal rows, a random start of 130 rows, and for every pair the `high` start row overwritten
    with the `low` one."""
    rng = np.random.RandomState(8)
    emb = np.maximum(rng.normal(0.16, 0.24, size=(TIE_N, TIE_DIM)), 0).astype(F)
    init = rng.permutation(TIE_N)[:TIE_K]
    for low, high in TIE_PAIRS:
        emb[init[high]] = emb[init[low]]
    return frozen(emb, init)


# ---- the loop --------------------------------------------------------------------------------------------------------
LOOP_DIM, LOOP_K, LOOP_ROWS_PER_BLOB, LOOP_SEED = 260, 33, 5, 5
LOOP_MARGIN = 10.0       # every decision of the twin's trajectory is this many tol clear (trajectory_margin)
FAR_INDEX, FAR_VALUE = 17, 50.0


def step64(emb, centroids):
    """One iteration of the twin from given centroids: (centroids, labels, inertia)."""
    from unina_yolo_dla_amd import mining
    c, labels, hist, _, _ = mining.kmeans_numpy(emb, len(centroids), None, 1, centroids=centroids)
    return c, labels, float(hist[0])


def trajectory_margin(emb, start, iters):
    """The twin's trajectory from `start`, iteration by iteration: the smallest, over iterations and rows, of
    (second-best d2 - best d2) / (tol(i, second) + tol(i, best)). Above 1 the device's label is the twin's on the SAME
    centroids. The device's centroids differ from the twin's by gamma(count + 1) mean|x| per channel (count <= 165: 1e-5
    relative), which moves a score by 2 sum_d (|x_d| + |c_d|) |delta_d|, about 2 gamma(166) / gamma(262) = 1.3 tol at most;
    at a margin of LOOP_MARGIN every device label is the twin's, and the two walk one trajectory label for label."""
    c = np.asarray(start, np.float64)
    worst = np.inf
    for _ in range(iters):
        d2, tol, best, _ = one_step_reference(emb, c)
        rows = np.arange(len(emb))
        ratio = (d2 - d2[rows, best][:, None]) / (tol + tol[rows, best][:, None])
        ratio[rows, best] = np.inf
        worst = min(worst, float(ratio.min()))
        c, _, _ = step64(emb, c)
    return worst


@functools.lru_cache(maxsize=None)
def loop_data():
    """33 blobs of 5 rows in 260 channels (centres N(0, 0.25^2), noise 0.25: a row is 4 from its blob's centre, 5.7 from its
    blob's other rows and 8 from the rows of other blobs), shuffled."""
    rng = np.random.RandomState(260)
    centres = rng.normal(0, 0.25, size=(LOOP_K, LOOP_DIM))
    n = LOOP_K * LOOP_ROWS_PER_BLOB
    emb = (centres[np.arange(n) % LOOP_K] + rng.normal(0, 0.25, size=(n, LOOP_DIM))).astype(F)
    emb = emb[rng.permutation(n)]
    return frozen(emb)[0]


@functools.lru_cache(maxsize=None)
def loop_case():
    """(emb, init_rows, twin): 33 random rows as the start, which double some blobs and miss others, so the twin needs several
    iterations (LOOP_SEED: of the first 16 seeds the one whose trajectory keeps the widest margin); twin =
    mining.kmeans_numpy(emb, 33, init_rows, 100) = (centroids, labels, history, iters, converged)."""
    from unina_yolo_dla_amd import mining
    emb = loop_data()
    init = np.random.RandomState(LOOP_SEED).permutation(len(emb))[:LOOP_K].astype(np.int64)
    twin = mining.kmeans_numpy(emb, LOOP_K, init, 100)
    return emb, init, twin


@functools.lru_cache(maxsize=None)
def far_case():
    """(emb, start, twin): the loop case's data and start rows as a centroid matrix, centroid FAR_INDEX replaced by a point
    far from all data (every channel 50): it has no member in any iteration."""
    from unina_yolo_dla_amd import mining
    emb, init, _ = loop_case()
    start = emb[init].copy()
    start[FAR_INDEX] = F(FAR_VALUE)
    twin = mining.kmeans_numpy(emb, LOOP_K, None, 100, centroids=start)
    return emb, frozen(start)[0], twin


# ---- non-finite values -----------------------------------------------------------------------------------------------
NONFINITE_ITERS = 3
NAN_ROW, INF_ROW = 11, 23


@functools.lru_cache(maxsize=None)
def nonfinite():
    """(emb [40, 8], init_rows): three tight blobs (row i in blob i % 3), one row with a NaN, one with a +inf; the start is one
    finite row per blob. Iteration 1 sends the NaN row to cluster 0 (all its scores are NaN) and makes centroid 0 NaN; from
    iteration 2 on every row's score against it is NaN."""
    rng = np.random.RandomState(40)
    centres = rng.normal(0, 1, size=(3, 8))
    emb = (centres[np.arange(40) % 3] + rng.normal(0, 0.05, size=(40, 8))).astype(F)
    assert (emb != 0).all()
    emb[NAN_ROW, 3] = np.nan
    emb[INF_ROW, 5] = np.inf
    return frozen(emb, np.array([0, 1, 2], np.int64))


def rule_labels(emb, centroids):
    """The non-finite rule spelled out row by row, in float64: a running minimum from (+inf, index 0) that only a strictly
    smaller score replaces. A NaN score never wins; a row all of whose scores are NaN or +inf keeps label 0."""
    x, c = np.asarray(emb, np.float64), np.asarray(centroids, np.float64)
    labels = np.zeros(len(x), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        cn = (c * c).sum(axis=1)
        for i, row in enumerate(x):
            best = np.inf
            for j in range(len(c)):
                s = cn[j] - 2.0 * float((row * c[j]).sum())
                if s < best:
                    best, labels[i] = s, j
    return labels
