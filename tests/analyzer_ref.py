"""Not a test: a numpy restatement of the Analyzer over an export() dict (keys, vecs, deg, adj,
entry, dead) -- analyzer.go's QualityMetrics with the engine's stated policies (the sample is the
first min(100, NodeCount) live layer-0 rows in ascending row id, pairs i < j in nested order, the
standard deviation summed over the degree histogram in ascending degree), estimateGraphDistance
for every pair of a row set, the reachability of the rows from the top layer's entry down the
layers, and a layer's degree histogram.

A row is a live member of layer l when deg[l] != -2 and it is not deleted.  Every walk follows
every stored edge (positions below deg, ids >= 0), through deleted rows too."""
import math

import numpy as np

from tests import batch_ref as BR

MAX_DEPTH = 10  # analyzer.go:211

# The 1,531-row batch graph of the GPU tests (1,531: no multiple of 32 or 64) as a batch_ref
# case, and the seed of its crafted unreachable rows: test_analyzer_ref.py pins that the oracle's
# relink of them drops no reverse proposal and leaves no row unreachable.
REPAIR_CASE = BR._case(d=24, n=1531, M=16, m0=32, ef_construction=64, heuristic=2, keep_pruned=1, script=(("add", 1, 1),))
REPAIR_SEED = 3


def live(ex, l):
    return (ex["deg"][l] != -2) & (ex["dead"] == 0)


def neighbours(ex, l, i):
    d = max(int(ex["deg"][l, i]), 0)
    row = ex["adj"][l, i, :d]
    return row[row >= 0]


def degree_histogram(ex, layer):
    """int64[64]: live members of the layer by degree (below 0 counts as 0)"""
    if layer >= ex["deg"].shape[0]:
        return np.zeros(64, np.int64)
    d = np.maximum(ex["deg"][layer][live(ex, layer)], 0)
    assert d.size == 0 or d.max() < 64
    return np.bincount(d, minlength=64).astype(np.int64)


def _bfs_levels(ex, l, seeds, max_depth=None):
    """level of every row reached in layer l from `seeds` (level 0), -1 elsewhere, and the number
    of levels expanded until the frontier emptied (or max_depth)"""
    deg, adj = ex["deg"][l], ex["adj"][l]
    slot = np.arange(adj.shape[1])[None, :]
    level = np.full(deg.shape[0], -1, np.int64)
    frontier = np.unique(np.asarray(seeds, np.int64))
    level[frontier] = 0
    depth = 0
    while frontier.size and (max_depth is None or depth < max_depth):
        depth += 1
        rows = adj[frontier]  # (the rows' neighbours(): positions below deg, ids >= 0)
        nb = np.unique(rows[(slot < deg[frontier][:, None]) & (rows >= 0)])
        frontier = nb[level[nb] < 0].astype(np.int64)
        level[frontier] = depth
    return level, depth


def hops(ex, rows, max_depth=MAX_DEPTH):
    """int32[n, n]: edges on the shortest directed layer-0 path rows[i] -> rows[j], 0 on the
    diagonal, -1 without a path of at most max_depth edges (analyzer.go:193-240)"""
    rows = np.asarray(rows, np.int64)
    out = np.full((len(rows), len(rows)), -1, np.int32)
    for i, r in enumerate(rows):
        level, _ = _bfs_levels(ex, 0, [r], max_depth)
        out[i] = level[rows]
    return out


def reachability(ex):
    """dict(members, reached, depth: one entry per layer; unreachable: the live layer-0 rows no
    search can visit, ascending).  T = the highest layer with a live member, R_T = what its
    entry reaches there, R_l = what R_(l+1)'s members of layer l (deg != -2) reach in layer l."""
    L = ex["deg"].shape[0]
    members, reached, depth = [0] * L, [0] * L, [0] * L
    tops = [l for l in range(L) if live(ex, l).any()]
    if not tops:
        return dict(members=members, reached=reached, depth=depth, unreachable=np.zeros(0, np.int64))
    T = tops[-1]
    R = None
    for l in range(T, -1, -1):
        if l == T:
            seeds = [int(ex["entry"][T])] if ex["entry"][T] >= 0 else []
        else:
            seeds = np.flatnonzero(R & (ex["deg"][l] != -2))
        level, depth[l] = _bfs_levels(ex, l, seeds)
        R = level >= 0
        members[l] = int(live(ex, l).sum())
        reached[l] = int((live(ex, l) & R).sum())
    return dict(members=members, reached=reached, depth=depth, unreachable=np.flatnonzero(live(ex, 0) & ~R))


def craft_unreachable(ex, seed, count=25):
    """The reachability tests' crafted graph: `count` live level-0 rows U that are no layer's
    entry lose every in-edge (the adjacency rows are closed up, order kept).  -> (a new export,
    U ascending)"""
    rng = np.random.default_rng(seed)
    L, N = ex["deg"].shape
    level0 = live(ex, 0) & ~(ex["deg"][1:] != -2).any(axis=0)
    level0[ex["entry"][ex["entry"] >= 0]] = False
    U = np.sort(rng.choice(np.flatnonzero(level0), count, replace=False))
    out = {k: v.copy() for k, v in ex.items()}
    for l in range(L):
        for i in np.flatnonzero(ex["deg"][l] > 0):
            row = ex["adj"][l, i, : ex["deg"][l, i]]
            kept = row[~np.isin(row, U)]
            out["adj"][l, i, :] = -1
            out["adj"][l, i, : len(kept)] = kept
            out["deg"][l, i] = len(kept)
    return out, U


def layer_balance(counts, ml):
    """analyzer.go:245-279 over the layers' live member counts"""
    L = len(counts)
    if L <= 1 or ml <= 0 or ml >= 1 or counts[0] == 0:
        return 0.0
    s = 0.0
    for i in range(1, L):
        expected = float(counts[0]) * math.pow(ml, float(i))
        if expected == 0:
            continue
        ratio = float(counts[i]) / expected
        if ratio > 1:
            ratio = 1 / ratio
        s += ratio
    return s / float(L - 1)


def sample_rows(ex):
    return np.flatnonzero(live(ex, 0))[:100]


def quality_metrics(ex, ml, dist):
    """analyzer.go:51-67 -> dict with the reference's field names; dist(i, j): the float32
    distance with q = row i's vector and X = row j's"""
    L = ex["deg"].shape[0]
    out = dict(NodeCount=0, AvgConnectivity=0.0, ConnectivityStdDev=0.0, DistortionRatio=0.0, LayerBalance=0.0,
               GraphHeight=L)
    if L == 0:
        return out
    hist = degree_histogram(ex, 0)
    nodes = int(hist.sum())
    out["NodeCount"] = nodes
    if nodes:
        avg = int((hist * np.arange(64)).sum()) / nodes
        ss = 0.0
        for d in range(64):
            if hist[d]:
                ss += float(hist[d]) * ((float(d) - avg) * (float(d) - avg))
        out["AvgConnectivity"] = avg
        out["ConnectivityStdDev"] = math.sqrt(ss / nodes)
    if nodes >= 10:
        S = sample_rows(ex)
        hp = hops(ex, S)
        total, pairs = np.float64(0.0), 0
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(len(S)):
                for j in range(i + 1, len(S)):
                    a = np.float64(np.float32(dist(int(S[i]), int(S[j]))))
                    if hp[i, j] > 0 and np.isfinite(a):
                        total = total + np.float64(hp[i, j]) / a  # a zero distance: +Inf, as in Go
                        pairs += 1
            if pairs:
                out["DistortionRatio"] = float(total / np.float64(pairs))
    out["LayerBalance"] = layer_balance([int(live(ex, l).sum()) for l in range(L)], ml)
    return out
