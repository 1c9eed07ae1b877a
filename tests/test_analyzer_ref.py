"""CPU: tests/analyzer_ref.py, the restatement the GPU tests compare the Analyzer with, pinned
on its own: the reference's cases of analyzer_test.go on oracle-built graphs, hops against
scipy's shortest paths and reachability against networkx closures on small random graphs, and
the input of the Repair test (the crafted graph, relinked by the oracle's update)."""
import math

import numpy as np
import pytest

from tests import analyzer_ref as AR
from tests import batch_ref as BR

REPAIR_CASE, REPAIR_SEED = AR.REPAIR_CASE, AR.REPAIR_SEED


def _line_graph(O, n):
    """analyzer_test.go: newTestGraph (graph_test.go:76-84) with Vector{float32(i)} for key i"""
    g = O.Graph(metric=O.EUCLIDEAN, order=O.ORDER_REF, M=6, Ml=0.5, EfSearch=20, seed=0)
    if n:
        g.add(np.arange(n), np.arange(n, dtype=np.float32).reshape(n, 1))
    return g


def _dist_of(O, ex, metric=1):
    return lambda i, j: O.distance(metric, O.ORDER_REF, ex["vecs"][j], ex["vecs"][i])


def test_empty_graph_is_all_zero(O):
    # TestAnalyzer_EmptyGraph, and the first half of TestAnalyzer_QualityMetrics
    ex = _line_graph(O, 0).export()
    m = AR.quality_metrics(ex, 0.5, None)
    assert m == dict(NodeCount=0, AvgConnectivity=0.0, ConnectivityStdDev=0.0, DistortionRatio=0.0, LayerBalance=0.0,
                     GraphHeight=0)
    r = AR.reachability(ex)
    assert r["members"] == [] and r["reached"] == [] and len(r["unreachable"]) == 0


@pytest.mark.parametrize("n", [100, 20])
def test_reference_properties(O, n):
    # TestAnalyzer_QualityMetrics (100), _DistortionRatio (20), _ConnectivityMetrics, _LayerBalance
    g = _line_graph(O, n)
    ex = g.export()
    m = AR.quality_metrics(ex, 0.5, _dist_of(O, ex))
    assert m["NodeCount"] == n
    assert 0.0 < m["AvgConnectivity"] <= 6.0
    assert m["ConnectivityStdDev"] >= 0.0
    assert m["GraphHeight"] >= 1 and m["GraphHeight"] == len(g.topography())
    assert 0.0 <= m["LayerBalance"] <= 1.0
    assert m["DistortionRatio"] >= 0.0 and math.isfinite(m["DistortionRatio"])
    deg = np.maximum(ex["deg"][0], 0)
    assert m["AvgConnectivity"] == deg.sum() / n
    assert abs(m["ConnectivityStdDev"] - np.std(deg.astype(np.float64))) <= 1e-12 * max(1.0, m["ConnectivityStdDev"])
    assert AR.degree_histogram(ex, 0).sum() == n
    r = AR.reachability(ex)
    assert r["members"] == g.topography()
    assert all(0 < a <= b for a, b in zip(r["reached"], r["members"]))
    assert len(r["unreachable"]) == r["members"][0] - r["reached"][0]


def test_line_of_four(O):
    # TestAnalyzer_EstimateGraphDistance
    ex = _line_graph(O, 4).export()
    hp = AR.hops(ex, [0, 1, 3])
    assert hp[0, 0] == 0 and hp[1, 1] == 0 and hp[2, 2] == 0
    assert hp[0, 1] >= 0 and hp[0, 2] >= 0
    assert AR.quality_metrics(ex, 0.5, _dist_of(O, ex))["DistortionRatio"] == 0.0  # fewer than 10 rows


def _random_export(rng, N, L, cap, p_dead=0.1):
    """a random layered digraph in export form: nested membership, random rows with duplicates,
    self-loops and edges to deleted rows"""
    deg = np.full((L, N), -2, np.int32)
    adj = np.full((L, N, cap), -1, np.int32)
    level = np.minimum(rng.geometric(0.5, N) - 1, L - 1)
    level[rng.integers(N)] = L - 1
    dead = (rng.random(N) < p_dead).astype(np.uint8)
    entry = np.full(L, -1, np.int32)
    for l in range(L):
        mem = np.flatnonzero(level >= l)
        for i in mem:
            d = int(rng.integers(0, min(cap, 3) + 1))
            deg[l, i] = d
            adj[l, i, :d] = rng.choice(mem, d)
        livem = mem[dead[mem] == 0]
        if len(livem):
            entry[l] = livem[0]
    return dict(keys=np.arange(N, dtype=np.int64), vecs=rng.normal(size=(N, 4)).astype(np.float32), deg=deg, adj=adj,
                entry=entry, dead=dead)


@pytest.mark.parametrize("seed", range(6))
def test_hops_match_scipy(seed):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path

    rng = np.random.default_rng(seed)
    N = int(rng.integers(5, 61))
    ex = _random_export(rng, N, 3, 5)
    A = np.zeros((N, N), np.int8)
    for i in range(N):
        A[i, AR.neighbours(ex, 0, i)] = 1
    np.fill_diagonal(A, 0)
    D = shortest_path(csr_matrix(A), directed=True, unweighted=True)
    rows = np.flatnonzero(AR.live(ex, 0))
    for depth in (1, 3, 10):
        want = np.where(D[np.ix_(rows, rows)] <= depth, D[np.ix_(rows, rows)], -1).astype(np.int32)
        assert np.array_equal(AR.hops(ex, rows, depth), want), depth


@pytest.mark.parametrize("seed", range(6))
def test_reachability_matches_closure(seed):
    import networkx as nx

    rng = np.random.default_rng(100 + seed)
    N = int(rng.integers(5, 61))
    ex = _random_export(rng, N, 4, 5, p_dead=0.2)
    got = AR.reachability(ex)
    L = 4
    tops = [l for l in range(L) if AR.live(ex, l).any()]
    T = tops[-1]
    R = None
    for l in range(T, -1, -1):
        G = nx.DiGraph()
        G.add_nodes_from(range(N))
        G.add_edges_from((i, int(j)) for i in range(N) for j in AR.neighbours(ex, l, i))
        seeds = [int(ex["entry"][T])] if l == T else [i for i in R if ex["deg"][l, i] != -2]
        R = set(seeds)
        for s in seeds:
            R |= nx.descendants(G, s)
        livel = set(np.flatnonzero(AR.live(ex, l)).tolist())
        assert got["members"][l] == len(livel) and got["reached"][l] == len(livel & R), l
        # levels run: the eccentricity of the seed set, plus the level that finds nothing new
        if seeds:
            ecc = max(nx.multi_source_dijkstra_path_length(G, set(seeds)).values())
            assert got["depth"][l] == ecc + 1, l
        else:
            assert got["depth"][l] == 0
    assert got["unreachable"].tolist() == sorted(set(np.flatnonzero(AR.live(ex, 0)).tolist()) - R)
    for l in range(T + 1, L):
        assert got["members"][l] == 0 and got["reached"][l] == 0 and got["depth"][l] == 0


def test_repair_input_is_pinned(O):
    """The crafted graph of the GPU Repair test: on the oracle's build of the same case, the 25
    rows of REPAIR_SEED are exactly the unreachable ones, and the oracle's update of them with
    their own vectors (what Relink restates) drops no reverse proposal and leaves none."""
    drv = BR.run_oracle(O, REPAIR_CASE, 0)
    ex = drv.export()
    assert len(AR.reachability(ex)["unreachable"]) == 0
    crafted, U = AR.craft_unreachable(ex, REPAIR_SEED)
    assert AR.reachability(crafted)["unreachable"].tolist() == U.tolist() and len(U) == 25
    sh = REPAIR_CASE["shape"]
    o = O.Graph(metric=0, order=O.ORDER_DEV, M=sh["M"], M0=sh["m0"], Ml=0.25, EfSearch=64, seed=BR.RNG_SEED)
    o.import_graph(**crafted)
    found, cn = o.update(crafted["keys"][U], crafted["vecs"][U], **REPAIR_CASE["opts"])
    assert found.all() and cn["dropped_proposals"] == 0
    after = o.export()
    assert np.array_equal(after["vecs"].view(np.uint32), crafted["vecs"].view(np.uint32))
    assert len(AR.reachability(after)["unreachable"]) == 0
