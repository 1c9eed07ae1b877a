"""GPU: the Analyzer on the device (QualityMetrics, DegreeHistogram, Hops, Reachability, Repair)
and Graph.Relink.  Every comparison with tests/analyzer_ref.py on the handle's own export is bit
for bit: doubles through their uint64 image, lists and matrices with array_equal.  The built
graphs are small (1,531 rows: no multiple of 32 or 64, several workgroups); the hand-built
imports are the shapes at which a BFS kernel goes wrong -- the depth limit, a bitmap's tail
word, a seed that is no member, a row only a deleted row points at."""
import numpy as np
import pytest

from tests import analyzer_ref as AR
from tests import batch_ref as BR
from tests.test_gpu_compact import _pattern
from tests.test_gpu_parity import _metric_fn

pytestmark = pytest.mark.gpu

CASE = AR.REPAIR_CASE
N, D = CASE["shape"]["n"], CASE["shape"]["d"]


def _batch_graph(H, metric, n=N, M=None, m0=None, **opts):
    sh = CASE["shape"]
    o = dict(CASE["opts"])
    o.update(opts)
    g = H.Graph(M=M or sh["M"], Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=BR.RNG_SEED,
                build_mode=H.BUILD_BATCH, m0=m0 or sh["m0"], **o)
    gen, X, labels = BR.data_of(CASE, metric)
    keys = BR.keys_of(n)
    if n:
        g.add_arrays(keys, X[:n])
    return g, gen, X[:n], labels[:n], keys


def _bits(x):
    return np.asarray([x], np.float64).view(np.uint64)[0]


def _dist_of(H, metric, ex):
    """dist(i, j) of the restatement: mhnsw_distance, q = row i's vector, X = row j's"""
    fn = _metric_fn(H, metric)
    S = AR.sample_rows(ex) if ex["deg"].shape[0] else np.zeros(0, np.int64)
    pos = {int(r): k for k, r in enumerate(S)}
    Dm = np.stack([fn.sweep(ex["vecs"][i], ex["vecs"][S]) for i in S]) if len(S) >= 10 else None
    return lambda i, j: Dm[pos[i], pos[j]]


def _check(H, g, metric, hop_rows=24):
    """the whole Analyzer against the restatement on the handle's export"""
    an = H.Analyzer(g)
    ex = g.export()
    L = ex["deg"].shape[0]
    want = AR.quality_metrics(ex, g.Ml, _dist_of(H, metric, ex))
    got = an.QualityMetrics()
    print("quality", got, want)
    assert got.NodeCount == want["NodeCount"] and got.GraphHeight == want["GraphHeight"] == an.Height()
    for f in ("AvgConnectivity", "ConnectivityStdDev", "DistortionRatio", "LayerBalance"):
        assert _bits(getattr(got, f)) == _bits(want[f]), (f, getattr(got, f), want[f])
    for l in range(L):
        assert np.array_equal(an.DegreeHistogram(l), AR.degree_histogram(ex, l)), l
    if got.NodeCount:
        deg = np.maximum(ex["deg"][0][AR.live(ex, 0)], 0).astype(np.float64)
        assert abs(got.ConnectivityStdDev - np.std(deg)) <= 1e-9 * max(np.std(deg), 1e-300)
        assert got.AvgConnectivity == an.Connectivity()[0]
    assert an.Topography() == g.Topography()
    r, w = an.Reachability(), AR.reachability(ex)
    print("reach", r.members, r.reached, r.depth, len(r.unreachable_keys))
    assert r.members == w["members"] and r.reached == w["reached"] and r.depth == w["depth"]
    assert r.members == g.Topography()
    assert r.unreachable_keys == ex["keys"][w["unreachable"]].tolist()
    rows = np.flatnonzero(AR.live(ex, 0)) if L else np.zeros(0, np.int64)
    if len(rows):
        rows = rows[np.unique(np.linspace(0, len(rows) - 1, hop_rows).astype(int))]
        for depth in (10, 2):
            assert np.array_equal(an.Hops(ex["keys"][rows], depth), AR.hops(ex, rows, depth)), depth
    return ex, got, r


# ---- built graphs ----
@pytest.mark.parametrize("metric", [0, 1])
def test_built_deleted_compacted_updated(H, metric):
    g, gen, X, labels, keys = _batch_graph(H, metric)
    _, _, r = _check(H, g, metric)
    assert r.unreachable_keys == []  # (the crafted graph starts from here)
    dead = _pattern(N, np.random.default_rng(7 + metric))
    assert all(g.BatchDelete(keys[dead]))
    ex, q, r = _check(H, g, metric)
    assert q.NodeCount == int((~dead).sum()) == r.members[0]
    assert g.Compact() == int(dead.sum())
    _check(H, g, metric)
    live = np.flatnonzero(~dead)
    rows = live[np.linspace(0, len(live) - 1, 150).astype(int)]
    assert g.update_arrays(keys[rows], gen.moved(labels[rows])).all()
    _check(H, g, metric)
    g.close()


def test_compat_graph_with_deletes(H):
    rng = np.random.default_rng(11)
    n = 700
    X = BR.clustered(rng, n, D)
    keys = BR.keys_of(n)
    g = H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=H.CosineDistance, Rng=3)
    g.add_arrays(keys, X)
    gone = rng.permutation(n)[:60]
    assert all(g.BatchDelete(keys[gone]))
    ex, q, r = _check(H, g, 0)
    assert q.NodeCount == n - 60 == r.members[0] and r.reached[0] <= r.members[0]
    g.close()


def test_every_lane_live(H):
    # M0 63: rows of 63 neighbours, cap 64 -- every lane of the wave holds an edge
    g, *_ = _batch_graph(H, 1, n=700, M=32, m0=63)
    ex, _, _ = _check(H, g, 1)
    assert ex["adj"].shape[2] == 64 and ex["deg"][0].max() > 32
    g.close()


@pytest.mark.parametrize("n", [1, 9, 33])
def test_small_graphs(H, n):
    g, *_ = _batch_graph(H, 0, n=n)
    _, q, r = _check(H, g, 0)
    assert q.NodeCount == n and (n >= 10 or q.DistortionRatio == 0.0)
    assert r.unreachable_keys == []
    g.close()


def test_empty_and_single_layer(H):
    g, *_ = _batch_graph(H, 0, n=0)
    an = H.Analyzer(g)
    assert an.QualityMetrics() == H.GraphQualityMetrics() and an.Height() == 0
    r = an.Reachability()
    assert r.members == [] and r.reached == [] and r.depth == [] and r.unreachable_keys == []
    assert an.Repair() == (0, 0)
    g.close()
    g = H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=H.EuclideanDistance, Rng=3, build_mode=H.BUILD_BATCH)
    g.add_arrays(np.arange(40), BR.clustered(np.random.default_rng(2), 40, D), levels=np.zeros(40, np.int32))
    _, q, _ = _check(H, g, 1)
    assert q.GraphHeight == 1 and q.LayerBalance == 0.0
    g.close()


# ---- hand-built imports ----
def _import(H, deg, adj, entry, dead=None, vecs=None, metric=1):
    deg = np.asarray(deg, np.int32)
    L, n = deg.shape
    if vecs is None:
        vecs = np.arange(n * 4, dtype=np.float32).reshape(n, 4) ** 1.5 + 1
    g = H.Graph(M=4, Ml=0.25, EfSearch=16, Distance=_metric_fn(H, metric), build_mode=H.BUILD_BATCH, m0=8)
    g.import_graph(np.arange(n, dtype=np.int64) * 2 + 1, vecs, deg, np.asarray(adj, np.int32), entry, dead)
    return g


def _rows(n, cap, edges):
    """deg, adj of one layer from {row: [neighbours]} (rows not named: degree 0)"""
    deg, adj = np.zeros(n, np.int32), np.full((n, cap), -1, np.int32)
    for i, nb in edges.items():
        deg[i] = len(nb)
        adj[i, : len(nb)] = nb
    return deg, adj


def _chain(H):
    deg, adj = _rows(13, 4, {i: [i + 1] for i in range(11)})  # 0 -> 1 -> ... -> 11; 12 apart
    return _import(H, [deg], [adj], [0])


def test_chain_depth_limit(H):
    g = _chain(H)
    keys = np.arange(13) * 2 + 1
    hp = H.Analyzer(g).Hops(keys)
    assert hp[0, 10] == 10 and hp[0, 11] == -1 and hp[11, 0] == -1 and hp[1, 11] == 10
    assert np.array_equal(hp, AR.hops(g.export(), np.arange(13)))
    _check(H, g, 1, hop_rows=13)
    g.close()


def test_chain_depth_three(H):
    g = _chain(H)
    hp = H.Analyzer(g).Hops(np.arange(13) * 2 + 1, max_depth=3)
    assert hp[0, 3] == 3 and hp[0, 4] == -1 and hp[8, 11] == 3 and hp[7, 11] == -1
    assert np.array_equal(hp, AR.hops(g.export(), np.arange(13), 3))
    g.close()


def test_two_islands_member_seed(H):
    """Layer 0 is two islands, {0..4} and {5..9}.  The top layer's entry 0 reaches row 7 in layer 1
    only: layer 0's second island is visited through the seed 7, not from the entry.  Row 8 of
    the top walk is deleted and no member of layer 0 (deg -2): no seed."""
    n, cap = 70, 4  # (70 rows: the bitmaps have a tail word)
    d0, a0 = _rows(n, cap, {0: [1], 1: [2], 2: [3], 3: [4], 4: [0], 5: [6], 6: [5], 7: [5], 9: [7], 40: [69], 69: [40]})
    d1, a1 = _rows(n, cap, {0: [7, 8], 7: [0], 8: [0]})
    d1[[i for i in range(n) if i not in (0, 7, 8)]] = -2
    d0[8] = -2
    dead = np.zeros(n, np.uint8)
    dead[8] = 1
    g = _import(H, [d0, d1], [a0, a1], [0, 0], dead)
    ex, _, r = _check(H, g, 1)
    assert r.members == [n - 1, 2] and r.reached == [8, 2]  # 0..4, 7, 5, 6
    reach0 = set(range(5)) | {5, 6, 7}
    assert r.unreachable_keys == [2 * i + 1 for i in range(n) if i not in reach0 and i != 8]
    g.close()


def test_in_edge_from_dead_row_only(H):
    # row 3's only in-edge comes from the deleted row 2, which routes: 3 is reachable, 2 not counted
    d0, a0 = _rows(6, 4, {0: [1], 1: [2], 2: [3], 3: [0]})
    dead = np.zeros(6, np.uint8)
    dead[2] = 1
    g = _import(H, [d0], [a0], [0], dead)
    _, _, r = _check(H, g, 1, hop_rows=6)
    assert r.members == [5] and r.reached == [3] and r.unreachable_keys == [9, 11]
    hp = H.Analyzer(g).Hops([1, 7])
    assert hp[0, 1] == 3
    g.close()


def test_identical_vectors_give_infinite_distortion(H):
    n = 12
    vecs = np.arange(n * 4, dtype=np.float32).reshape(n, 4) + 1
    vecs[5] = vecs[2]
    d0, a0 = _rows(n, 4, {i: [(i + 1) % n] for i in range(n)})
    g = _import(H, [d0], [a0], [0], vecs=vecs)
    _, q, _ = _check(H, g, 1, hop_rows=12)
    assert q.DistortionRatio == np.inf
    g.close()


def test_self_loop_and_duplicate_neighbour(H):
    n = 11
    d0, a0 = _rows(n, 4, {i: [i, (i + 1) % n, (i + 1) % n] for i in range(n - 1)})
    g = _import(H, [d0], [a0], [0])
    _, q, r = _check(H, g, 1, hop_rows=11)
    assert r.reached == [n] and q.AvgConnectivity == 30 / 11
    hp = H.Analyzer(g).Hops([1, 21])
    assert hp[0, 1] == 10 and hp[1, 0] == -1
    g.close()


# ---- hops ----
def test_hops_properties(H):
    g, _, X, _, keys = _batch_graph(H, 0)
    an = H.Analyzer(g)
    ex = g.export()
    rows = np.unique(np.linspace(0, N - 1, 128).astype(int))
    assert len(rows) == 128
    hp = an.Hops(keys[rows])
    assert hp.dtype == np.int32 and np.array_equal(hp, AR.hops(ex, rows))
    for _ in range(2):
        assert np.array_equal(an.Hops(keys[rows]), hp)
    S = AR.sample_rows(ex)
    full = an.Hops(keys[S])
    assert np.array_equal(full[:40, :40], an.Hops(keys[S[:40]])) and np.array_equal(full, AR.hops(ex, S))
    with pytest.raises(H.HnswError, match="hops supports at most 128 keys") as e:
        an.Hops(keys[:129])
    assert e.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match="duplicate key 10 in hops") as e:
        an.Hops([7, 10, 13, 10])
    assert e.value.code == H._lib.EINVAL
    assert g.Delete(int(keys[5]))
    with pytest.raises(H.HnswError, match=f"key {keys[5]} has no live layer-0 row") as e:
        an.Hops(keys[3:8])
    assert e.value.code == H._lib.EINVAL
    with pytest.raises(H.HnswError, match="no live layer-0 row"):
        an.Hops([8])  # never added
    g.close()


def test_refusals(H):
    f = H.Graph(Distance=H.CosineDistance, build_mode=H.BUILD_FLAT)
    f.add_arrays(np.arange(20), np.random.default_rng(0).normal(size=(20, 8)).astype(np.float32))
    an = H.Analyzer(f)
    for call in (an.QualityMetrics, an.Reachability, lambda: an.Hops([1, 2])):
        with pytest.raises(H.HnswError, match=r"analyzer needs a compat or batch \(build_mode 0 or 1\) handle") as e:
            call()
        assert e.value.code == H._lib.EUNSUPPORTED
    assert f.Relink([1, 2, 99]) == [True, True, False]
    f.close()
    c = H.Graph(M=8, Distance=H.CosineDistance)
    X = np.random.default_rng(1).normal(size=(30, 8)).astype(np.float32)
    c.add_arrays(np.arange(30), X)
    with pytest.raises(H.HnswError, match=r"update needs a batch or flat \(build_mode 1 or 2\) handle"):
        c.Relink([1, 2])
    with pytest.raises(H.HnswError, match="node not added"):  # graph.go:1015-1037: replaced, then the error
        c.add_arrays(np.array([4]), X[:1])  # a replaced key: several rows of one key
    an = H.Analyzer(c)
    for call in (an.QualityMetrics, an.Reachability, lambda: an.Hops([1, 2]), an.DegreeHistogram):
        with pytest.raises(H.HnswError, match="replaced or re-added key") as e:
            call()
        assert e.value.code == H._lib.EUNSUPPORTED
    c.close()


def test_out_of_range_id_is_reported(H):
    d0, a0 = _rows(8, 4, {0: [1], 1: [5000], 2: [0]})
    g = _import(H, [d0], [a0], [0])
    an = H.Analyzer(g)
    for call in (an.Reachability, lambda: an.Hops([1, 3])):
        with pytest.raises(H.HnswError, match=r"out-of-range node id in adjacency \(graph corrupt\)"):
            call()
    g.close()


# ---- the crafted graph: reachability and repair ----
def test_crafted_unreachable_rows_and_repair(H):
    g0, *_ = _batch_graph(H, 0)
    ex = g0.export()
    g0.close()
    assert len(AR.reachability(ex)["unreachable"]) == 0
    crafted, U = AR.craft_unreachable(ex, AR.REPAIR_SEED)
    g = _batch_graph(H, 0, n=0)[0]
    g.import_graph(**crafted)
    an = H.Analyzer(g)
    r = an.Reachability()
    assert r.unreachable_keys == crafted["keys"][U].tolist() and len(U) == 25
    assert r.members[0] == N and r.reached[0] == N - 25
    assert g.get_option("last_reach_ns") > 0 and g.get_option("last_analyzer_scratch_bytes") > 0
    dropped = g.stats()["dropped_proposals"]
    before, after = an.Repair()
    ex2 = g.export()
    print("repair", before, after, g.stats()["dropped_proposals"] - dropped)
    assert before == 25 and after == len(AR.reachability(ex2)["unreachable"])
    if g.stats()["dropped_proposals"] == dropped:  # the case test_analyzer_ref.py pins on the oracle
        assert after == 0
    assert np.array_equal(ex2["vecs"].view(np.uint32), crafted["vecs"].view(np.uint32))
    _check(H, g, 0)
    g.close()


# ---- relink against a twin ----
@pytest.mark.parametrize("metric", [0, 1])
def test_relink_equals_update_with_own_vectors(H, metric):
    a, _, X, _, keys = _batch_graph(H, metric)
    b = _batch_graph(H, metric)[0]
    dead = np.zeros(N, bool)
    dead[100:160:3] = True
    for g in (a, b):
        assert all(g.BatchDelete(keys[dead]))
        g.search_arrays(X[:8], 5, mode=H.MODE_EXACT)  # (the exact path's planes exist on both)
    ex0 = a.export()
    rows = np.array(sorted({0, N - 1, int(ex0["entry"][-1]), 100} | set(np.linspace(1, N - 2, 200).astype(int).tolist())))
    ukeys = np.concatenate([keys[rows], [1]])  # a deleted key among them, and a key never added
    fa = a.relink_arrays(ukeys)
    fb = b.update_arrays(ukeys, np.concatenate([X[rows], X[:1]]))
    assert np.array_equal(fa, fb) and not fa[-1] and fa.sum() == len(rows) - int(dead[rows].sum())
    for o in ("last_update_rows", "last_update_chunks", "last_update_repaired"):
        assert a.get_option(o) == b.get_option(o) > 0, o
    exa, exb = a.export(), b.export()
    BR.same_export(exa, exb, a.export_edge_dist(), b.export_edge_dist(), "relink")
    assert np.array_equal(exa["vecs"].view(np.uint32), ex0["vecs"].view(np.uint32))
    Q = X[::50] + np.float32(0.01)
    for mode in (H.MODE_BEAM, H.MODE_EXACT):
        ra, rb = a.search_arrays(Q, 10, mode=mode, ef=64), b.search_arrays(Q, 10, mode=mode, ef=64)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[2], rb[2])
        assert np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32))
    with pytest.raises(H.HnswError, match="duplicate key 7 in update"):
        a.relink_arrays(np.array([7, 10, 7]))
    assert a.Relink([int(keys[3]), 2]) == [True, False]
    a.close()
    b.close()


# ---- read-only behaviour ----
def test_calls_change_nothing(H):
    g, _, X, _, keys = _batch_graph(H, 0)
    assert all(g.BatchDelete(keys[10:40]))
    flt = g.Filter(keys[200:300].tolist())
    g.search_arrays(X[:4], 5, mode=H.MODE_BEAM, ef=32)
    ex0, ed0, st0, fc0 = g.export(), g.export_edge_dist(), g.stats(), flt.count()
    an = H.Analyzer(g)
    an.QualityMetrics(), an.Reachability(), an.Hops(keys[50:90]), an.DegreeHistogram(0), an.DegreeHistogram(1)
    BR.same_export(ex0, g.export(), ed0, g.export_edge_dist(), "read-only")
    assert g.stats() == st0 and flt.count() == fc0
    g.close()


def test_reachability_waits_for_enqueued_search(H):
    import torch

    g, _, X, _, keys = _batch_graph(H, 1)
    rng = np.random.default_rng(5)
    B, k = 4096, 10
    Q = torch.tensor(rng.normal(size=(B, D)).astype(np.float32), device="cuda")
    want = g.search_arrays(Q.cpu().numpy(), k, mode=H.MODE_BEAM, ef=64)
    ok = torch.empty(B, k, dtype=torch.int64, device="cuda")
    od = torch.empty(B, k, dtype=torch.float32, device="cuda")
    on = torch.empty(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g.search_device(Q.data_ptr(), B, D, k, ok.data_ptr(), od.data_ptr(), on.data_ptr(), mode=H.MODE_BEAM, ef=64,
                    stream=s.cuda_stream)
    r = H.Analyzer(g).Reachability()
    hp = H.Analyzer(g).Hops(keys[:16])
    torch.cuda.synchronize()
    g.device_status()
    assert np.array_equal(ok.cpu().numpy(), want[0]) and np.array_equal(on.cpu().numpy(), want[2])
    assert np.array_equal(od.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    ex = g.export()
    assert r.reached == AR.reachability(ex)["reached"] and np.array_equal(hp, AR.hops(ex, np.arange(16)))
    g.close()


# ---- string and float keys ----
@pytest.mark.parametrize("kind", ["str", "float"])
def test_other_key_types(H, kind):
    n = 40
    X = BR.clustered(np.random.default_rng(9), n, D)
    names = [f"k{i:03d}" for i in range(n)] if kind == "str" else [i + 0.5 for i in range(n)]
    # 35 rows in one batch onto 5: batch-mates do not see each other, so the new rows' in-edges
    # are the 5 x 4 slots of the old rows at most (one layer) -- at least 15 rows stay unreachable
    g = H.Graph(M=2, Ml=0.25, EfSearch=32, Distance=H.CosineDistance, Rng=2, build_mode=H.BUILD_BATCH, m0=4)
    g.BatchAdd([H.MakeNode(k, x) for k, x in zip(names[:5], X[:5])], levels=np.zeros(5, np.int32))
    g.set_option("batch_min", 64)
    g.BatchAdd([H.MakeNode(k, x) for k, x in zip(names[5:], X[5:])], levels=np.zeros(35, np.int32))
    ex = g.export()
    want = AR.reachability(ex)["unreachable"]
    assert len(want) >= 15
    an = H.Analyzer(g)
    assert an.Reachability().unreachable_keys == [names[i] for i in want]
    assert np.array_equal(an.Hops(names[:12]), AR.hops(ex, np.arange(12)))
    absent = "zzz" if kind == "str" else 1e9
    assert g.Relink([names[2], absent, names[1]]) == [True, False, True]
    ex = g.export()
    before, after = an.Repair()
    assert before == len(AR.reachability(ex)["unreachable"])
    assert after == len(AR.reachability(g.export())["unreachable"])
    g.close()
