"""GPU: compaction (mhnsw_compact / Graph.Compact / ExactIndex.Compact).  The deleted rows
leave the store in place; the export afterwards is tests/compact_ref.py's restatement of the
export before, and every search returns the keys, distance bits and counts it returned
before.  The delete pattern makes every chunk of the in-place move occur: an untouched live
prefix, single deleted rows (destination and source chunks overlap: the staged path), a
deleted block (the direct path), random deletions and a deleted tail."""
import numpy as np
import pytest

from tests import compact_ref as CR
from tests.test_gpu_parity import _same_graph

pytestmark = pytest.mark.gpu

SHAPES = [(3000, 24), (1531, 768)]
M, M0, EFC = 16, 32, 64


def _metric_fn(H, metric):
    return H.CosineDistance if metric == 0 else H.EuclideanDistance


def _pattern(n, rng):
    """rows 0-199 live; every 7th row of [200, 550) dead; a dead block [550, 850); 15 % of
    [850, n - 50) dead at random; the last 50 dead.  Rows 100 and 900 (one vector) stay."""
    dead = np.zeros(n, bool)
    dead[200:550:7] = True
    dead[550:850] = True
    dead[850:n - 50] = rng.random(n - 900) < 0.15
    dead[n - 50:] = True
    dead[900] = False
    return dead


def _make(H, n, d, metric, dead=None, **options):
    """-> (graph, X, keys, dead): a batch-mode graph with the pattern's rows deleted."""
    rng = np.random.default_rng(1000 * metric + d)
    X = rng.normal(size=(n, d)).astype(np.float32)
    if n > 900:
        X[900] = X[100]  # duplicates of one vector on both sides of the dead block
    keys = np.arange(n, dtype=np.int64) * 5 + 11
    if dead is None:
        dead = _pattern(n, rng)
    g = H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=7, build_mode=H.BUILD_BATCH, m0=M0,
                ef_construction=EFC, **options)
    g.add_arrays(keys, X)
    if dead.any():
        assert g.BatchDelete(keys[dead]) == [True] * int(dead.sum())
    return g, X, keys, dead


def _queries(X, d, seed=5, B=300):
    rng = np.random.default_rng(seed)
    Q = rng.normal(size=(B, d)).astype(np.float32)
    Q[0] = X[100]  # the duplicated vector: a tie broken by row id
    Q[1:9] = X[[3, 250, 560, 700, 901, 1200, 1500, 199]]  # stored rows, deleted ones among them
    return Q


def _oracle(O, ex, metric):
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=M, M0=M0, Ml=0.25, EfSearch=64)
    o.import_graph(**ex)
    return o


def _row_bytes(g, ex):
    pitch = g.get_option("pitch")
    layers = sum(4 + ((M0 if l == 0 else M) + 1) * 8 for l in range(ex["deg"].shape[0]))
    return pitch * 4 + pitch * 2 + 4 + 8 + 8 + 4 + layers  # f32, fp16, norm, fp16 aux, key, level, deg + adj + adjd


def _no_dangling(ex):
    dead = ex["dead"].astype(bool)
    for l in range(ex["deg"].shape[0]):
        for i in np.flatnonzero(~dead & (ex["deg"][l] > 0)):
            assert not dead[ex["adj"][l, i, : ex["deg"][l, i]]].any(), (l, i)


# ---------------------------------------------------------------- 1. the export is the remap
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n,d", SHAPES)
def test_export_is_the_remap(H, n, d, metric):
    g, X, keys, dead = _make(H, n, d, metric)
    nd = int(dead.sum())
    E0 = g.export()
    _no_dangling(E0)  # the batched repair leaves no live row pointing at a dead one
    want, dangling = CR.compact_export(E0)
    assert dangling == 0
    bytes0 = g.export_bytes()
    cap0, len0 = g.get_option("capacity"), g.Len()
    assert g.get_option("dead_rows") == nd and len0 == n - nd
    assert g.Compact() == nd
    assert g.Len() == len0 and g.get_option("dead_rows") == 0 and g.get_option("capacity") == cap0
    assert g.get_option("last_compact_dangling") == 0 and g.get_option("last_compact_ns") > 0
    E1 = g.export()
    CR.same_export(E1, want)
    assert g.export_bytes() == bytes0  # the Go format skips dead rows and writes neighbour keys ascending
    assert g.contains(keys).tolist() == (~dead).tolist()
    v, ok = g.Lookup(int(keys[900]))
    assert ok and np.array_equal(v, X[900])
    assert g.Compact() == 0  # nothing left: nothing written
    CR.same_export(g.export(), want)
    g.close()


# ---------------------------------------------------------------- 2. searches are identical
def _probe(H, g, Q, radii, negs):
    """Every search mode's lists, and the beam searches' counters [0] and [1]."""
    out, cnt = {}, {}

    def beam(name, q, k, ef):
        g.reset_stats()
        out[name] = g.search_arrays(q, k, mode=H.MODE_BEAM, ef=ef)
        st = g.stats()
        cnt[name] = (st["search_dist_evals"], st["search_expansions"])

    beam("beam k10 ef64", Q, 10, 64)
    beam("beam k64 ef64", Q, 64, 64)
    beam("beam ef768", Q[:40], 10, 768)
    beam("beam B1", Q[:1], 10, 64)
    g.set_option("search_expand", 4)
    beam("beam expand4", Q, 10, 64)
    g.set_option("search_expand", 1)
    out["exact k10"] = g.search_arrays(Q, 10, mode=H.MODE_EXACT)
    out["exact k256"] = g.search_arrays(Q[:50], 256, mode=H.MODE_EXACT)
    rng_ = {"range exact": g.range_search_arrays(Q[:60], radii, mode=H.MODE_EXACT),
            "range beam": g.range_search_arrays(Q[:60], radii, mode=H.MODE_BEAM, ef=64)}
    neg = {m: g.search_negatives_arrays(Q[:20], negs, 5, 0.5, mode=m, ef=64) for m in (H.MODE_BEAM, H.MODE_EXACT)}
    return out, cnt, rng_, neg


@pytest.mark.parametrize("screen", [1, 0])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n,d", SHAPES)
def test_searches_identical(H, O, n, d, metric, screen):
    g, X, keys, dead = _make(H, n, d, metric, screen=screen)
    Q = _queries(X, d)
    # radii at a boundary distance: exactly the 5th neighbour's (inclusive), and just below the 3rd's
    _, xd, _ = g.search_arrays(Q[:60], 5, mode=H.MODE_EXACT)
    radii = xd[:, 4].copy()
    radii[1::2] = np.nextafter(xd[1::2, 2], np.float32(-np.inf))
    rng = np.random.default_rng(3)
    negs = [rng.normal(size=(b % 4, d)).astype(np.float32) for b in range(20)]
    out0, cnt0, rng0, neg0 = _probe(H, g, Q, radii, negs)
    assert g.Compact() == int(dead.sum())
    out1, cnt1, rng1, neg1 = _probe(H, g, Q, radii, negs)
    for name in out0:
        CR.same_lists(out0[name], out1[name])
        assert out1[name][2].max() > 0, name
    assert cnt0 == cnt1
    for name in rng0:
        l0, k0, d0 = rng0[name]
        l1, k1, d1 = rng1[name]
        assert np.array_equal(l0, l1) and np.array_equal(k0, k1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32)), name
    assert (np.diff(rng1["range exact"][0]) >= 2).all()  # the boundary row is a hit: the radius is inclusive
    for m in neg0:
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(neg0[m], neg1[m])), m
    # and the oracle on the compacted export, where it has the mode
    o = _oracle(O, g.export(), metric)
    CR.same_lists(out1["beam k10 ef64"], o.search(Q, 10, mode=O.MODE_BEAM, ef=64))
    CR.same_lists(out1["beam k64 ef64"], o.search(Q, 64, mode=O.MODE_BEAM, ef=64))
    CR.same_lists(out1["beam ef768"], o.search(Q[:40], 10, mode=O.MODE_BEAM, ef=768))
    CR.same_lists(out1["beam B1"], o.search(Q[:1], 10, mode=O.MODE_BEAM, ef=64))
    CR.same_lists(out1["exact k10"], o.search(Q, 10, mode=O.MODE_EXACT))
    CR.same_lists(out1["exact k256"], o.search(Q[:50], 256, mode=O.MODE_EXACT))
    o.set_search_expand(4)
    CR.same_lists(out1["beam expand4"], o.search(Q, 10, mode=O.MODE_BEAM, ef=64))
    g.close()


# ---------------------------------------------------------------- 3. chunking
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n,d", SHAPES)
def test_stage_sizes_give_one_result(H, n, d, metric):
    want = None
    # 64: staged chunks through the single deleted rows, direct ones from the block on; 400:
    # a staged chunk that straddles the block; 1: no stage, every chunk as long as the rows deleted
    # below it; the default and >= N: one staged chunk
    for stage in (64, 400, 1, None, 10 * n):
        g, X, keys, dead = _make(H, n, d, metric)
        if want is None:
            want, _ = CR.compact_export(g.export())
        default = g.get_option("compact_stage_rows")
        assert default >= 1
        if stage is not None:
            g.set_option("compact_stage_rows", stage)
            assert g.get_option("compact_stage_rows") == stage
        assert g.Compact() == int(dead.sum())
        E1 = g.export()
        CR.same_export(E1, want)
        if stage == 64:
            assert 0 < g.get_option("last_compact_scratch_bytes") <= 8 * n + 64 * _row_bytes(g, E1)
        g.close()
    g = H.Graph(build_mode=H.BUILD_BATCH)
    with pytest.raises(H.HnswError, match="compact_stage_rows must be >= 1"):
        g.set_option("compact_stage_rows", 0)
    g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_edge_cases(H, O, metric):
    n, d = 700, 24
    Qs = np.random.default_rng(9).normal(size=(5, d)).astype(np.float32)
    # everything dead but one row
    dead = np.ones(n, bool)
    dead[333] = False
    g, X, keys, _ = _make(H, n, d, metric, dead=dead)
    want, _ = CR.compact_export(g.export())
    assert g.Compact() == n - 1 and g.Len() == 1
    CR.same_export(g.export(), want)
    for mode in (H.MODE_BEAM, H.MODE_EXACT):
        ok, _, on = g.search_arrays(Qs, 3, mode=mode, ef=16)
        assert on.tolist() == [1] * 5 and (ok[:, 0] == keys[333]).all()
    g.close()
    # everything dead: an empty store that takes rows again
    g, X, keys, _ = _make(H, n, d, metric, dead=np.ones(n, bool))
    assert g.Compact() == n and g.Len() == 0 and g.get_option("dead_rows") == 0
    assert len(g.export()["keys"]) == 0
    for mode in (H.MODE_BEAM, H.MODE_EXACT):
        assert g.search_arrays(Qs, 3, mode=mode, ef=16)[2].tolist() == [0] * 5
    g.add_arrays(keys[:300], X[:300])  # the deleted keys come back
    assert g.Len() == 300
    o = _oracle(O, g.export(), metric)
    for mode, om in ((H.MODE_BEAM, O.MODE_BEAM), (H.MODE_EXACT, O.MODE_EXACT)):
        CR.same_lists(g.search_arrays(Qs, 3, mode=mode, ef=32), o.search(Qs, 3, mode=om, ef=32))
    g.close()
    # nothing dead: returns 0, the export is identical
    g, X, keys, _ = _make(H, n, d, metric, dead=np.zeros(n, bool))
    E0 = g.export()
    assert g.Compact() == 0
    CR.same_export(g.export(), E0)
    g.close()


# ---------------------------------------------------------------- 4. filters
@pytest.mark.parametrize("metric", [0, 1])
def test_filters_follow_the_rows(H, metric):
    n, d = SHAPES[0]
    rng = np.random.default_rng(21 + metric)
    g, X, keys, _ = _make(H, n, d, metric, dead=np.zeros(n, bool))
    dead = _pattern(n, rng)
    fa = g.Filter(keys[::3])  # made before the delete: it names keys that are deleted
    assert g.BatchDelete(keys[dead]) == [True] * int(dead.sum())
    fb = g.Filter(keys[rng.random(n) < 0.3])
    ca, cb = fa.count(), fb.count()
    assert ca == int((~dead)[::3].sum()) and cb > 0
    Q = _queries(X, d, B=60)
    per_query = [(fa, fb, None)[b % 3] for b in range(len(Q))]

    def probe():
        return [g.search_filtered_arrays(Q, 10, flt, ef=64, mode=mode)
                for mode in (H.MODE_BEAM, H.MODE_EXACT) for flt in (fa, fb, per_query)]

    before = probe()
    assert g.Compact() == int(dead.sum())
    assert fa.count() == ca and fb.count() == cb
    for a, b in zip(before, probe()):
        CR.same_lists(a, b)
        assert b[2].max() > 0
    # 400 new rows land in the freed slots, each one the nearest row of a query: no filtered
    # search returns them until a filter's update names their keys
    new_keys = np.arange(400, dtype=np.int64) + 10 ** 6
    Q2 = Q[9:]  # (the queries that are no stored row: a copy of one is its single nearest row)
    XN = np.tile(Q2, (8, 1))[:400]
    g.add_arrays(new_keys, XN)
    assert g.get_option("capacity") >= g.Len() and len(g.export()["keys"]) == n - int(dead.sum()) + 400
    assert fa.count() == ca and fb.count() == cb
    for a, b in zip(before[:2] + before[3:5], [g.search_filtered_arrays(Q, 10, flt, ef=64, mode=mode)
                                                for mode in (H.MODE_BEAM, H.MODE_EXACT) for flt in (fa, fb)]):
        assert not np.isin(b[0], new_keys).any()
        CR.same_lists(a, b)
    fa.add(new_keys[:len(Q2)])
    assert fa.count() == ca + len(Q2)
    for mode in (H.MODE_BEAM, H.MODE_EXACT):
        ok, _, on = g.search_filtered_arrays(Q2, 1, fa, ef=64, mode=mode)
        assert on.tolist() == [1] * len(Q2) and ok[:, 0].tolist() == new_keys[:len(Q2)].tolist()
        ok, _, _ = g.search_filtered_arrays(Q, 10, fb, ef=64, mode=mode)
        assert not np.isin(ok, new_keys).any()
    g.close()


def test_facets_keep_their_filters(H):
    from hnsw_amd import facets as F
    rng = np.random.default_rng(4)
    n, d = 600, 24
    X = rng.normal(size=(n, d)).astype(np.float32)
    g = H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=7, build_mode=H.BUILD_BATCH, m0=M0,
                ef_construction=EFC)
    fg = F.FacetedGraph(g, F.MemoryFacetStore())
    fg.BatchAdd([F.NewFacetedNode(H.MakeNode(i, X[i]), [F.BasicFacet("category", "abc"[i % 3])]) for i in range(n)])
    fg.BatchDelete(list(range(50, 400, 2)))
    flt = [F.EqualityFilter("category", "b")]
    before = [[x.Node.Key for x in fg.Search(X[i], flt, 5, mode=mode, ef=64)] for mode in (H.MODE_BEAM, H.MODE_EXACT)
              for i in (1, 51, 599)]
    cached = [f for _, f in fg._filters.values()]
    assert len(cached) == 1 and g.Compact() == 175
    after = [[x.Node.Key for x in fg.Search(X[i], flt, 5, mode=mode, ef=64)] for mode in (H.MODE_BEAM, H.MODE_EXACT)
             for i in (1, 51, 599)]
    assert before == after and all(len(r) == 5 and all(k % 3 == 1 for k in r) for r in after)
    assert [f for _, f in fg._filters.values()][0] is cached[0] and cached[0].id is not None
    fg.close()
    g.close()


# ---------------------------------------------------------------- 5. life goes on
@pytest.mark.parametrize("metric", [0, 1])
def test_life_goes_on(H, O, metric):
    n, d = SHAPES[0]
    g, X, keys, dead = _make(H, n, d, metric)
    Q = _queries(X, d, B=100)
    rng = np.random.default_rng(77 + metric)

    def check():
        ex = g.export()
        o = _oracle(O, ex, metric)
        CR.same_lists(g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=64), o.search(Q, 10, mode=O.MODE_BEAM, ef=64))
        CR.same_lists(g.search_arrays(Q, 10, mode=H.MODE_EXACT), o.search(Q, 10, mode=O.MODE_EXACT))
        return ex, o

    assert g.Compact() == int(dead.sum())
    check()
    # 500 rows, 100 of them deleted keys coming back with new vectors
    back = keys[np.flatnonzero(dead)[:100]]
    add_keys = np.concatenate([back, np.arange(400, dtype=np.int64) + 10 ** 6])
    XA = rng.normal(size=(500, d)).astype(np.float32)
    g.add_arrays(add_keys, XA)
    assert g.Len() == n - int(dead.sum()) + 500 and g.get_option("dead_rows") == 0
    ok, od, on = g.search_arrays(XA[:100], 1, mode=H.MODE_EXACT)
    assert ok[:, 0].tolist() == back.tolist()
    ex, o = check()
    # the engine's delete after a compaction == the oracle's repair of the same graph
    live_keys = ex["keys"]
    top = ex["deg"].shape[0] - 1
    gone = [int(live_keys[ex["entry"][top]])] + [int(x) for x in rng.permutation(live_keys)[: len(live_keys) // 10]]
    gone = list(dict.fromkeys(gone))
    assert g.BatchDelete(gone) == o.delete(gone, mode=1) == [True] * len(gone)
    ex = g.export()
    _same_graph(ex, o.export())
    _no_dangling(ex)
    check()
    want, dangling = CR.compact_export(ex)
    assert dangling == 0 and g.Compact() == len(gone)
    CR.same_export(g.export(), want)
    check()
    g.close()


# ---------------------------------------------------------------- 6. flat handles
@pytest.mark.parametrize("metric", [0, 1])
def test_exact_index(H, metric):
    rng = np.random.default_rng(31 + metric)
    n, d = 1200, 24
    X = rng.normal(size=(n, d)).astype(np.float32)
    keys = list(range(0, 3 * n, 3))
    x = H.ExactIndex(_metric_fn(H, metric))
    x.BatchAdd(keys, X)
    gone = [keys[i] for i in rng.permutation(n)[:300]] + keys[-20:]
    gone = list(dict.fromkeys(gone))
    assert x.BatchDelete(gone) == [True] * len(gone)
    Q = np.concatenate([rng.normal(size=(30, d)).astype(np.float32), X[:10]])
    fl = x.Filter(keys[::2])
    before, fbefore = x.search_batch(Q, 10), x.search_filtered_batch(Q, 10, fl)
    rbefore = x.range_search_batch(Q, before[1][:, 3])
    assert x.Compact() == len(gone) and x.Len() == n - len(gone) and x.Compact() == 0
    after, fafter = x.search_batch(Q, 10), x.search_filtered_batch(Q, 10, fl)
    rafter = x.range_search_batch(Q, before[1][:, 3])
    for a, b in ((before, after), (fbefore, fafter)):
        assert a[0] == b[0] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    assert np.array_equal(rbefore[0], rafter[0]) and rbefore[1] == rafter[1]
    # Replace (a present key) and Add (a deleted key, a new key) work afterwards
    live = [k for k in keys if k not in set(gone)]
    v = rng.normal(size=(3, d)).astype(np.float32)
    x.BatchAdd([live[5], gone[0], 10 ** 6], v)
    assert x.Len() == n - len(gone) + 2
    for key, q in zip([live[5], gone[0], 10 ** 6], v):
        assert x.Search(q, 1)[0].Key == key
    x.Close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(H):
    rng = np.random.default_rng(2)
    X = rng.normal(size=(200, 16)).astype(np.float32)
    g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=H.CosineDistance)  # compat mode
    g.add_arrays(np.arange(200), X)
    g.BatchDelete(list(range(0, 200, 4)))
    E0 = g.export()
    with pytest.raises(H.HnswError, match=r"compact needs a batch or flat \(build_mode 1 or 2\) handle") as e:
        g.Compact()
    assert e.value.code == H._lib.EUNSUPPORTED
    E1 = g.export()
    CR.same_export(E1, E0)
    assert np.array_equal(E1["adj"], E0["adj"])
    g.close()
    # out_removed == NULL is accepted
    g, _, _, dead = _make(H, 700, 24, 0, dead=np.arange(700) % 5 == 2)
    assert H.load().mhnsw_compact(g._h, None) == 0
    assert g.get_option("dead_rows") == 0 and len(g.export()["keys"]) == 700 - int(dead.sum())
    g.close()


# ---------------------------------------------------------------- 8. ordering
def test_enqueued_search_is_not_overtaken(H):
    import torch
    n, d = SHAPES[0]
    g, X, keys, dead = _make(H, n, d, 0)
    B, k = 4096, 10
    Q = torch.from_numpy(np.random.default_rng(8).normal(size=(B, d)).astype(np.float32)).cuda()
    outs = []
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for step in range(2):
        ok = torch.zeros((B, k), dtype=torch.int64, device="cuda")
        od = torch.zeros((B, k), dtype=torch.float32, device="cuda")
        on = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g.search_device(Q.data_ptr(), B, d, k, ok.data_ptr(), od.data_ptr(), on.data_ptr(), mode=H.MODE_BEAM, ef=64,
                        stream=s.cuda_stream)
        if step == 0:
            assert g.Compact() == int(dead.sum())  # the search above is still on its stream
        outs.append((ok, od, on))
    torch.cuda.synchronize()
    g.device_status()
    a, b = [[t.cpu().numpy() for t in o] for o in outs]
    CR.same_lists(a, b)
    assert (a[2] == k).all()
    CR.same_lists(a, g.search_arrays(Q.cpu().numpy(), k, mode=H.MODE_BEAM, ef=64))
    g.close()


# ---------------------------------------------------------------- 9. string keys
def test_string_keys(H):
    rng = np.random.default_rng(12)
    n, d = 500, 24
    X = rng.normal(size=(n, d)).astype(np.float32)
    names = ["k%03d-%s" % (i, "xyz"[i % 3]) for i in rng.permutation(n)]
    g = H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=7, build_mode=H.BUILD_BATCH, m0=M0,
                ef_construction=EFC)
    g.BatchAdd([H.MakeNode(names[i], X[i]) for i in range(n)])
    gone = names[40:400:3]
    assert g.BatchDelete(gone) == [True] * len(gone)
    Q = X[[0, 41, 200, 499]]
    before = [[x.Key for x in g.Search(q, 8, mode=mode)] for mode in (H.MODE_BEAM, H.MODE_EXACT) for q in Q]
    labels = g.get_option("strkeys")
    assert g.Compact() == len(gone)
    after = [[x.Key for x in g.Search(q, 8, mode=mode)] for mode in (H.MODE_BEAM, H.MODE_EXACT) for q in Q]
    assert before == after and all(len(r) == 8 and not set(r) & set(gone) for r in after)
    assert g.get_option("strkeys") == labels  # keys do not change: the labels stay
    assert g.decode_keys(g.export()["keys"]) == [s for s in names if s not in set(gone)]
    g.Add(H.MakeNode(gone[0], X[40]))  # a deleted string comes back into a freed row
    assert g.Search(X[40], 1, mode=H.MODE_EXACT)[0].Key == gone[0]
    g.close()
