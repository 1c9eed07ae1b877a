"""The batched insert's link pass (option batch_link): after a layer's commit
every row of the batch searches the layer again and takes the batch-mates it
finds into its neighbour selection.  These are properties of the exported
graph, oracle replay of the searches on it, comparisons with the unlinked build
of the same rows, and (test_link_structure_and_replay) the whole export against
the oracle's restatement of the batched build and the link pass, bit for bit."""
import numpy as np
import pytest

from tests import batch_ref as BR
from tests.test_gpu_parity import _metric_fn, _same_results

pytestmark = pytest.mark.gpu


def _clustered(rng, n, d, nc=64, intrinsic=12, noise=0.05):
    C = rng.normal(size=(nc, intrinsic)).astype(np.float32)
    A = rng.normal(size=(intrinsic, d)).astype(np.float32) / np.sqrt(intrinsic)
    z = C[rng.integers(0, nc, n)] + 0.35 * rng.normal(size=(n, intrinsic)).astype(np.float32)
    x = z @ A + noise * rng.normal(size=(n, d)).astype(np.float32)
    return x.astype(np.float32)


def _same_export(a, b):
    for f in ("keys", "vecs", "deg", "adj", "entry", "dead"):
        assert np.array_equal(a[f], b[f]), f


SHAPE = dict(n0=3000, nb=600, d=48, M=12, m0=24, efc=64)


def _data(seed, n0, nb, d):
    rng = np.random.default_rng(seed)
    X = _clustered(rng, n0 + nb, d)
    rng.shuffle(X)  # base and batch rows share the clusters
    return X, _clustered(rng, 200, d)


def _build(H, X, metric, link, n0, nb, d, M, m0, efc, link_ef=0, **opts):
    """Base of n0 rows (link off), then nb rows in exactly one batch with batch_link = link
    (None: never set).  Returns the handle and the export of the base."""
    g = H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=5, build_mode=H.BUILD_BATCH, m0=m0,
                ef_construction=efc, heuristic=2, keep_pruned=1, **opts)
    lv0 = g.preview_levels(n0)
    g.add_arrays(np.arange(n0), X[:n0], levels=lv0)
    base = g.export()
    top = base["deg"].shape[0] - 1
    if link is not None:
        g.set_option("batch_link", link)
        g.set_option("batch_link_ef", link_ef)
    g.set_option("batch_ratio_pct", 0)
    g.set_option("batch_max", nb)
    g.set_option("batch_min", nb)
    lv1 = np.minimum(g.preview_levels(nb), top).astype(np.int32)
    g.add_arrays(np.arange(n0, n0 + nb), X[n0:n0 + nb], levels=lv1)
    return g, base


def _pair(H, X, metric, **kw):
    ga, base_a = _build(H, X, metric, 0, **kw)
    gb, base_b = _build(H, X, metric, 1, **kw)
    _same_export(base_a, base_b)
    return ga, gb


def _batch_edges(ex, n0):
    """(layer, row, neighbour) of every edge from a batch row to a batch row"""
    out = []
    L, N = ex["deg"].shape
    for l in range(L):
        for i in range(n0, N):
            dg = ex["deg"][l, i]
            if dg > 0:
                out += [(l, i, int(c)) for c in ex["adj"][l, i, :dg] if c >= n0]
    return out


def _check_linked(gb, exa, exb, n0, caps):
    """1(b)-(e) on the linked export exb, exa the unlinked build of the same rows"""
    L, N = exb["deg"].shape
    edges = _batch_edges(exb, n0)
    assert len(edges) > 0                                             # (b)
    assert gb.get_option("last_link_edges") > 0
    # (a row counts once per layer the pass changed it in)
    assert 0 < gb.get_option("last_link_rows") <= int((exb["deg"][:, n0:] >= 0).sum())
    dead = exb["dead"].astype(bool)
    for l in range(L):
        for i in range(N):
            dg = exb["deg"][l, i]
            assert dg <= caps[l], (l, i, dg)                          # (d)
            if dg <= 0:
                continue
            row = exb["adj"][l, i, :dg]
            assert row.min() >= 0 and row.max() < N, (l, i)
            assert i not in row and len(set(row.tolist())) == dg, (l, i)
            assert not dead[row].any(), (l, i)
            if i >= n0:                                               # (c)
                new = set(row.tolist()) - set(exa["adj"][l, i, : max(exa["deg"][l, i], 0)].tolist())
                assert all(c >= n0 for c in new), (l, i, new)
            else:  # the pass proposes to batch-mates only: the old rows are the unlinked build's
                assert np.array_equal(exb["adj"][l, i], exa["adj"][l, i]), (l, i)
    for l, i, c in edges:                                             # (e)
        assert exb["deg"][l, i] >= 0 and exb["deg"][l, c] >= 0, (l, i, c)
    assert np.array_equal(exa["deg"] >= 0, exb["deg"] >= 0)


def _check_replay(H, O, gb, exb, Q, metric, M, m0):
    """2: the oracle's searches on the exported graph == the engine's on the device's"""
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=M, M0=m0, Ml=0.25, EfSearch=64)
    o.import_graph(**exb)
    _same_results(*gb.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=64), *o.search(Q, 10, mode=O.MODE_BEAM, ef=64))
    _same_results(*gb.search_arrays(Q, 10, mode=H.MODE_EXACT), *o.search(Q, 10, mode=O.MODE_EXACT))


@pytest.mark.parametrize("metric", [0, 1])
def test_link_structure_and_replay(H, O, metric):
    """1 and 2 at the base shape: the unlinked batch holds no batch -> batch edge, the
    linked one does, and everything the pass changed in a batch row is a batch-mate."""
    X, Q = _data(21 + metric, SHAPE["n0"], SHAPE["nb"], SHAPE["d"])
    ga, gb = _pair(H, X, metric, **SHAPE)
    exa, exb = ga.export(), gb.export()
    assert _batch_edges(exa, SHAPE["n0"]) == []                       # (a)
    assert ga.get_option("last_link_edges") == 0 and ga.get_option("last_link_rows") == 0
    _check_linked(gb, exa, exb, SHAPE["n0"], [SHAPE["m0"]] + [SHAPE["M"]] * 31)
    _check_replay(H, O, gb, exb, Q, metric, SHAPE["M"], SHAPE["m0"])
    assert gb.get_option("last_link_ns") == 0  # (time_build is off)
    # the restatement (og_add_batch) given the same rows, levels and options builds both graphs:
    # every field, adj in stored order, and the bits of every stored edge distance
    n0, nb = SHAPE["n0"], SHAPE["nb"]
    opts = dict(ef_construction=SHAPE["efc"], heuristic=2, keep_pruned=1)
    for g, ex, link in ((ga, exa, 0), (gb, exb, 1)):
        assert g.stats()["dropped_proposals"] == 0
        lv = BR.levels_of(ex)
        o = O.Graph(metric=metric, order=O.ORDER_DEV, M=SHAPE["M"], M0=SHAPE["m0"], Ml=0.25, EfSearch=64)
        cn = o.add_batch(np.arange(n0), X[:n0], lv[:n0], **opts)
        cl = o.add_batch(np.arange(n0, n0 + nb), X[n0:n0 + nb], lv[n0:], batch_link=link, batch_ratio_pct=0,
                         batch_max=nb, batch_min=nb, **opts)
        assert cn["dropped_proposals"] == 0 and cl["dropped_proposals"] == 0
        assert cl["link_rows"] == g.get_option("last_link_rows") and cl["link_edges"] == g.get_option("last_link_edges")
        BR.same_export(ex, o.export(), g.export_edge_dist(), o.export_edge_dist(), what=("link", link))
    ga.close()
    gb.close()


def test_link_deterministic(H):
    """3: the same build twice gives the same export, and no proposal was dropped"""
    X, _ = _data(23, SHAPE["n0"], SHAPE["nb"], SHAPE["d"])
    exs = []
    for _ in range(2):
        g, _ = _build(H, X, 0, 1, **SHAPE)
        assert g.stats()["dropped_proposals"] == 0
        exs.append(g.export())
        g.close()
    _same_export(*exs)


TIERS = [
    # efC 128: the two-register list; efC 256: four registers, the merge path
    dict(efc=128, build_expand=1), dict(efc=128, build_expand=2), dict(efc=128, build_expand=4),
    dict(efc=256, build_expand=1), dict(efc=256, build_expand=2), dict(efc=256, build_expand=4),
    dict(m0=63),                                  # the degree cap
    dict(metric=1, d=768, n0=1500, nb=300),       # three float4 a lane
    dict(efc=128, link_ef=32),                    # the narrow width
]


@pytest.mark.parametrize("case", TIERS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_link_tiers(H, O, case):
    """4: 1(b)-(e) and 2 at every list tier and expansion width of the link search"""
    kw = dict(SHAPE)
    kw.update(case)
    metric = kw.pop("metric", 0)
    X, Q = _data(31, kw["n0"], kw["nb"], kw["d"])
    ga, gb = _pair(H, X, metric, **kw)
    exa, exb = ga.export(), gb.export()
    if "link_ef" in case:
        assert gb.get_option("batch_link_ef") == 32
    _check_linked(gb, exa, exb, kw["n0"], [kw["m0"]] + [kw["M"]] * 31)
    _check_replay(H, O, gb, exb, Q, metric, kw["M"], kw["m0"])
    ga.close()
    gb.close()


@pytest.mark.parametrize("opt", ["screen", "fuse_descent"])
def test_link_same_graph_either_way(H, O, opt):
    """4: the screening copy and the fused descent change how the link pass runs, not what it
    builds; 1(b)-(e) and 2 on that graph, built with the option off"""
    X, Q = _data(33, SHAPE["n0"], SHAPE["nb"], SHAPE["d"])
    exs, gs = [], []
    for v in (0, 1):
        g, _ = _build(H, X, 0, 1, **SHAPE, **{opt: v})
        assert g.get_option("last_link_edges") > 0
        exs.append(g.export())
        gs.append(g)
    _same_export(*exs)
    ga, _ = _build(H, X, 0, 0, **SHAPE, **{opt: 0})
    _check_linked(gs[0], ga.export(), exs[0], SHAPE["n0"], [SHAPE["m0"]] + [SHAPE["M"]] * 31)
    _check_replay(H, O, gs[0], exs[0], Q, 0, SHAPE["M"], SHAPE["m0"])
    for g in gs + [ga]:
        g.close()


def test_link_time_and_counters(H):
    """With time_build the link kernels' device time is reported alone (last_link_ns) and is
    part of the build kernel time; the pass's work is added to the build counters."""
    X, _ = _data(39, SHAPE["n0"], SHAPE["nb"], SHAPE["d"])
    st = []
    for link in (0, 1):
        g, _ = _build(H, X, 0, link, **SHAPE, time_build=1)
        st.append((g.stats(), g.get_option("last_link_ns")))
        g.close()
    (s0, ns0), (s1, ns1) = st
    assert ns0 == 0 and ns1 > 0
    assert s1["build_search_us"] * 1000 >= ns1
    for f in ("build_dist_evals", "build_expansions", "build_f32_rows"):
        assert s1[f] > s0[f], f


def test_link_off_is_off(H):
    """5: batch_link 0 is the build without the option; 2 is refused; compat and flat builds ignore it"""
    X, _ = _data(35, SHAPE["n0"], SHAPE["nb"], SHAPE["d"])
    g0, _ = _build(H, X, 0, None, **SHAPE)
    g1, _ = _build(H, X, 0, 0, **SHAPE)
    assert g0.get_option("batch_link") == 0 and g0.get_option("batch_link_ef") == 0
    _same_export(g0.export(), g1.export())
    with pytest.raises(H.HnswError, match="batch_link must be 0 or 1") as e:
        g1.set_option("batch_link", 2)
    assert e.value.code == -1  # MHNSW_EINVAL
    assert g1.get_option("batch_link") == 0
    g1.set_option("batch_link_ef", 7)      # stored as given: the clamp to [row cap, 512] is applied per layer, at use
    assert g1.get_option("batch_link_ef") == 7
    g0.close()
    g1.close()
    for mode in (H.BUILD_COMPAT, H.BUILD_FLAT):
        exs = []
        for link in (0, 1):
            g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=H.CosineDistance, Rng=5, build_mode=mode,
                        batch_link=link)
            g.add_arrays(np.arange(400), X[:400])
            assert g.get_option("last_link_rows") == 0
            exs.append(g.export())
            g.close()
        _same_export(*exs)


def _self_share(H, X, n0, link=0, **opts):
    """X[:n0] built at the defaults, X[n0:] added with the options; the share of X[n0:] that
    finds its own key (k 1, ef 64)"""
    g = H.Graph(M=12, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=5, build_mode=H.BUILD_BATCH, m0=24,
                ef_construction=64)
    g.add_arrays(np.arange(n0), X[:n0])
    g.set_option("batch_link", link)
    for k, v in opts.items():
        g.set_option(k, v)
    g.add_arrays(np.arange(n0, len(X)), X[n0:])
    k, _, n = g.search_arrays(X[n0:], 1, mode=H.MODE_BEAM, ef=64)
    g.close()
    return float(np.mean((n > 0) & (k[:, 0] == np.arange(n0, len(X)))))


def test_link_documented_case(H):
    """6: 1,000 rows added to 5,100 in one 20 % batch.  The share of the new rows that find
    their own key at ef 64: U unlinked, L linked, S one row a batch (the sequential
    reference).  The margin is 10 rows of 1,000: three standard deviations of a binomial
    share near 0.99 over 1,000 trials.  As in the case the option's documentation quotes
    (test_batch_delete_repair_parity's Adds after its deletions), the new rows are a second
    draw of the generator: new documents in clusters of their own, whose neighbours are
    mostly each other."""
    rng = np.random.default_rng(61)
    X = np.concatenate([_clustered(rng, 5100, 48), _clustered(rng, 1000, 48)])
    U = _self_share(H, X, 5100, 0, batch_ratio_pct=20)
    L = _self_share(H, X, 5100, 1, batch_ratio_pct=20)
    S = _self_share(H, X, 5100, 0, batch_max=1)
    print(f"batch_link documented case: U={U:.4f} L={L:.4f} S={S:.4f}")
    assert L >= S - 0.01, (U, L, S)
    assert L > U, (U, L, S)


def test_link_then_delete_and_compact(H):
    """7: deletions and compaction on a linked graph: deleted keys never return, and the
    searches before and after Compact give the same keys and distance bits"""
    n0, nb = SHAPE["n0"], SHAPE["nb"]
    X, Q = _data(37, n0, nb, SHAPE["d"])
    g, _ = _build(H, X, 0, 1, **SHAPE)
    assert g.get_option("last_link_edges") > 0
    rng = np.random.default_rng(38)
    gone = [int(x) for x in rng.permutation(n0)[:150]] + [int(x) for x in n0 + rng.permutation(nb)[:150]]
    assert g.BatchDelete(gone) == [True] * 300
    before = g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=64)
    assert g.Compact() == 300
    after = g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=64)
    _same_results(*before, *after)
    for b in range(len(Q)):
        assert not set(after[0][b, : after[2][b]].tolist()) & set(gone)
    ex = g.export()
    assert not ex["dead"].any() and len(ex["keys"]) == n0 + nb - 300
    g.close()
