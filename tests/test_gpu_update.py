"""GPU: the in-place update (mhnsw_update / Graph.update_arrays / Graph.Update): stored rows
take new vectors, keep their ids, levels, layer membership and filter bits, and the graph
around them is relinked on the device.  These are properties of the export, oracle replay of the searches on
it, comparisons with the route the call replaces (Delete + Add), and (_check_update) the whole
export against the oracle's restatement of the build and the update, bit for bit."""
import numpy as np
import pytest

from tests import batch_ref as BR
from tests import compact_ref as CR
from tests.test_gpu_parity import _metric_fn

pytestmark = pytest.mark.gpu

SHAPE = dict(n=3000, d=48, M=12, m0=24, efc=64)
WIDE = dict(n=1531, d=768, M=12, m0=24, efc=64)
NC, INTRINSIC = 64, 12


class Gen:
    """The clustered generator of test_gpu_batch_link.py with the labels kept: a row's new
    vector can be drawn from another cluster than its own."""

    def __init__(self, seed, d):
        self.rng = np.random.default_rng(seed)
        self.d = d
        self.C = self.rng.normal(size=(NC, INTRINSIC)).astype(np.float32)
        self.A = self.rng.normal(size=(INTRINSIC, d)).astype(np.float32) / np.sqrt(INTRINSIC)

    def draw(self, labels):
        n = len(labels)
        z = self.C[labels] + 0.35 * self.rng.normal(size=(n, INTRINSIC)).astype(np.float32)
        return (z @ self.A + 0.05 * self.rng.normal(size=(n, self.d)).astype(np.float32)).astype(np.float32)

    def rows(self, n):
        labels = self.rng.integers(0, NC, n)
        return self.draw(labels), labels

    def moved(self, labels):
        """one draw per label, each from another cluster"""
        return self.draw((labels + self.rng.integers(1, NC, len(labels))) % NC)


def _graph(H, metric, n, d, M, m0, efc, **opts):
    return H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=5, build_mode=H.BUILD_BATCH, m0=m0,
                   ef_construction=efc, heuristic=2, keep_pruned=1, **opts)


def _keys(n):
    return np.arange(n, dtype=np.int64) * 3 + 7


def _levels(ex):
    """each row's level: its highest layer"""
    member = ex["deg"] != -2
    return (member.shape[0] - 1 - np.argmax(member[::-1], axis=0)).astype(np.int32)


def _update_rows(ex, dead_rows, want):
    """`want` rows spread over the id range: row 0 and the last, a row of every upper layer, the
    top layer's entry; no deleted row"""
    L, N = ex["deg"].shape
    rows = {0, N - 1, int(ex["entry"][L - 1])}
    for l in range(1, L):
        rows.add(int(np.flatnonzero((ex["deg"][l] >= 0) & (ex["dead"] == 0))[-1]))
    for r in np.linspace(1, N - 2, want).astype(int):
        if len(rows) >= want:
            break
        rows.add(int(r))
    rows -= set(int(r) for r in dead_rows)
    return np.array(sorted(rows))


def _invariants(ex, caps):
    """contract item 6, the structure: per layer deg <= cap - 1 (the row cap), set-valued rows,
    no self-loop, no edge to a deleted, absent or foreign row -- over every row, deleted ones
    included (their edges are shown by the export and must not name an absent row either)"""
    L, N = ex["deg"].shape
    dead = ex["dead"].astype(bool)
    for l in range(L):
        member = ex["deg"][l] >= 0
        for i in np.flatnonzero(ex["deg"][l] > 0):
            dg = ex["deg"][l, i]
            assert dg <= caps[l], (l, i, dg)
            row = ex["adj"][l, i, :dg]
            assert row.min() >= 0 and row.max() < N, (l, i)
            assert i not in row and len(set(row.tolist())) == dg, (l, i)
            assert member[row].all(), (l, i)
            if not dead[i]:
                assert not dead[row].any(), (l, i)


def _edge_violations(H, metric, ex, adjd):
    """(layer, row, slot) of every stored edge distance that is not, bit for bit, mhnsw_distance
    of the two current vectors; slots past the degree must hold 0"""
    fn = _metric_fn(H, metric)
    bad = set()
    L, N = ex["deg"].shape
    for l in range(L):
        for i in np.flatnonzero(ex["deg"][l] > 0):
            dg = ex["deg"][l, i]
            want = fn.sweep(ex["vecs"][i], ex["vecs"][ex["adj"][l, i, :dg]])
            got = adjd[l, i, :dg]
            for j in np.flatnonzero(want.view(np.uint32) != got.view(np.uint32)):
                if not (np.isnan(want[j]) and np.isnan(got[j])):
                    bad.add((l, int(i), int(j)))
        past = np.arange(adjd.shape[2])[None, :] >= np.maximum(ex["deg"][l], 0)[:, None]
        assert not adjd[l][past].any(), l
    return bad


def _oracle(O, ex, metric, M, m0):
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=M, M0=m0, Ml=0.25, EfSearch=64)
    o.import_graph(**ex)
    return o


def _replay(H, O, g, ex, Q, metric, M, m0, own=None):
    """3: the oracle's searches on the export == the engine's (keys, counts, distance bits); an
    oracle flat index of the final vectors gives the same exact results; own = (keys, vectors):
    each vector finds its key first, at the self-distance's bits"""
    o = _oracle(O, ex, metric, M, m0)
    for ef in (64, 256):
        CR.same_lists(g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=ef), o.search(Q, 10, mode=O.MODE_BEAM, ef=ef))
    exact = g.search_arrays(Q, 10, mode=H.MODE_EXACT)
    CR.same_lists(exact, o.search(Q, 10, mode=O.MODE_EXACT))
    N = len(ex["keys"])
    flat = O.Graph(metric=metric, order=O.ORDER_DEV, M=M, M0=m0, Ml=0.25, EfSearch=64)
    flat.import_graph(keys=ex["keys"], vecs=ex["vecs"], deg=np.zeros((1, N), np.int32),
                      adj=np.full((1, N, 1), -1, np.int32), entry=np.zeros(1, np.int32), dead=ex["dead"])
    CR.same_lists(exact, flat.search(Q, 10, mode=O.MODE_EXACT))
    if own is not None:
        keys, V = own
        fn = _metric_fn(H, metric)
        k1, d1, n1 = g.search_arrays(V, 1, mode=H.MODE_EXACT)
        assert (n1 == 1).all() and k1[:, 0].tolist() == keys.tolist()
        self_d = np.array([fn.sweep(v, v[None])[0] for v in V], np.float32)
        assert np.array_equal(d1[:, 0].view(np.uint32), self_d.view(np.uint32))
        CR.same_lists(g.search_arrays(V, 10, mode=H.MODE_BEAM, ef=64), o.search(V, 10, mode=O.MODE_BEAM, ef=64))


def _recall(H, g, Q, ef=64, k=10):
    bk, _, bn = g.search_arrays(Q, k, mode=H.MODE_BEAM, ef=ef)
    xk, _, xn = g.search_arrays(Q, k, mode=H.MODE_EXACT)
    hit = sum(len(set(bk[b, :bn[b]].tolist()) & set(xk[b, :xn[b]].tolist())) for b in range(len(Q)))
    return hit / float(xn.sum())


def _self_found(H, g, keys, V, ef=64):
    bk, _, bn = g.search_arrays(V, 1, mode=H.MODE_BEAM, ef=ef)
    return float(np.mean((bn == 1) & (bk[:, 0] == keys)))


def _scenario(H, metric, n, d, M, m0, efc, nupd, seed=31, **opts):
    """A built graph with a few rows deleted and two filters, and an update of `nupd` keys that
    holds a deleted key and a key never added; nothing applied yet."""
    gen = Gen(seed + metric, d)
    X, labels = gen.rows(n)
    keys = _keys(n)
    g = _graph(H, metric, n, d, M, m0, efc, **opts)
    g.add_arrays(keys, X, levels=g.preview_levels(n))
    dead_rows = np.array([5, 17, n // 3, n - 7])
    assert g.BatchDelete(keys[dead_rows]) == [True] * len(dead_rows)
    f1 = g.Filter(keys[::3].tolist())
    f2 = g.Filter(keys[100:600].tolist())
    ex0 = g.export()
    rows = _update_rows(ex0, dead_rows, nupd - 2)
    ukeys = np.concatenate([keys[rows], [keys[17], 1]])  # (1 is no key: keys are 7 mod 3)
    V = gen.moved(np.concatenate([labels[rows], labels[[17, 0]]]))
    order = np.random.default_rng(seed).permutation(len(ukeys))  # not in row order
    Q, _ = gen.rows(200)
    return dict(g=g, X=X, keys=keys, ex0=ex0, rows=rows, ukeys=ukeys[order], V=V[order], Q=Q, filters=(f1, f2),
                dead_rows=dead_rows, gen=gen, labels=labels)


def _check_update(H, O, metric, shape, nupd, screen=1):
    """1-3 on one scenario"""
    M, m0 = shape["M"], shape["m0"]
    caps = [m0] + [M] * 31
    s = _scenario(H, metric, nupd=nupd, screen=screen, **shape)
    g, ex0, ukeys, V = s["g"], s["ex0"], s["ukeys"], s["V"]
    _invariants(ex0, caps)
    before_d = g.export_edge_dist()
    before = _edge_violations(H, metric, ex0, before_d)
    assert before == set(), sorted(before)[:5]
    state0 = (g.Len(), g.get_option("capacity"), g.get_option("dead_rows"), [f.count() for f in s["filters"]],
              g.preview_levels(16).tolist())
    found = g.update_arrays(ukeys, V)
    absent = (ukeys == s["keys"][17]) | (ukeys == 1)
    assert found.tolist() == (~absent).tolist()
    assert g.get_option("last_update_rows") == int(found.sum()) and g.get_option("last_update_chunks") >= 1
    assert g.get_option("last_update_repaired") > 0 and g.get_option("last_update_ns") == 0  # (time_build is off)
    assert g.stats()["dropped_proposals"] == 0
    # 1: ids and stores
    ex1 = g.export()
    assert np.array_equal(ex1["keys"], ex0["keys"]) and np.array_equal(ex1["dead"], ex0["dead"])
    assert np.array_equal(ex1["deg"] >= 0, ex0["deg"] >= 0) and np.array_equal(ex1["deg"] == -2, ex0["deg"] == -2)
    assert np.array_equal(ex1["entry"], ex0["entry"])
    row_of = {int(k): i for i, k in enumerate(s["keys"])}
    urows = np.array([row_of[int(k)] for k in ukeys[found]])
    assert sorted(urows.tolist()) == s["rows"].tolist()
    want = ex0["vecs"].copy()
    want[urows] = V[found]
    assert np.array_equal(ex1["vecs"].view(np.uint32), want.view(np.uint32))
    assert state0 == (g.Len(), g.get_option("capacity"), g.get_option("dead_rows"), [f.count() for f in s["filters"]],
                      g.preview_levels(16).tolist())
    # 2: invariants and edge distances
    _invariants(ex1, caps)
    after_d = g.export_edge_dist()
    after = _edge_violations(H, metric, ex1, after_d)
    assert after == set(), sorted(after)[:5]
    # 3: replay
    Q = np.concatenate([s["Q"], V[found]])
    _replay(H, O, g, ex1, Q, metric, M, m0, own=(ukeys[found], V[found]))
    # 4: the restatement (og_add_batch, delete mode 1, og_update) given the same calls builds the
    # same graph before and after the update: every field, adj in stored order, edge distance bits
    opts = dict(ef_construction=shape["efc"], heuristic=2, keep_pruned=1)
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=M, M0=m0, Ml=0.25, EfSearch=64)
    cn = o.add_batch(s["keys"], s["X"], BR.levels_of(ex0), **opts)
    assert all(o.delete(s["keys"][s["dead_rows"]], mode=1, heuristic=2, keep_pruned=1))
    BR.same_export(ex0, o.export(), before_d, o.export_edge_dist(), what="before the update")
    ofound, ucn = o.update(ukeys, V, **opts)
    assert ofound.tolist() == found.tolist()
    assert cn["dropped_proposals"] == 0 and ucn["dropped_proposals"] == 0
    assert ucn["update_chunks"] == g.get_option("last_update_chunks")
    assert ucn["repaired"] == g.get_option("last_update_repaired")
    BR.same_export(ex1, o.export(), after_d, o.export_edge_dist(), what="after the update")
    return s, ex1, urows


@pytest.mark.parametrize("screen", [1, 0])
@pytest.mark.parametrize("metric", [0, 1])
def test_update_ids_invariants_replay(H, O, metric, screen):
    s, _, _ = _check_update(H, O, metric, SHAPE, 300, screen=screen)
    s["g"].close()


def test_update_wide_rows(H, O):
    """4: the other row-engine configuration (three float4 a lane), cosine"""
    s, _, _ = _check_update(H, O, 0, WIDE, 64)
    s["g"].close()


@pytest.mark.parametrize("metric", [0, 1])
def test_update_against_delete_add(H, metric):
    """5: twin handles, A updated in place, B through Delete + Add at the rows' own levels"""
    sa = _scenario(H, metric, nupd=300, **SHAPE)
    sb = _scenario(H, metric, nupd=300, **SHAPE)
    CR.same_export(sa["ex0"], sb["ex0"])
    ga, gb, ukeys, V, keys = sa["g"], sb["g"], sa["ukeys"], sa["V"], sa["keys"]
    count0 = sa["filters"][1].count()
    found = ga.update_arrays(ukeys, V)
    present = gb.contains(ukeys.tolist())
    assert present.tolist() == found.tolist()
    lv = _levels(sb["ex0"])
    row_of = {int(k): i for i, k in enumerate(keys)}
    urows = np.array([row_of[int(k)] for k in ukeys[found]])
    assert gb.BatchDelete(ukeys[found].tolist()) == [True] * len(urows)
    gb.add_arrays(ukeys[found], V[found], levels=lv[urows])
    fa, fb = _self_found(H, ga, ukeys[found], V[found]), _self_found(H, gb, ukeys[found], V[found])
    ra, rb = _recall(H, ga, sa["Q"]), _recall(H, gb, sb["Q"])
    print(f"metric {metric}: self-found A {fa:.4f} B {fb:.4f}; recall@10 ef 64 A {ra:.4f} B {rb:.4f}")
    assert fa >= fb - 0.01
    assert ra >= rb - 0.01
    # a filter that held some of the keys: A returns the updated rows at their new distances,
    # on B they left the filter with their old rows
    f2a, f2b = sa["filters"][1], sb["filters"][1]
    held = np.flatnonzero(found & np.isin(ukeys, keys[100:600]))
    assert len(held) >= 10
    fn = _metric_fn(H, metric)
    for mode in (H.MODE_BEAM, H.MODE_EXACT):
        ak, ad, an = ga.search_filtered_arrays(V[held], 1, f2a, ef=64, mode=mode)
        self_d = np.array([fn.sweep(v, v[None])[0] for v in V[held]], np.float32)
        if mode == H.MODE_EXACT:
            assert (an == 1).all() and ak[:, 0].tolist() == ukeys[held].tolist()
            assert np.array_equal(ad[:, 0].view(np.uint32), self_d.view(np.uint32))
        else:  # (the beam is approximate: the rows it returns carry the new distances)
            hit = (an == 1) & (ak[:, 0] == ukeys[held])
            assert hit.any() and np.array_equal(ad[hit, 0].view(np.uint32), self_d[hit].view(np.uint32))
        bk, _, bn = gb.search_filtered_arrays(V[held], 10, f2b, ef=64, mode=mode)
        assert not np.isin(bk[np.arange(10)[None, :] < bn[:, None]], ukeys[held]).any()
    assert f2a.count() == count0 and f2b.count() == count0 - len(held)
    ga.close()
    gb.close()


def _small(H, metric, n=2000, seed=41):
    gen = Gen(seed, SHAPE["d"])
    X, labels = gen.rows(n)
    keys = _keys(n)
    shape = dict(SHAPE, n=n)
    g = _graph(H, metric, **shape)
    lv = g.preview_levels(n)
    g.add_arrays(keys, X, levels=lv)
    return g, gen, X, labels, keys, lv, shape


def test_update_every_row(H, O):
    """6: every row in one call, in chunks; the graph is a fresh build's equal at ef 64"""
    g, gen, X, labels, keys, lv, shape = _small(H, 0)
    X2, _ = gen.rows(len(keys))
    Q, _ = gen.rows(200)
    assert g.update_arrays(keys, X2).all()
    assert g.get_option("last_update_chunks") > 1 and g.get_option("last_update_rows") == len(keys)
    ex = g.export()
    caps = [shape["m0"]] + [shape["M"]] * 31
    _invariants(ex, caps)
    assert _edge_violations(H, 0, ex, g.export_edge_dist()) == set()
    assert np.array_equal(ex["vecs"].view(np.uint32), X2.view(np.uint32))
    _replay(H, O, g, ex, Q, 0, shape["M"], shape["m0"])
    fresh = _graph(H, 0, **shape)
    fresh.add_arrays(keys, X2, levels=lv)
    ru, rf = _recall(H, g, Q), _recall(H, fresh, Q)
    print(f"recall@10 ef 64: updated {ru:.4f} fresh {rf:.4f}")
    assert ru >= rf - 0.01
    fresh.close()
    g.close()


def test_update_top_layers(H, O):
    """6, second part: every member of the two highest layers in one call"""
    g, gen, X, labels, keys, lv, shape = _small(H, 0)
    ex0 = g.export()
    L = ex0["deg"].shape[0]
    assert L >= 3
    rows = np.flatnonzero(ex0["deg"][L - 2] >= 0)
    assert set(np.flatnonzero(ex0["deg"][L - 1] >= 0).tolist()) <= set(rows.tolist())
    V = gen.moved(labels[rows])
    g.set_option("batch_min", len(rows))  # one chunk holds them all
    assert g.update_arrays(keys[rows], V).all()
    assert g.get_option("last_update_chunks") == 1
    ex = g.export()
    _invariants(ex, [shape["m0"]] + [shape["M"]] * 31)
    assert _edge_violations(H, 0, ex, g.export_edge_dist()) == set()
    assert np.array_equal(ex["entry"], ex0["entry"]) and np.array_equal(ex["deg"] >= 0, ex0["deg"] >= 0)
    # layers whose every member was in the chunk have nothing to link
    assert (ex["deg"][L - 1][ex["deg"][L - 1] >= 0] == 0).all()
    Q, _ = gen.rows(200)
    _replay(H, O, g, ex, np.concatenate([Q, V]), 0, shape["M"], shape["m0"], own=(keys[rows], V))
    g.close()


def test_update_deterministic_and_life(H, O):
    """7: twin handles agree; afterwards the handle compacts, adds, deletes, updates and range-searches"""
    M, m0 = SHAPE["M"], SHAPE["m0"]
    caps = [m0] + [M] * 31
    sa, sb = _scenario(H, 0, nupd=300, **SHAPE), _scenario(H, 0, nupd=300, **SHAPE)
    ga, gb, ukeys, V, keys, gen = sa["g"], sb["g"], sa["ukeys"], sa["V"], sa["keys"], sa["gen"]
    fa, fb = ga.update_arrays(ukeys, V), gb.update_arrays(ukeys, V)
    assert fa.tolist() == fb.tolist()
    CR.same_export(ga.export(), gb.export())
    assert np.array_equal(ga.export_edge_dist().view(np.uint32), gb.export_edge_dist().view(np.uint32))
    assert ga.stats()["dropped_proposals"] == 0
    gb.close()
    Q = sa["Q"]
    # unchanged vectors: every exact result bit-identical (the graph is relinked, the store is not)
    x0 = ga.search_arrays(Q, 10, mode=H.MODE_EXACT)
    ex = ga.export()
    row_of = {int(k): i for i, k in enumerate(keys)}
    same = np.array([row_of[int(k)] for k in ukeys[fa]][:50])
    assert ga.update_arrays(keys[same], ex["vecs"][same]).all()
    CR.same_lists(x0, ga.search_arrays(Q, 10, mode=H.MODE_EXACT))
    assert np.array_equal(ga.export()["vecs"].view(np.uint32), ex["vecs"].view(np.uint32))
    # Compact: the export-restatement check
    want, dangling = CR.compact_export(ga.export())
    assert dangling == 0
    assert ga.Compact() == len(sa["dead_rows"])
    CR.same_export(ga.export(), want)
    # a later Add, a later Delete, a second update of the same keys, a range search
    n = len(keys)
    Xn, _ = gen.rows(100)
    nk = np.arange(100, dtype=np.int64) * 3 + 8
    ga.add_arrays(nk, Xn)
    assert ga.BatchDelete(keys[200:230].tolist()) == [True] * 30
    V2 = gen.moved(sa["labels"][[row_of.get(int(k), 0) for k in ukeys]])
    f2 = ga.update_arrays(ukeys, V2)
    gone = np.isin(ukeys, keys[200:230]) | ~fa
    assert f2.tolist() == (~gone).tolist()
    ex2 = ga.export()
    _invariants(ex2, caps)
    assert _edge_violations(H, 0, ex2, ga.export_edge_dist()) == set()
    assert ga.Len() == n - len(sa["dead_rows"]) + 100 - 30
    _replay(H, O, ga, ex2, np.concatenate([Q, Xn[:20]]), 0, M, m0, own=(ukeys[f2], V2[f2]))
    _, xd, _ = ga.search_arrays(V2[f2][:40], 5, mode=H.MODE_EXACT)
    lims, rk, rd = ga.range_search_arrays(V2[f2][:40], xd[:, 4].copy(), mode=H.MODE_EXACT)
    assert (np.diff(lims) >= 5).all() and rk[lims[:-1]].tolist() == ukeys[f2][:40].tolist()
    ga.close()


def test_update_refusals(H):
    """8: every refusal leaves the export as it was; a flat handle does what Replace does"""
    s = _scenario(H, 0, nupd=40, **SHAPE)
    g, keys, d = s["g"], s["keys"], SHAPE["d"]
    ex0, ed0, lv0 = g.export(), g.export_edge_dist(), g.preview_levels(8).tolist()
    V = s["V"][:4]
    with pytest.raises(H.HnswError, match="duplicate key 13 in update") as e:
        g.update_arrays(np.array([10, 13, 16, 13]), V)
    assert e.value.code == -1
    with pytest.raises(H.HnswError, match=f"embedding dimension mismatch: {d} != {d - 1}") as e:
        g.update_arrays(keys[:4], V[:, : d - 1])
    assert e.value.code == -2
    lib, C = H.load(), __import__("ctypes")
    out = (C.c_uint8 * 4)()
    k4 = np.ascontiguousarray(keys[:4])
    for kp, vp, op in ((None, V.ctypes.data_as(C.POINTER(C.c_float)), out),
                       (k4.ctypes.data_as(C.POINTER(C.c_int64)), None, out),
                       (k4.ctypes.data_as(C.POINTER(C.c_int64)), V.ctypes.data_as(C.POINTER(C.c_float)), None)):
        assert lib.mhnsw_update(g._h, kp, vp, 4, d, op) == -1
        assert b"must be non-NULL" in lib.mhnsw_last_error(g._h)
    CR.same_export(g.export(), ex0)
    assert np.array_equal(g.export_edge_dist().view(np.uint32), ed0.view(np.uint32))
    assert g.preview_levels(8).tolist() == lv0
    g.close()
    c = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=H.CosineDistance, Rng=3)
    c.add_arrays(keys[:50], s["X"][:50])
    with pytest.raises(H.HnswError, match=r"update needs a batch or flat \(build_mode 1 or 2\) handle") as e:
        c.update_arrays(keys[:4], V)
    assert e.value.code == -6
    c.close()
    # flat: the results of mhnsw_replace on a twin
    uk = np.concatenate([keys[40:480:11], [1]])
    Vf, _ = s["gen"].rows(len(uk))
    twins = []
    for call in ("update_arrays", "replace_arrays"):
        f = H.Graph(Distance=H.CosineDistance, build_mode=H.BUILD_FLAT)
        f.add_arrays(keys[:500], s["X"][:500])
        f.search_arrays(s["Q"], 10, mode=H.MODE_EXACT)  # (the exact path's planes exist)
        assert getattr(f, call)(uk, Vf).tolist() == [True] * (len(uk) - 1) + [False]
        twins.append((f, f.search_arrays(s["Q"], 10, mode=H.MODE_EXACT)))
    CR.same_lists(twins[0][1], twins[1][1])
    CR.same_export(twins[0][0].export(), twins[1][0].export())
    assert np.array_equal(twins[0][0].export()["vecs"][40:480:11].view(np.uint32), Vf[:-1].view(np.uint32))
    for f, _ in twins:
        f.close()


def test_update_device_entry(H):
    """9: mhnsw_update_device from a torch tensor gives the host call's export"""
    import torch

    sa, sb = _scenario(H, 1, nupd=120, **SHAPE), _scenario(H, 1, nupd=120, **SHAPE)
    ukeys, V = sa["ukeys"], sa["V"]
    fa = sa["g"].update_arrays(ukeys, V)
    t = torch.from_numpy(V).to("cuda")
    torch.cuda.synchronize()
    fb = sb["g"].update_device(ukeys, t.data_ptr(), len(ukeys), V.shape[1])
    assert fa.tolist() == fb.tolist()
    CR.same_export(sa["g"].export(), sb["g"].export())
    assert np.array_equal(sa["g"].export_edge_dist().view(np.uint32), sb["g"].export_edge_dist().view(np.uint32))
    CR.same_lists(sa["g"].search_arrays(sa["Q"], 10, mode=H.MODE_EXACT), sb["g"].search_arrays(sa["Q"], 10, mode=H.MODE_EXACT))
    sa["g"].close()
    sb["g"].close()
