"""The Python host's Update / Upsert (hnsw_amd.Graph) over mhnsw_update: int, float and
string keys through the existing key images, Upsert = Update of the present keys + BatchAdd
of the absent ones, and the facets extension's cached device filters over an updated row."""
import numpy as np
import pytest

from tests import compact_ref as CR

pytestmark = pytest.mark.gpu

D = 16


def _graph(H):
    return H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=H.EuclideanDistance, Rng=3, build_mode=H.BUILD_BATCH, m0=16,
                   ef_construction=32)


def _vecs(seed, n):
    return np.random.default_rng(seed).normal(size=(n, D)).astype(np.float32)


KEYS = {
    "int": lambda i: 10 * i + 1,
    "float": lambda i: i * 0.5 - 20.25,
    "str": lambda i: f"doc-{i:04d}",
}


@pytest.mark.parametrize("kind", ["int", "float", "str"])
def test_update_and_upsert_keys(H, kind):
    key = KEYS[kind]
    X = _vecs(1, 200)
    g = _graph(H)
    g.BatchAdd([H.MakeNode(key(i), X[i]) for i in range(200)])
    assert g.Delete(key(9))
    V = _vecs(2, 6) + 8.0  # far from every stored row
    found = g.Update([H.MakeNode(key(3), V[0]), H.MakeNode(key(150), V[1]), H.MakeNode(key(9), V[2]),
                      H.MakeNode(key(5000), V[3])])
    assert found == [True, True, False, False]
    assert g.Len() == 199 and g.get_option("last_update_rows") == 2
    for i, v in ((3, V[0]), (150, V[1])):
        assert [n.Key for n in g.Search(v, 1, mode=H.MODE_BEAM)] == [key(i)]
        got, ok = g.Lookup(key(i))
        assert ok and np.array_equal(got, v)
    assert key(3) not in [n.Key for n in g.Search(X[3], 3, mode=H.MODE_EXACT)]
    # Upsert: 150 present; 9 (deleted) and 5000 (never added) are added
    found = g.Upsert([H.MakeNode(key(5000), V[3]), H.MakeNode(key(150), V[4]), H.MakeNode(key(9), V[5])])
    assert found == [False, True, False]
    assert g.Len() == 201
    for i, v in ((5000, V[3]), (150, V[4]), (9, V[5])):
        assert [n.Key for n in g.Search(v, 1, mode=H.MODE_EXACT)] == [key(i)]
    with pytest.raises(H.HnswError, match="duplicate key .* in update") as e:
        g.Upsert([H.MakeNode(key(4), V[0]), H.MakeNode(key(4), V[1])])
    assert e.value.code == -1
    assert g.Update([]) == [] and g.Upsert([]) == []
    g.close()


def test_upsert_is_update_plus_batchadd(H):
    X = _vecs(4, 300)
    nodes = [H.MakeNode(7 * i, X[i]) for i in range(300)]
    V = _vecs(5, 40)
    mixed = [H.MakeNode(7 * i if j % 2 else 7 * i + 3, V[j]) for j, i in enumerate(range(20, 260, 6))]
    present = [n for n in mixed if n.Key % 7 == 0]
    absent = [n for n in mixed if n.Key % 7]
    a, b = _graph(H), _graph(H)
    a.BatchAdd(nodes)
    b.BatchAdd(nodes)
    assert a.Upsert(mixed) == [n.Key % 7 == 0 for n in mixed]
    assert b.Update(present) == [True] * len(present)
    b.BatchAdd(absent)
    CR.same_export(a.export(), b.export())
    assert np.array_equal(a.export_edge_dist().view(np.uint32), b.export_edge_dist().view(np.uint32))
    assert a.Len() == 300 + len(absent)
    a.close()
    b.close()


def test_facets_follow_an_updated_row(H):
    """the facets extension's device filter is cached while the store is unchanged: an updated
    row keeps its id, so it is still found through it, at its new vector"""
    from hnsw_amd import facets as F

    X = _vecs(6, 120)
    fg = F.FacetedGraph(_graph(H))
    fg.BatchAdd([F.NewFacetedNode(H.MakeNode(i, X[i]), [F.BasicFacet("colour", "red" if i % 3 == 0 else "blue")])
                 for i in range(120)])
    red = [F.EqualityFilter("colour", "red")]
    assert [n.Node.Key for n in fg.Search(X[30], red, 1, mode=H.MODE_BEAM, ef=32)] == [30]
    v = (X[30] + 9.0).astype(np.float32)
    assert fg.Graph.Update([H.MakeNode(30, v)]) == [True]
    for mode in (H.MODE_BEAM, H.MODE_EXACT):
        assert [n.Node.Key for n in fg.Search(v, red, 1, mode=mode, ef=32)] == [30]
        assert fg.Search(X[30], red, 1, mode=mode, ef=32)[0].Node.Key != 30
    assert fg.Search(v, [F.EqualityFilter("colour", "blue")], 1, mode=H.MODE_EXACT)[0].Node.Key != 30
    fg.close()
    fg.Graph.close()
