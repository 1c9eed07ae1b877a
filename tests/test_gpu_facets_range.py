"""GPU: hnsw_amd.facets.FacetedGraph.RangeSearch -- every node that matches a filter list
within a radius.  It equals the masked cut: the plain range search's hits (checked against the
oracle by tests/test_gpu_range.py) with the nodes that do not match removed, in the same order.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D = 1200, 16
CATS = ["Electronics", "Books", "Garden tools", "Toys"]


@pytest.fixture(scope="module")
def catalogue(H):
    from hnsw_amd import facets as F

    rng = np.random.default_rng(17)
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=5, build_mode=H.BUILD_BATCH)
    fg = F.FacetedGraph(g, F.MemoryFacetStore())
    X = rng.normal(size=(N, D)).astype(np.float32)
    fg.BatchAdd([F.NewFacetedNode(H.MakeNode(i, X[i]), [F.BasicFacet("category", CATS[i % 4]),
                                                         F.BasicFacet("price", float(10 + (i * 37) % 500))])
                 for i in range(N)])
    assert fg.Delete(5) and fg.Delete(402)  # a Books row and another, gone from graph and store
    yield F, fg, X
    fg.close()
    g.close()


def _masked_cut(fg, q, filters, radius, **kw):
    """the plain range search's keys, the ones whose node matches"""
    out = []
    for n in fg.Graph.RangeSearch(q, radius, **kw):
        node, ok = fg.Store.Get(n.Key)
        if ok and node.MatchesAllFilters(filters):
            out.append(n.Key)
    return out


def test_equality_and_range_filters(catalogue, H):
    F, fg, X = catalogue
    books = [F.EqualityFilter("category", "Books")]  # 299 rows: the filter GEMM over the gathered plane
    cheap = [F.EqualityFilter("category", "Books"), F.RangeFilter("price", 100, 200)]  # a few dozen: the sweep
    everything = None
    for filters in (books, cheap, everything):
        for i in (1, 2, 9, 64):
            q = X[i] + np.float32(0.01)
            d = np.sort(H.CosineDistance.sweep(q, X))
            for radius in (float(d[40]), float(d[400]), 3.0, -1.0):
                got = fg.RangeSearch(q, filters, radius)
                assert [n.Node.Key for n in got] == _masked_cut(fg, q, filters, radius), (filters, i, radius)
                assert all(n.MatchesAllFilters(filters) for n in got)
            if filters is books:  # X[1] is a Books row 0.01 away; the deleted row 5 never comes back
                every = [n.Node.Key for n in fg.RangeSearch(q, filters, 3.0)]
                assert len(every) == 299 and 5 not in every and (i != 1 or every[0] == 1)
    assert len(fg._filters) == 3  # one device filter per filter list, cached


def test_beam_mode_and_errors(catalogue, H):
    F, fg, X = catalogue
    books = [F.EqualityFilter("category", "Books")]
    q = X[9] + np.float32(0.01)
    radius = float(np.sort(H.CosineDistance.sweep(q, X))[200])
    exact = [n.Node.Key for n in fg.RangeSearch(q, books, radius)]
    beam = [n.Node.Key for n in fg.RangeSearch(q, books, radius, mode=F.MODE_BEAM, ef=64, route=512)]
    assert beam and set(beam) <= set(exact) and beam == [k for k in exact if k in set(beam)]
    f = fg._device_filter(books)[0]
    _, keys, _ = fg.Graph.range_search_arrays(q, radius, filters=f, mode=H.MODE_BEAM, ef=64, route=512)
    assert beam == keys.tolist()
    with pytest.raises(F.FacetError, match="range search supports beam and exact mode"):
        fg.RangeSearch(q, books, radius, mode=F.MODE_COMPAT)
    with pytest.raises(H.HnswError, match=r"filtered search supports max\(ef,k\) <= 128"):
        fg.RangeSearch(q, books, radius, mode=F.MODE_BEAM, ef=200)


def test_after_an_import_dropped_the_filters(catalogue, H):
    """an Import drops the engine's filters: the cached one is rebuilt, not reported"""
    F, fg, X = catalogue
    g = fg.Graph
    filters = [F.RangeFilter("price", 50, 300)]
    q = X[2] + np.float32(0.01)
    radius = float(np.sort(H.CosineDistance.sweep(q, X))[300])
    before = [n.Node.Key for n in fg.RangeSearch(q, filters, radius)]
    assert before and before == _masked_cut(fg, q, filters, radius)
    stale = fg._device_filter(filters)[0]
    g.import_bytes(g.export_bytes())
    got = [n.Node.Key for n in fg.RangeSearch(q, filters, radius)]
    assert got == _masked_cut(fg, q, filters, radius) and sorted(got) == sorted(before)
    assert fg._device_filter(filters)[0] is not stale
    # an uncacheable filter object is built per search and closed again
    class Odd:
        def Name(self):
            return "price"

        def Matches(self, v):
            return int(v) % 2 == 1

    n_before = len(fg._filters)
    got = [n.Node.Key for n in fg.RangeSearch(q, [Odd()], radius)]
    assert got == _masked_cut(fg, q, [Odd()], radius) and len(fg._filters) == n_before
