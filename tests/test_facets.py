"""CPU: hnsw_amd.facets' store and filters -- the matching rules of the
reference's facets.go, with the nodes of its TestFacetedGraph as data.  (The
searches of FacetedGraph run on the GPU: tests/test_gpu_filtered.py.)"""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def F(H):
    from hnsw_amd import facets

    return facets


def _store(H, F):
    s = F.MemoryFacetStore()
    # facets_test.go:20-38
    s.Add(F.NewFacetedNode(H.MakeNode(1, [0.1, 0.2, 0.3]), [F.BasicFacet("category", "Electronics"),
                                                            F.BasicFacet("price", 150.0)]))
    s.Add(F.NewFacetedNode(H.MakeNode(2, [0.2, 0.3, 0.4]), [F.BasicFacet("category", "Electronics"),
                                                            F.BasicFacet("price", 200.0)]))
    s.Add(F.NewFacetedNode(H.MakeNode(3, [0.9, 0.1, 0.0]), [F.BasicFacet("category", "Garden Tools"),
                                                            F.BasicFacet("price", 20), F.BasicFacet("stock", True)]))
    return s


# (filters, the keys they keep)
CASES = [
    (lambda F: [], {1, 2, 3}),
    (lambda F: None, {1, 2, 3}),
    (lambda F: [F.EqualityFilter("category", "Electronics")], {1, 2}),
    (lambda F: [F.EqualityFilter("category", "electronics")], set()),            # equality is exact
    (lambda F: [F.EqualityFilter("price", 150.0)], {1}),
    (lambda F: [F.EqualityFilter("price", 150)], set()),                         # DeepEqual is typed: int != float64
    (lambda F: [F.EqualityFilter("price", 20)], {3}),
    (lambda F: [F.EqualityFilter("colour", "red")], set()),                      # no such facet
    (lambda F: [F.RangeFilter("price", 100, 175)], {1}),
    (lambda F: [F.RangeFilter("price", 150, 200)], {1, 2}),                      # both ends inclusive
    (lambda F: [F.RangeFilter("price", 0, 1000)], {1, 2, 3}),                    # int and float values
    (lambda F: [F.RangeFilter("category", 0, 1000)], set()),                     # a non-numeric value never matches
    (lambda F: [F.RangeFilter("stock", 0, 1)], set()),                           # nor does a bool
    (lambda F: [F.StringContainsFilter("category", "TOOLS")], {3}),              # case-insensitive
    (lambda F: [F.StringContainsFilter("category", "tron")], {1, 2}),
    (lambda F: [F.StringContainsFilter("price", "50")], {1}),                    # other values through their text
    (lambda F: [F.StringContainsFilter("stock", "TRUE")], {3}),
    (lambda F: [F.EqualityFilter("category", "Electronics"), F.RangeFilter("price", 175, 300)], {2}),  # all must match
    (lambda F: [F.EqualityFilter("category", "Electronics"), F.StringContainsFilter("category", "garden")], set()),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_store_filter(H, F, i):
    make, want = CASES[i]
    s = _store(H, F)
    assert {n.Node.Key for n in s.Filter(make(F))} == want
    for n in s.GetAllNodes():
        assert n.MatchesAllFilters(make(F)) == (n.Node.Key in want)


def test_store_and_node(H, F):
    s = _store(H, F)
    n, ok = s.Get(1)
    assert ok and n.Node.Key == 1 and np.allclose(n.Node.Value, [0.1, 0.2, 0.3])
    assert n.GetFacet("price").Value() == 150.0 and n.GetFacet("price").Name() == "price"
    assert n.GetFacet("nope") is None
    assert n.GetFacet("price").Match(150.0) and not n.GetFacet("price").Match(150)
    assert not n.MatchesFilter(F.EqualityFilter("nope", 1))
    assert s.Get(9) == (None, False)
    assert s.Delete(1) and not s.Delete(1)
    assert s.Get(1) == (None, False) and len(s.GetAllNodes()) == 2
    # Add replaces the node of a present key
    s.Add(F.NewFacetedNode(H.MakeNode(2, [0.0, 0.0, 1.0]), [F.BasicFacet("category", "Books")]))
    assert len(s.GetAllNodes()) == 2 and s.Get(2)[0].GetFacet("price") is None


@pytest.mark.parametrize("value,text", [
    (150.0, "150"), (0.5, "0.5"), (199.99, "199.99"), (-2.5, "-2.5"), (0.0, "0"), (123456.0, "123456"),
    (1e6, "1e+06"), (1234567.0, "1.234567e+06"), (1e21, "1e+21"), (9.223372036854776e18, "9.223372036854776e+18"),
    (0.0001, "0.0001"), (1e-5, "1e-05"), (float("inf"), "+Inf"), (True, "true"), (20, "20"), ("Abc", "Abc"),
])
def test_values_print_as_go_prints_them(F, value, text):
    """what StringContainsFilter searches in for a value that is no string: fmt's
    %v, for a float64 strconv's shortest 'g' form"""
    assert F._go_text(value) == text
    assert F.StringContainsFilter("x", text).Matches(value)


def test_facet_error_text(F):
    e = F.FacetError("k must be greater than 0")
    assert str(e) == "facet error: k must be greater than 0" and e.Message == "k must be greater than 0"
