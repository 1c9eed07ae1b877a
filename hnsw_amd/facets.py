"""Faceted search: the reference's hnsw-extensions/facets package (facets.go,
search.go) over this engine.

A FacetedGraph pairs a Graph with a store of per-key attributes.  Its Search
has three modes:

MODE_COMPAT  the reference's procedure, literally (search.go:15-88): Search for
             k * expandFactor neighbours, keep the ones whose facets match, ask
             once more for twice as many when that came up short, sort by
             distance, cut to k.
MODE_BEAM    the engine's filtered beam search (Graph.search_filtered_arrays):
             the keys of store.Filter(filters) become a device-resident
             allow-list (cached per filter list) and the predicate is applied
             inside the layer-0 walk; expandFactor does not apply.
MODE_EXACT   the same allow-list, searched by the engine's filtered exact
             search (brute force over the allowed rows only): the exact k
             nearest matching nodes; expandFactor, ef and route do not apply.

RangeSearch (not in the reference) returns every matching node within a radius
of the query, through the same allow-list (Graph.range_search_arrays).

Go's interface{} values are Python objects here.  reflect.DeepEqual is typed:
an int never equals a float, so values compare equal only within one type.
"""
from __future__ import annotations

from decimal import Decimal
from typing import Any, Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from ._lib import HnswError
from .graph import Graph, Node

MODE_COMPAT, MODE_BEAM, MODE_EXACT = 0, 1, 2


class FacetError(Exception):  # facets.go:279-286
    def __init__(self, Message: str):
        super().__init__(f"facet error: {Message}")
        self.Message = Message


def _deep_equal(a, b) -> bool:
    """reflect.DeepEqual on facet values: same dynamic type and equal"""
    return type(a) is type(b) and bool(a == b)


def _go_float(v: float) -> str:
    """strconv.FormatFloat(v, 'g', -1, 64), what %v prints for a float64: the
    shortest digits that round-trip; plain notation for a decimal exponent in
    [-4, 6) (with the shortest digits strconv decides as at precision 6:
    1e6 prints "1e+06", 9.223372036854776e18 so), else d.ddde+XX with at least
    two exponent digits"""
    if v != v:
        return "NaN"
    if v in (float("inf"), float("-inf")):
        return "+Inf" if v > 0 else "-Inf"
    sign, digits, exp = Decimal(repr(v)).as_tuple()
    digits = "".join(map(str, digits)).rstrip("0") or "0"
    if digits == "0":
        return "-0" if sign else "0"
    e10 = len("".join(map(str, Decimal(repr(v)).as_tuple()[1]))) + exp - 1  # of the first digit
    neg = "-" if sign else ""
    if -4 <= e10 < 6:
        if e10 < 0:
            return neg + "0." + "0" * (-e10 - 1) + digits
        if len(digits) <= e10 + 1:
            return neg + digits + "0" * (e10 + 1 - len(digits))
        return neg + digits[: e10 + 1] + "." + digits[e10 + 1:]
    mant = digits[0] + ("." + digits[1:] if len(digits) > 1 else "")
    return f"{neg}{mant}e{'-' if e10 < 0 else '+'}{abs(e10):02d}"


def _go_text(v) -> str:
    """fmt.Sprintf("%v", v) for the values a facet holds: a float as Go prints
    a float64 (150.0 -> "150", 2500000.0 -> "2.5e+06"), a bool in lower case"""
    if isinstance(v, str):
        return v
    if isinstance(v, (bool, np.bool_)):
        return "true" if v else "false"
    if isinstance(v, (float, np.floating)):
        return _go_float(float(v))
    return str(v)


class BasicFacet:  # facets.go:78-105
    def __init__(self, name: str, value: Any):
        self._name, self._value = name, value

    def Name(self) -> str:
        return self._name

    def Value(self) -> Any:
        return self._value

    def Match(self, query: Any) -> bool:
        return _deep_equal(self._value, query)


class EqualityFilter:  # facets.go:108-129
    def __init__(self, name: str, value: Any):
        self._name, self._value = name, value

    def Name(self) -> str:
        return self._name

    def Matches(self, value: Any) -> bool:
        return _deep_equal(self._value, value)

    def _cache_key(self):
        return ("eq", self._name, type(self._value).__name__, repr(self._value))


class RangeFilter:  # facets.go:132-172
    def __init__(self, name: str, min: float, max: float):
        self._name, self._min, self._max = name, float(min), float(max)

    def Name(self) -> str:
        return self._name

    def Matches(self, value: Any) -> bool:
        # Go's numeric cases: float64, float32, int, int64, int32 -- a bool or a
        # string is "not a numeric type"
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
            return False
        v = float(value)
        return self._min <= v <= self._max

    def _cache_key(self):
        return ("range", self._name, self._min, self._max)


class StringContainsFilter:  # facets.go:175-206
    def __init__(self, name: str, contains: str):
        self._name, self._contains = name, contains

    def Name(self) -> str:
        return self._name

    def Matches(self, value: Any) -> bool:
        return self._contains.lower() in _go_text(value).lower()

    def _cache_key(self):
        return ("contains", self._name, self._contains.lower())


class FacetedNode(NamedTuple):  # facets.go:35-75
    Node: Node
    Facets: Sequence[Any]

    def GetFacet(self, name: str):
        return next((f for f in self.Facets if f.Name() == name), None)

    def MatchesFilter(self, flt) -> bool:
        f = self.GetFacet(flt.Name())
        return f is not None and flt.Matches(f.Value())

    def MatchesAllFilters(self, filters) -> bool:
        return all(self.MatchesFilter(f) for f in (filters or ()))


def NewFacetedNode(node: Node, facets: Sequence[Any]) -> FacetedNode:
    return FacetedNode(node, list(facets))


class MemoryFacetStore:  # facets.go:224-276
    def __init__(self):
        self.nodes: Dict[Any, FacetedNode] = {}
        self.version = 0  # bumped by every change (FacetedGraph's filter cache)

    def Add(self, node: FacetedNode):
        self.nodes[node.Node.Key] = node
        self.version += 1

    def Get(self, key):
        n = self.nodes.get(key)
        return n, n is not None

    def Delete(self, key) -> bool:
        self.version += 1
        return self.nodes.pop(key, None) is not None

    def Filter(self, filters) -> List[FacetedNode]:
        return [n for n in self.nodes.values() if n.MatchesAllFilters(filters)]

    def GetAllNodes(self) -> List[FacetedNode]:
        return list(self.nodes.values())


class FacetAggregation(NamedTuple):  # search.go:277-280
    Name: str
    Values: Dict[Any, int]


class FacetedGraph:  # search.go:166-329
    def __init__(self, graph: Graph, store: Optional[MemoryFacetStore] = None):
        self.Graph = graph
        self.Store = store if store is not None else MemoryFacetStore()
        self._filters: Dict[tuple, tuple] = {}  # filter list -> (store version, graph Filter)

    def close(self):
        for _, f in self._filters.values():
            try:
                f.close()
            except HnswError:  # (dropped by an Import: the engine no longer knows it)
                pass
        self._filters.clear()

    def Add(self, node: FacetedNode):
        self.Graph.Add(node.Node)
        self.Store.Add(node)

    def BatchAdd(self, nodes: Sequence[FacetedNode]):
        self.Graph.BatchAdd([n.Node for n in nodes])
        for n in nodes:
            self.Store.Add(n)

    def Delete(self, key) -> bool:
        a = self.Graph.Delete(key)
        b = self.Store.Delete(key)
        return a or b

    def BatchDelete(self, keys) -> List[bool]:
        keys = list(keys)
        a = self.Graph.BatchDelete(keys)
        b = [self.Store.Delete(k) for k in keys]
        return [x or y for x, y in zip(a, b)]

    # -- search.go:15-88 ---------------------------------------------------------
    def _matching(self, candidates, filters) -> List[FacetedNode]:
        out = []
        for c in candidates:
            n, ok = self.Store.Get(c.Key)
            if ok and n.MatchesAllFilters(filters):
                out.append(n)
        return out

    def _search_compat(self, query, filters, k: int, expandFactor: int) -> List[FacetedNode]:
        if expandFactor <= 0:
            expandFactor = 3
        wide = k * expandFactor
        cand = self.Graph.Search(query, wide)
        found = self._matching(cand, filters)
        if len(found) < k and len(cand) == wide:
            more = self.Graph.Search(query, wide * 2)
            found += self._matching(more[wide:], filters)
        q = np.asarray(query, np.float32)
        dist = [self.Graph.Distance(n.Node.Value, q) for n in found]
        order = sorted(range(len(found)), key=lambda i: dist[i])  # (stable, as the distances are computed once)
        return [found[i] for i in order][:k]

    def _device_filter(self, filters, fresh: bool = False):
        """-> (the device filter of store.Filter(filters), cached).  Cached per
        filter list while the store is unchanged, for the built-in filter kinds
        only: a filter object of another class has no value to key on (its
        address can be reused by another predicate), so it is built per search.
        fresh: rebuild even on a hit (the engine dropped the cached one)."""
        filters = list(filters or ())
        key = tuple(f._cache_key() for f in filters) if all(hasattr(f, "_cache_key") for f in filters) else None
        hit = self._filters.get(key) if key is not None else None
        if hit is not None and not fresh and hit[0] == self.Store.version and hit[1].id is not None:
            return hit[1], True
        if hit is not None:
            del self._filters[key]
            try:
                hit[1].close()
            except HnswError:  # (dropped by an Import: the engine no longer knows it)
                pass
        f = self.Graph.Filter([n.Node.Key for n in self.Store.Filter(filters)])
        if key is not None:
            self._filters[key] = (self.Store.version, f)
        return f, key is not None

    def Search(self, query, filters, k: int, expandFactor: int = 0, mode: int = MODE_COMPAT, ef: int = 0,
               route: int = 0) -> List[FacetedNode]:
        if k <= 0:
            raise FacetError("k must be greater than 0")
        if mode == MODE_COMPAT:
            return self._search_compat(query, filters, k, expandFactor)
        if mode not in (MODE_BEAM, MODE_EXACT):
            raise FacetError(f"unknown search mode {mode}")
        q = np.asarray(query, np.float32).reshape(1, -1)
        f, cached = self._device_filter(filters)
        try:
            try:
                keys, _, n = self.Graph.search_filtered_arrays(q, k, f, ef=ef, route=route, mode=mode)
            except HnswError as e:
                if not cached or "unknown filter" not in str(e):
                    raise
                # the graph was Imported since: its filters are gone, the store's keys are not
                f, cached = self._device_filter(filters, fresh=True)
                keys, _, n = self.Graph.search_filtered_arrays(q, k, f, ef=ef, route=route, mode=mode)
        finally:
            if not cached:
                f.close()
        out = []
        for key in self.Graph.decode_keys(keys[0, : n[0]]):
            node, ok = self.Store.Get(key)
            if ok:
                out.append(node)
        return out

    def RangeSearch(self, query, filters, radius: float, mode: int = MODE_EXACT, ef: int = 0,
                    route: int = 0) -> List[FacetedNode]:
        """Every node that matches `filters` within `radius` of the query,
        nearest first (Graph.RangeSearch over the filter list's allow-list).
        MODE_EXACT returns all of them; MODE_BEAM the ones the filtered walk at
        k = ef finds.  The reference has no such call: it extends Search."""
        if mode not in (MODE_BEAM, MODE_EXACT):
            raise FacetError(f"range search supports beam and exact mode, got mode {mode}")
        q = np.asarray(query, np.float32).reshape(1, -1)
        f, cached = self._device_filter(filters)
        kw = dict(mode=mode, ef=ef, route=route)
        try:
            try:
                _, keys, _ = self.Graph.range_search_arrays(q, radius, filters=f, **kw)
            except HnswError as e:
                if not cached or "unknown filter" not in str(e):
                    raise
                # the graph was Imported since: its filters are gone, the store's keys are not
                f, cached = self._device_filter(filters, fresh=True)
                _, keys, _ = self.Graph.range_search_arrays(q, radius, filters=f, **kw)
        finally:
            if not cached:
                f.close()
        out = []
        for key in self.Graph.decode_keys(keys):
            node, ok = self.Store.Get(key)
            if ok:
                out.append(node)
        return out

    # -- search.go:283-329 -------------------------------------------------------
    def GetFacetAggregations(self, query, filters, facetNames: Sequence[str], k: int,
                             expandFactor: int) -> Dict[str, FacetAggregation]:
        cand = self.Graph.Search(query, k * expandFactor)
        agg = {name: FacetAggregation(name, {}) for name in facetNames}
        for n in self._matching(cand, filters):
            for name in facetNames:
                f = n.GetFacet(name)
                if f is not None:
                    agg[name].Values[f.Value()] = agg[name].Values.get(f.Value(), 0) + 1
        return agg
