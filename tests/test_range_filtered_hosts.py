"""The filtered range search's host surfaces without a device: include/mhnsw.h declares the
two entry points, hnsw_amd._lib binds them with matching argument types and the built library
exports them; the Python hosts take a filter and check their arguments before any device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mhnsw_range_search_filtered", "mhnsw_range_search_filtered_device")

# a C parameter's declared type -> the ctypes type _lib.py binds it with (device buffers and
# the stream are opaque pointers there)
_HOST = {"mhnsw_index *": C.c_void_p, "const float *": C.POINTER(C.c_float), "int64_t": C.c_int64, "int": C.c_int,
         "const int32_t *": C.POINTER(C.c_int32), "int64_t *": C.POINTER(C.c_int64)}
_DEVICE = dict(_HOST, **{"const float *": C.c_void_p, "int64_t *": C.c_void_p, "float *": C.c_void_p,
                         "void *": C.c_void_p})


def _decl(name):
    src = open(os.path.join(ROOT, "include", "mhnsw.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, name
    out = []
    for a in m.group(1).replace("\n", " ").split(","):
        t, n = re.match(r"\s*(.*?)(\w+)\s*$", a).groups()
        out.append((t.strip(), n))
    return out


def test_header_declares_and_binding_binds(H):
    lib = H.load()
    for name, types in zip(NAMES, (_HOST, _DEVICE)):
        args = _decl(name)
        res, sig = H.SIGNATURES[name]
        assert res is C.c_int and hasattr(lib, name), name
        assert [types[t] for t, _ in args] == list(sig), name
    assert [n for _, n in _decl(NAMES[0])] == ["h", "queries", "B", "dim", "radius", "mode", "ef", "route", "filter_of",
                                               "out_lims"]
    assert [n for _, n in _decl(NAMES[1])] == ["h", "d_queries", "B", "dim", "d_radius", "mode", "ef", "route", "filter",
                                               "cap", "d_lims", "d_keys", "d_dist", "stream"]


def test_python_hosts_take_a_filter(H):
    p = inspect.signature(H.Graph.range_search_arrays).parameters
    assert p["filters"].default is None and p["route"].default == 0 and p["mode"].default == H.MODE_EXACT
    assert list(p)[:5] == ["self", "queries", "radius", "mode", "ef"]  # today's positional calls keep their meaning
    p = inspect.signature(H.Graph.RangeSearch).parameters
    assert p["filter"].default is None and list(p)[:5] == ["self", "near", "radius", "mode", "ef"]
    p = inspect.signature(H.Graph.range_search_filtered_device).parameters
    assert p["mode"].default == H.MODE_EXACT and p["route"].default == 0 and p["stream"].default == 0
    assert inspect.signature(H.ExactIndex.RangeSearch).parameters["filter"].default is None
    assert inspect.signature(H.ExactIndex.range_search_batch).parameters["filters"].default is None
    from hnsw_amd import facets

    p = inspect.signature(facets.FacetedGraph.RangeSearch).parameters
    assert list(p) == ["self", "query", "filters", "radius", "mode", "ef", "route"]
    assert p["mode"].default == facets.MODE_EXACT == H.MODE_EXACT and p["ef"].default == 0 and p["route"].default == 0


def _bare(H):
    """a Graph and two Filters that never touched a device: only what the checks read"""
    g, other = object.__new__(H.Graph), object.__new__(H.Graph)
    g._h = other._h = None
    fs = []
    for owner, fid in ((g, 3), (other, 4)):
        f = object.__new__(H.Filter)
        f._g, f.id, f._was = owner, fid, fid
        fs.append(f)
    return g, fs[0], fs[1]


def test_argument_errors_before_the_device(H):
    g, mine, foreign = _bare(H)
    Q = np.zeros((3, 4), np.float32)
    with pytest.raises(H.HnswError, match="2 filters for 3 queries") as e:
        g.range_search_arrays(Q, 0.5, filters=[mine, None])
    assert e.value.code == H._lib.EINVAL
    with pytest.raises(H.HnswError, match="filter of another graph") as e:
        g.range_search_arrays(Q, 0.5, filters=foreign)
    assert e.value.code == H._lib.EINVAL
    with pytest.raises(H.HnswError, match="filter of another graph"):
        g.range_search_arrays(Q, 0.5, filters=[mine, foreign, None])
    with pytest.raises(H.HnswError, match="filter of another graph"):
        g.range_search_filtered_device(0, 3, 4, 0, foreign, 0, 0, 0, 0)
    with pytest.raises(H.HnswError, match="range search supports beam and exact mode") as e:
        g.range_search_arrays(Q, 0.5, mode=H.MODE_COMPAT, filters=mine)
    assert e.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match="range search supports beam and exact mode"):
        g.RangeSearch(Q[0], 0.5, mode=H.MODE_COMPAT, filter=mine)
    mine.id = None  # closed
    with pytest.raises(H.HnswError, match="unknown filter 3"):
        g.range_search_arrays(Q, 0.5, filters=mine)
    assert np.array_equal(g._filter_ids([None, None], 2), [-1, -1])
