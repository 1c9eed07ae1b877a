"""The range search's host surfaces without a device: include/mhnsw.h declares the three
entry points and hnsw_amd._lib binds them with the same arguments, the Python hosts check
their arguments before any device work, and the ragged result unpacks per query."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mhnsw_range_search", "mhnsw_range_results", "mhnsw_range_search_device")


def _decl(name):
    src = open(os.path.join(ROOT, "include", "mhnsw.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_header_declares_and_binding_binds(H):
    lib = H.load()
    for name in NAMES:
        args = _decl(name)
        res, sig = H.SIGNATURES[name]
        assert res is C.c_int and len(sig) == len(args) and hasattr(lib, name), name
    # h, queries, B, dim, radius, mode, ef, out_lims
    assert [a.split()[-1].lstrip("*") for a in _decl(NAMES[0])] == ["h", "queries", "B", "dim", "radius", "mode", "ef",
                                                                   "out_lims"]
    sig = H.SIGNATURES[NAMES[0]][1]
    assert sig[2] is C.c_int64 and sig[4] is C.POINTER(C.c_float) and sig[7] is C.POINTER(C.c_int64)
    # h, out_keys, out_dist, cap
    assert H.SIGNATURES[NAMES[1]][1][3] is C.c_int64
    # ..., mode, ef, cap, d_lims, d_keys, d_dist, stream
    dev = [a.split()[-1].lstrip("*") for a in _decl(NAMES[2])]
    assert dev[5:] == ["mode", "ef", "cap", "d_lims", "d_keys", "d_dist", "stream"]
    assert H.SIGNATURES[NAMES[2]][1][7] is C.c_int64


def test_python_hosts(H):
    for fn in (H.Graph.range_search_arrays, H.Graph.RangeSearch, H.ExactIndex.RangeSearch):
        p = inspect.signature(fn).parameters
        assert p["mode"].default == H.MODE_EXACT and p["ef"].default == 0
    assert inspect.signature(H.Graph.range_search_device).parameters["mode"].default == H.MODE_EXACT


def test_argument_errors_before_the_device(H):
    Q = np.zeros((3, 4), np.float32)
    q, rad = H.Graph._range_io(Q, 0.25, H.MODE_EXACT)  # a scalar radius is broadcast
    assert q.shape == (3, 4) and rad.dtype == np.float32 and rad.tolist() == [0.25] * 3 and rad.flags.c_contiguous
    q, rad = H.Graph._range_io(Q[0], [0.5], H.MODE_BEAM)  # one query as a vector
    assert q.shape == (1, 4) and rad.tolist() == [0.5]
    with pytest.raises(H.HnswError, match="range search supports beam and exact mode") as e:
        H.Graph._range_io(Q, 0.25, H.MODE_COMPAT)
    assert e.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match="2 radii for 3 queries") as e:
        H.Graph._range_io(Q, [0.1, 0.2], H.MODE_EXACT)
    assert e.value.code == H._lib.EINVAL
    with pytest.raises(H.HnswError, match="radii"):
        H.Graph._range_io(Q, np.zeros((3, 1)), H.MODE_EXACT)


def test_split_ragged(H):
    lims = np.array([0, 2, 2, 5], np.int64)
    keys, dist = np.arange(5) * 10, np.arange(5, dtype=np.float32)
    per = H.split_ragged(lims, keys, dist)
    assert [p[0].tolist() for p in per] == [[0, 10], [], [20, 30, 40]]
    assert [p[1].tolist() for p in per] == [[0.0, 1.0], [], [2.0, 3.0, 4.0]]
    assert [k for k in H.split_ragged(lims, list("abcde"))] == [["a", "b"], [], ["c", "d", "e"]]
    assert H.split_ragged([0], keys) == []
    for bad in ([1, 2], [0, 3, 2], []):
        with pytest.raises(ValueError):
            H.split_ragged(bad, keys)
    with pytest.raises(ValueError):
        H.split_ragged(lims, keys[:4])
