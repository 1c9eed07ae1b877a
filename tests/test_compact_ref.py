"""CPU: the compaction's yardstick and host surfaces.  compact_export (tests/compact_ref.py)
is pinned to the oracle: a graph with deleted rows and its compacted import return the same
lists in every search mode, because the map is monotone and every list is ordered by
(distance, row id).  And include/mhnsw.h declares mhnsw_compact, hnsw_amd._lib binds it and
the Python hosts expose it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import compact_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("metric", [0, 1])
def test_compacted_import_searches_identically(O, metric, seed):
    rng = np.random.default_rng(100 * seed + metric)
    n, d = 1500, 24
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[700] = X[20]  # three identical rows: ties in distance are broken by row id
    X[1400] = X[20]
    Q = np.concatenate([rng.normal(size=(40, d)).astype(np.float32), X[[20, 333]]])
    keys = np.arange(n, dtype=np.int64) * 7 + 3
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64, seed=seed)
    o.add(keys, X)
    gone = rng.permutation(n)[:455]
    gone = gone[(gone != 20) & (gone != 1400)]  # row 700 may go: the tie then spans the gap
    assert o.delete(keys[gone], mode=1) == [True] * len(gone)
    ex = o.export()
    assert int(ex["dead"].sum()) == len(gone)
    cx, dangling = CR.compact_export(ex)
    assert dangling == 0  # the batched repair leaves no live row pointing at a dead one
    assert len(cx["keys"]) == n - len(gone) and not cx["dead"].any()
    c = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64, seed=seed)
    c.import_graph(**cx)
    assert len(c) == len(o) == n - len(gone) and c.topography() == o.topography()
    for mode, k, ef in ((O.MODE_BEAM, 10, 64), (O.MODE_BEAM, 64, 64), (O.MODE_EXACT, 10, 0), (O.MODE_EXACT, 300, 0)):
        CR.same_lists(o.search(Q, k, mode=mode, ef=ef), c.search(Q, k, mode=mode, ef=ef))
    # compacting again changes nothing
    cx2, dangling = CR.compact_export(c.export())
    assert dangling == 0
    CR.same_export(cx2, c.export())


def test_compact_export_drops_dangling_edges():
    ex = dict(keys=np.array([10, 11, 12, 13]), vecs=np.arange(8, dtype=np.float32).reshape(4, 2),
              deg=np.array([[2, 1, 3, 1], [-2, -2, 0, -2]], np.int32),
              adj=np.array([[[1, 2, -1], [0, -1, -1], [0, 1, 3], [2, -1, -1]], [[-1] * 3] * 4], np.int32),
              entry=np.array([0, 2], np.int32), dead=np.array([0, 1, 0, 0], np.uint8))
    cx, dangling = CR.compact_export(ex)
    assert dangling == 2
    assert cx["keys"].tolist() == [10, 12, 13] and cx["entry"].tolist() == [0, 1]
    assert cx["deg"].tolist() == [[1, 2, 1], [-2, 0, -2]]
    assert cx["adj"][0].tolist() == [[1, -1, -1], [0, 2, -1], [1, -1, -1]]
    assert CR.new_ids(ex["dead"]).tolist() == [0, -1, 1, 2]


def test_header_declares_and_hosts_bind(H):
    src = open(os.path.join(ROOT, "include", "mhnsw.h")).read()
    m = re.search(r"\bint\s+mhnsw_compact\s*\(([^;]*)\)\s*;", src)
    assert m, "mhnsw_compact is not declared in include/mhnsw.h"
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["h", "out_removed"]
    res, sig = H.SIGNATURES["mhnsw_compact"]
    assert res is C.c_int and sig == [C.c_void_p, C.POINTER(C.c_int64)]
    assert hasattr(H.load(), "mhnsw_compact")
    for fn in (H.Graph.Compact, H.ExactIndex.Compact):
        assert list(inspect.signature(fn).parameters) == ["self"]
    shim = open(os.path.join(ROOT, "include", "hnsw_amd", "graph.hpp")).read()
    assert re.search(r"std::pair<int64_t, Error>\s+Compact\(\)", shim)
