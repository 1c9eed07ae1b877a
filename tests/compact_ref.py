"""TEST INFRASTRUCTURE ONLY -- what mhnsw_compact must leave behind, restated in numpy
on the CSR export (Graph.export / oracle.Graph.export): the export of a compacted handle
is compact_export(the export before).  tests/test_compact_ref.py pins it to the oracle
(every search over the compacted import returns what the uncompacted graph returned), and
the GPU tests compare the engine against it."""
import numpy as np


def new_ids(dead) -> np.ndarray:
    """new(i): the live rows below row i, -1 for a dead row (monotone on the live rows)."""
    live = ~np.asarray(dead).astype(bool)
    new = np.cumsum(live) - 1
    new[~live] = -1
    return new.astype(np.int64)


def compact_export(ex: dict):
    """-> (export, dangling): the dead rows removed, every id of adj and entry through
    new(), the order inside each adjacency row kept, dead all zero.  An edge to a dead row
    is dropped (the row closes up, its degree shrinks) and counted in `dangling`."""
    dead = np.asarray(ex["dead"]).astype(bool)
    new = new_ids(dead)
    live = np.flatnonzero(~dead)
    L = ex["deg"].shape[0]
    cap = ex["adj"].shape[2]
    deg = np.ascontiguousarray(ex["deg"][:, live])
    adj = np.full((L, len(live), cap), -1, np.int32)
    dangling = 0
    for l in range(L):
        for j, i in enumerate(live):
            d = int(ex["deg"][l, i])
            if d <= 0:
                continue
            row = new[ex["adj"][l, i, :d]]
            kept = row[row >= 0]
            dangling += d - len(kept)
            adj[l, j, : len(kept)] = kept
            deg[l, j] = len(kept)
    entry = np.array([new[e] if e >= 0 else -1 for e in ex["entry"]], np.int32)
    out = dict(keys=ex["keys"][live].copy(), vecs=ex["vecs"][live].copy(), deg=deg, adj=adj, entry=entry,
               dead=np.zeros(len(live), np.uint8))
    return out, dangling


def same_export(a: dict, b: dict):
    """Field by field, vectors by their bits; adjacency rows up to their degree, in order."""
    assert np.array_equal(a["keys"], b["keys"]), "keys"
    assert a["vecs"].shape == b["vecs"].shape and np.array_equal(
        np.ascontiguousarray(a["vecs"], np.float32).view(np.uint32),
        np.ascontiguousarray(b["vecs"], np.float32).view(np.uint32)), "vector bits"
    assert np.array_equal(a["deg"], b["deg"]), "degrees"
    assert np.array_equal(a["entry"], b["entry"]), ("entry", a["entry"], b["entry"])
    assert np.array_equal(a["dead"], b["dead"]), "dead"
    cap = min(a["adj"].shape[2], b["adj"].shape[2])
    assert int(a["deg"].max(initial=0)) <= cap
    mask = np.arange(cap)[None, None, :] < np.maximum(a["deg"], 0)[:, :, None]
    assert np.array_equal(np.where(mask, a["adj"][:, :, :cap], -1), np.where(mask, b["adj"][:, :, :cap], -1)), "adj"


def same_lists(a, b):
    """(keys, distances, counts) of two searches: the same keys, distance bits and counts."""
    ak, ad, an = a
    bk, bd, bn = b
    assert np.array_equal(an, bn), "counts"
    for q in range(len(an)):
        n = an[q]
        assert ak[q, :n].tolist() == bk[q, :n].tolist(), ("keys of query", q)
        x, y = np.asarray(ad[q, :n], np.float32), np.asarray(bd[q, :n], np.float32)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(
            x[~np.isnan(x)].view(np.uint32), y[~np.isnan(y)].view(np.uint32)), ("distance bits of query", q)
