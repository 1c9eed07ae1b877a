"""The filtered beam search restated in plain Python (DESIGN.md "Filtered
search"; the engine's kernel is beam.hpp k_search_beam_filt).

All comparisons are the engine's (distance, id) order; distances are the
canonical f32 ones, handed in as a table, and NaN is never offered to a list.

A filtered query has an allow-set A (rows whose filter bit is set and that are
not deleted), a route width W and a result width E = max(ef, k) <= W.  The
descent through the upper layers is the unfiltered one.  Layer 0:

    L: sorted list, capacity W, with expanded marks.  R: sorted list of rows in A, capacity E.
    init: the entry p goes to L; also to R when p in A.
    loop:
      c = first unexpanded entry of L; none -> stop
      if |R| == E and R[E-1] < c (strictly): stop
      mark c expanded (one expansion)
      BL = L[W-1] if |L| == W else +inf;  BR = R[E-1] if |R| == E else +inf   (BEFORE the step)
      every layer-0 neighbour v of c not yet visited (now visited), e = (d(v), v), d not NaN:
          offered  iff  e < BL and e < BR
      every offered row goes to L (L keeps its best W); every offered row in A also to R (its best E)
    result: the first k entries of R

The graph is an export (`deg` [L, N], `adj` [L, N, cap], `entry` [L], `dead`
[N]); a query is its row of the distance table (distance_table: the oracle's
ORDER_DEV distances, bit for bit).
"""
import bisect

import numpy as np

INF = float("inf")
NOID = 0x7FFFFFFF  # the id of an empty list slot: +inf bounds compare as (inf, NOID)


def distance_table(O, export, metric, Q):
    """[B, N] float32: the canonical distance of every query to every row, by
    row id -- an exact search with k = N on a copy of the graph imported with
    the dead flags cleared; rows missing from its list (NaN distances) are NaN."""
    N = len(export["keys"])
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64)
    o.import_graph(export["keys"], export["vecs"], export["deg"], export["adj"], export["entry"],
                   np.zeros(N, np.uint8))
    keys, dist, n = o.search(Q, N, mode=O.MODE_EXACT)
    row_of = {int(k): i for i, k in enumerate(export["keys"])}
    assert len(row_of) == N, "the table maps keys to rows: keys must be unique"
    T = np.full((len(Q), N), np.nan, np.float32)
    for b in range(len(Q)):
        rows = np.fromiter((row_of[int(x)] for x in keys[b, : n[b]]), np.int64, n[b])
        T[b, rows] = dist[b, : n[b]]
    return T


class Graph:
    """an export, as plain lists (the walks below are scalar Python)"""

    def __init__(self, export):
        deg = np.asarray(export["deg"])
        adj = np.asarray(export["adj"])
        self.L, self.N = deg.shape
        self.deg = deg
        self.nbrs = [[[int(v) for v in adj[l, i, : max(int(deg[l, i]), 0)] if v >= 0] if deg[l, i] > 0 else []
                      for i in range(self.N)] if (deg[l] > 0).any() else None for l in range(self.L)]
        self.entry = [int(e) for e in export["entry"]]
        self.dead = np.asarray(export["dead"]).astype(bool)
        live = [l for l in range(self.L) if self.entry[l] >= 0]
        self.top = max(live) if live else -1

    def row(self, l, c):
        return self.nbrs[l][c] if self.nbrs[l] is not None else []


def _offer(lst, cap, e):
    """the list keeps the best `cap` of itself and e (the exact visited set of
    the walks below offers a row once, so no id is listed twice)"""
    if len(lst) == cap and not e < lst[-1]:
        return
    bisect.insort(lst, e)
    if len(lst) > cap:
        lst.pop()


def _plain_layer(g, l, p, ef, d):
    """the unfiltered sorted-list search of one layer -> (list, expansions)"""
    lst, done, seen, nx = [], set(), {p}, 0
    if d[p] == d[p]:
        lst.append((d[p], p))
    while True:
        c = next((e for e in lst if e[1] not in done), None)
        if c is None:
            return lst, nx
        done.add(c[1])
        nx += 1
        for v in g.row(l, c[1]):
            if v in seen:
                continue
            seen.add(v)
            if d[v] == d[v]:
                _offer(lst, ef, (d[v], v))


def descend(g, d, upper_ef=1):
    """the unfiltered descent through the upper layers -> (the layer-0 entry, expansions)"""
    nx = 0
    p = g.entry[g.top]
    for l in range(g.top, 0, -1):
        if g.deg[l, p] == -2:
            if g.entry[l] < 0:
                continue
            p = g.entry[l]
        lst, x = _plain_layer(g, l, p, upper_ef, d)
        nx += x
        if lst:
            p = lst[0][1]
    if g.deg[0, p] == -2:
        p = g.entry[0]
    return p, nx


def search(g, dist, allow, k, ef, route, upper_ef=1, arrival=None):
    """One query.  dist: its row of the distance table; allow: bool [N] (None:
    every row), deleted rows are never in A; arrival: None, or f(list) that
    reorders (and may repeat) a step's neighbours in place -- the results do not
    depend on it.  -> (ids, distances, expansions), at most k results."""
    d = np.asarray(dist, np.float32).tolist()
    E = max(ef, k)
    W = max(route, E)
    if g.top < 0:
        return [], [], 0
    in_a = (~g.dead) if allow is None else (np.asarray(allow, bool) & ~g.dead)
    p, nx = descend(g, d, upper_ef)
    L, R, done, seen = [], [], set(), {p}
    if d[p] == d[p]:
        L.append((d[p], p))
        if in_a[p]:
            R.append((d[p], p))
    pos = 0  # every entry of L below pos is expanded
    while True:
        while pos < len(L) and L[pos][1] in done:
            pos += 1
        if pos == len(L):
            break
        c = L[pos]
        if len(R) == E and R[-1] < c:
            break
        done.add(c[1])
        nx += 1
        bl = L[-1] if len(L) == W else (INF, NOID)
        br = R[-1] if len(R) == E else (INF, NOID)
        nb = list(g.row(0, c[1]))
        if arrival is not None:
            arrival(nb)
        offered = []
        for v in nb:
            if v in seen:
                continue
            seen.add(v)
            e = (d[v], v)
            if e[0] == e[0] and e < bl and e < br:
                offered.append(e)
        for e in offered:
            _offer(L, W, e)
            i = bisect.bisect_left(L, e)
            if i < len(L) and L[i] == e:  # (listed: unexpanded, and the entries above it moved up)
                pos = min(pos, i)
            if in_a[e[1]]:
                _offer(R, E, e)
    out = R[:k]
    return [e[1] for e in out], [e[0] for e in out], nx


def search_batch(g, table, allow_of, keys, k, ef, route, **kw):
    """The batch form, shaped like the engine's outputs: (keys int64 [B, k],
    dist float32 [B, k], n int32 [B], expansions).  allow_of[b]: query b's
    allow mask, or None."""
    B = len(table)
    ok = np.full((B, k), -1, np.int64)
    od = np.full((B, k), np.inf, np.float32)
    on = np.zeros(B, np.int32)
    nx = 0
    for b in range(B):
        ids, ds, x = search(g, table[b], allow_of[b], k, ef, route, **kw)
        on[b] = len(ids)
        ok[b, : len(ids)] = [keys[i] for i in ids]
        od[b, : len(ids)] = ds
        nx += x
    return ok, od, on, nx
