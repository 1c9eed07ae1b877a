"""Hand-built one-layer graphs on which a layer-0 beam step flushes its merge
buffer more than once (device_search.hpp beam_layer MERGE / bl_merge), and a
plain restatement of that step batching.

The search meets the rows in a fixed order, a staircase of ever better groups:

    E (the entry)  ->  A_0..A_{W-1}
    the XW best rows of every fill level  ->  the next, better fill level
    P_0, P_1 (the two best rows of the last fill level)  ->  G1, G2
    the best row of G2  ->  the bait Z (better than every other row)

E, A and the fill levels hold ef + 1 rows, so the list is full, E is out, and
its W worst entries are the A rows when the *critical step* expands P_0 and
P_1 together (XW >= 2).  Their groups do not share a batch (2 W > 64): G1, W
rows better than everything listed, is flushed first and evicts every A row.
G2 lies between the worst entry left and the best A row: each of its rows beat
the worst entry before the step (the only test the step applies while it
collects candidates) and none beats the worst entry after G1's flush.  The
right list never holds a G2 row, so the bait behind G2's best row is never
reached; a merge that places the buffer's best row on the last entry instead
of dropping it expands that row later and returns the bait first.

Every row lies on a line (Euclidean: (origin + p, 0, 0, 0), the query at
`origin`, distance exactly p) or on an arc (cosine: angle 0.3 + p * 1.2 / 4096
from the query, scaled row by row), with one integer position p per row, so the
distances are distinct and bl_merge stays on its fast path.  `bad` > 0 adds
rows whose distance is not finite to the first fill step (Euclidean: squares
that overflow, +INF; cosine: zero rows, NaN), while the list is not yet full.

Ids are shuffled, so neither ids nor keys follow the distances.
"""
import numpy as np

EUCLIDEAN, COSINE = 1, 0
DIM = 4
INF = float("inf")


def staircase(ef, xw, metric, width=64, bad=0, origin=0.0, seed=0):
    """-> dict(graph=<import_graph arguments>, query=<[DIM] f32>, info=<dict>).

    info: ids of E, A, the fill `levels` (levels[0] is A), P (the rows the
    critical step expands first: P[0] -> G1, P[1] -> G2), G1, G2, g2_best (the
    only row adjacent to the bait), Z (the bait), bad (rows with a non-finite
    distance), and pos (id -> position p, -1 for the bad rows)."""
    assert 64 < ef <= 512 and xw in (1, 2, 4) and 33 <= width <= 64 and 0 <= bad <= 16
    assert width < ef
    cap = min(width, 64 - bad)  # new rows per expanded fill row
    adj, pos = {}, {}
    count = [0]

    def new(n):
        ids = list(range(count[0], count[0] + n))
        count[0] += n
        return ids

    (E,) = new(1)
    A = new(width)
    adj[E] = list(A)
    levels = [A]
    rest = ef - width  # E + A + the fill levels: ef + 1 rows
    sizes = []
    while rest > 0:
        sizes.append(min(rest, xw * cap))
        rest -= sizes[-1]
    if sizes[-1] < 2:  # (the last level holds P_0 and P_1)
        sizes[-2] -= 2 - sizes[-1]
        sizes[-1] = 2
    for n in sizes:
        parents = levels[-1][:xw]
        assert len(parents) == xw
        base, extra = divmod(n, len(parents))
        lvl = []
        for i, p in enumerate(parents):
            kids = new(base + (1 if i < extra else 0))
            lvl += kids
            adj[p] = kids[::-1] if i % 2 else list(kids)  # (rows are not in distance order)
        levels.append(lvl)
    assert len(levels[-1]) >= 2, "the last fill level needs two rows (P_0, P_1)"
    P = levels[-1][:2]
    G1, G2, (Z,) = new(width), new(width), new(1)
    mix = [(j * 37 + 5) % width for j in range(width)]  # (37 is coprime to 63 and 64)
    adj[P[0]] = [G1[j] for j in mix]
    adj[P[1]] = [G2[j] for j in mix]
    adj[G2[0]] = [Z]
    B = []
    for i, p in enumerate(levels[0][:xw]):  # the first fill step also meets the bad rows
        b = new(bad)
        B += b
        row = adj[p]
        for j, v in enumerate(b):
            row.insert(min(len(row), (5 * j + 2 * i) % (len(row) + 1)), v)
        assert len(row) <= 64

    # positions: Z 1, G1 100.., the fill levels from the last (best) one at 500,
    # 208 apart, G2 and A above the first fill level, E above A
    pos[Z] = 1
    for j, v in enumerate(G1):
        pos[v] = 100 + j
    r = 500
    for lvl in reversed(levels[1:]):
        for v in lvl:
            pos[v] = r
            r += 1
        r += 208
    top = r - 208  # one past the first fill level's worst row
    for j, v in enumerate(G2):
        pos[v] = top + 108 + j
    for j, v in enumerate(A):
        pos[v] = top + 208 + j
    pos[E] = top + 208 + width + 36
    assert top + 108 + width <= top + 208 and pos[E] < 4096
    for v in B:
        pos[v] = -1

    N = count[0]
    perm = np.random.default_rng(1000 + seed).permutation(N)  # old id -> new id
    vecs = np.zeros((N, DIM), np.float32)
    for v in range(N):
        p = pos[v]
        if metric == EUCLIDEAN:
            vecs[perm[v], 0] = origin + p if p >= 0 else 3e19 * (1.0 + (v % 16) / 16.0)
        elif p >= 0:
            th = 0.3 + p * (1.2 / 4096)
            s = 0.5 + (p % 7) * 0.25
            vecs[perm[v], 0] = s * np.cos(th)
            vecs[perm[v], 1] = s * np.sin(th)
    query = np.zeros(DIM, np.float32)
    query[0] = origin if metric == EUCLIDEAN else 1.0
    deg = np.zeros((1, N), np.int32)
    adja = np.full((1, N, 64), -1, np.int32)
    for v, row in adj.items():
        deg[0, perm[v]] = len(row)
        adja[0, perm[v], : len(row)] = [perm[u] for u in row]
    graph = dict(keys=perm_keys(N), vecs=vecs, deg=deg, adj=adja, entry=np.array([perm[E]], np.int32))
    m = lambda ids: [int(perm[v]) for v in ids]
    info = dict(E=int(perm[E]), A=m(A), levels=[m(l) for l in levels], P=m(P), G1=m(G1), G2=m(G2),
                g2_best=int(perm[G2[0]]), Z=int(perm[Z]), bad=m(B), pos={int(perm[v]): p for v, p in pos.items()},
                ef=ef, xw=xw, metric=metric, width=width)
    return dict(graph=graph, query=query, info=info)


def perm_keys(n):
    """keys that are neither the ids nor in their order"""
    return ((np.arange(n, dtype=np.int64) * 7919) % 10007) * 3 + 2


def _lt(d1, i1, d2, i2):
    return d1 < d2 or (d1 == d2 and i1 < i2)


def _insert(lst, ef, d, u):
    """bl_insert / the oracle's beam_insert: keeps the best ef by (distance, id)"""
    if d != d:
        return
    if len(lst) == ef and not _lt(d, u, lst[-1][0], lst[-1][1]):
        return
    if any(e[1] == u for e in lst):
        return
    p = 0
    while p < len(lst) and _lt(lst[p][0], lst[p][1], d, u):
        p += 1
    lst.insert(p, [d, u, False])
    del lst[ef:]


def restate(graph, dist, ef, xw):
    """The layer-0 search of beam_layer<MERGE> in plain Python: per step the XW
    first unexpanded entries are marked, their unvisited neighbours gathered row
    by row (rows share a batch while they fit 64), each batch's candidates that
    beat the worst entry *before the step* go to a buffer of 64, the buffer is
    flushed into the list when the next batch might not fit (bk + cnt > 64) and
    at the end of the step.  A flush is one bl_insert per candidate: bl_merge is
    not restated, only when it runs and on what.

    dist: the f32 distance of every row to the query.
    -> (list of [distance, id, expanded], expansions, steps); steps[i] =
    dict(cur, full_before, worst_before, flushes=[dict(ids, worst_after)])."""
    deg, adj = graph["deg"][0], graph["adj"][0]
    entry = int(graph["entry"][0])
    lst, visited, steps, nx = [], {entry}, [], 0
    _insert(lst, ef, float(dist[entry]), entry)
    while True:
        cur = []
        for e in lst:
            if len(cur) == xw:
                break
            if not e[2]:
                e[2] = True
                cur.append(e[1])
        if not cur:
            break
        nx += len(cur)
        batches = []
        for c in cur:
            new = []
            for v in adj[c, : deg[c]].tolist():
                if v >= 0 and v not in visited:
                    visited.add(v)
                    new.append(v)
            batches.append(new)
        b = 0
        for w in range(1, len(batches)):
            if len(batches[b]) + len(batches[w]) <= 64:
                batches[b] = batches[b] + batches[w]
                batches[w] = []
            else:
                b = w
        full = len(lst) == ef
        wd, wi = (lst[-1][0], lst[-1][1]) if full else (INF, 0x7FFFFFFF)
        step = dict(cur=cur, full_before=full, worst_before=wd, flushes=[])

        def flush(buf):
            for v in buf:
                _insert(lst, ef, float(dist[v]), v)
            step["flushes"].append(dict(ids=list(buf), worst_after=lst[-1][0] if len(lst) == ef else INF))

        buf = []
        for batch in batches:
            if not batch:
                continue
            if len(buf) + len(batch) > 64:
                flush(buf)
                buf = []
            buf += [v for v in batch if _lt(float(dist[v]), v, wd, wi)]
        if buf:
            flush(buf)
        steps.append(step)
    return lst, nx, steps


def oracle_graph(O, s):
    o = O.Graph(metric=s["info"]["metric"], order=O.ORDER_DEV, M=32, M0=63, Ml=0.25, EfSearch=64)
    o.import_graph(**s["graph"])
    return o


def oracle_list(O, o, s, k=None):
    """(keys, distances, count, expansions) of the oracle's search at k = ef"""
    ef, xw = s["info"]["ef"], s["info"]["xw"]
    o.set_search_expand(xw)
    x0 = o.stats()[1]
    rk, rd, rn = o.search(s["query"], k or ef, mode=O.MODE_BEAM, ef=ef)
    o.set_search_expand(1)
    return rk, rd, rn, o.stats()[1] - x0
