"""The batched insert where a commit drops reverse proposals: the cases and the set-valued check,
shared by test_batch_overflow.py (CPU: the check on the restatement alone) and
test_gpu_batch_overflow.py (GPU: the engine's graph is one of the valid ones).  Plain Python.

A row keeps at most inc_cap (64) of the proposals one commit sends it; which ones is decided by
arrival order, so there is no single expected graph.  A batch's searches read each layer as it
stood before that layer's commit, so everything else is determined: the batch rows' own rows
(hence every target's proposal set P), and every old row that received at most inc_cap
proposals.  For a row past the cap the valid rows are exactly { commit(old + S) : S a subset of
P, |S| = inc_cap }, and membership in that set is decidable from the row alone
(check_overflowed_batch).  What the graph cannot show -- that no more than inc_cap proposals were
kept, the extra ones being without effect -- the drop counter closes: it must equal
sum(max(0, |P| - inc_cap)).
"""
import numpy as np

from tests import batch_ref as BR

INC_CAP = 64     # the engine's slots per row and commit (index.hpp)
FULL_CAP = 4000  # the restatement run that keeps every proposal
NEXT = 100       # rows of the add that follows the overflowed batch
EFC = 64


def _case(n0, nb, d, M, m0, rules, metrics=(0, 1), **opts):
    o = dict(ef_construction=EFC)
    o.update(opts)
    return dict(n0=n0, nb=nb, d=d, M=M, m0=m0, rules=tuple(rules), metrics=tuple(metrics), opts=o)


# rules: (heuristic, keep_pruned)
CASES = {
    "heavy": _case(40, 300, 24, 8, 16, ((2, 1), (0, 0), (1, 1))),   # nearly every old row overflows
    "light": _case(200, 400, 24, 12, 24, ((2, 1), (0, 0))),         # rows with 65 .. 72 proposals: the check is tight
    "dense": _case(300, 500, 32, 32, 63, ((2, 1),), ef_construction=128),  # degree 63 + 64 slots: tot 127
    "wide": _case(40, 200, 768, 8, 16, ((2, 1),), metrics=(0,)),    # another dimension configuration
}
ALPHA_PCT = 100
# The link pass proposes to batch-mates only, so its own drops need a batch row that receives more
# than 64 link proposals: a batch 25 times the index it lands in (in the heavy case with
# batch_link 1 the restatement's link pass drops nothing under cosine).
LINK = _case(20, 500, 24, 8, 16, ((2, 1),))


def case_ids():
    return [(name, m, h, kp) for name, c in CASES.items() for m in c["metrics"] for h, kp in c["rules"]]


def mcaps_of(case):
    return [case["m0"]] + [case["M"]] * 31


def alpha_of(pct=ALPHA_PCT):
    return np.float32(pct) / np.float32(100)


def data_of(case, metric):
    """(keys, X): n0 pre-batch rows, nb batch rows, NEXT further rows"""
    gen = BR.Gen(7 + metric, case["d"])
    n = case["n0"] + case["nb"] + NEXT
    X, _ = gen.rows(n)
    return BR.keys_of(n), X


def one_batch(nb):
    return dict(batch_ratio_pct=0, batch_min=nb, batch_max=nb)


DEFAULT_SCHEDULE = dict(batch_ratio_pct=5, batch_min=1, batch_max=65536)


class Run:
    """One restatement run of a case: the n0 rows under the default schedule, then the nb rows as
    one batch (levels capped at the top layer).  levels: (pre-batch levels, batch levels), the
    engine's in the GPU test; None: the restatement's own preview."""

    def __init__(self, O, case, metric, h, kp, levels=None, inc_cap=INC_CAP, descending=False, batch_link=0):
        n0, nb = case["n0"], case["nb"]
        self.keys, self.X = data_of(case, metric)
        self.opts = dict(case["opts"], heuristic=h, keep_pruned=kp, prune_alpha_pct=ALPHA_PCT)
        self.g = g = O.Graph(metric=metric, order=O.ORDER_DEV, M=case["M"], M0=case["m0"], Ml=0.25, EfSearch=64,
                             seed=BR.RNG_SEED)
        g.set_batch_descending(descending)
        lv0 = g.preview_levels(n0) if levels is None else levels[0]
        self.cn0 = g.add_batch(self.keys[:n0], self.X[:n0], lv0, **self.opts)
        self.E0, self.D0 = g.export(), g.export_edge_dist()
        if levels is None:
            lvb = np.minimum(g.preview_levels(nb), self.E0["deg"].shape[0] - 1).astype(np.int32)
        else:
            lvb = levels[1]
        self.levels = (lv0, lvb)
        self.cn = g.add_batch(self.keys[n0:n0 + nb], self.X[n0:n0 + nb], lvb, inc_cap=inc_cap, batch_link=batch_link,
                              **one_batch(nb), **self.opts)
        self.ex, self.ed = g.export(), g.export_edge_dist()

    def add_next(self, levels=None):
        """the NEXT further rows under the default schedule -> (levels, counters)"""
        n1 = len(self.ex["keys"])
        lv = self.g.preview_levels(NEXT) if levels is None else levels
        cn = self.g.add_batch(self.keys[n1:n1 + NEXT], self.X[n1:n1 + NEXT], lv, **self.opts)
        return lv, cn


def continue_from(O, case, metric, h, kp, ex, ed):
    """a fresh restatement holding the graph (ex, ed), ready for the next add"""
    g = O.Graph(metric=metric, order=O.ORDER_DEV, M=case["M"], M0=case["m0"], Ml=0.25, EfSearch=64, seed=BR.RNG_SEED)
    g.import_graph(ex["keys"], ex["vecs"], ex["deg"], ex["adj"], ex["entry"], ex["dead"], edge_dist=ed)
    return g


# An update whose one chunk overflows: every other row of the first 2 * nu is moved next to two
# rows that stay, so those and their neighbours receive the chunk's proposals.
UPDATE = dict(n=300, nu=140, d=24, M=8, m0=16, opts=dict(ef_construction=EFC, heuristic=2, keep_pruned=1))


def update_data(metric):
    """(keys, X, updated keys, their new vectors); X holds NEXT further rows past n"""
    u = UPDATE
    gen = BR.Gen(11 + metric, u["d"])
    X, labels = gen.rows(u["n"])
    rows = np.arange(0, 2 * u["nu"], 2)
    V = gen.draw(labels[[1, 3]][np.arange(u["nu"]) % 2])
    Xn, _ = gen.rows(NEXT)
    return BR.keys_of(u["n"] + NEXT), np.concatenate([X, Xn]), BR.keys_of(u["n"])[rows], V


# ---- the checks --------------------------------------------------------------------------------

def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _row(ex, ed, l, v):
    """the row as [(distance, id)] in stored order"""
    deg = max(int(ex["deg"][l, v]), 0)
    return [(np.float32(ed[l, v, j]), int(ex["adj"][l, v, j])) for j in range(deg)]


def _rank(e):
    return (float(e[0]), e[1])


def proposals(ex, ed, n0):
    """P[l][v] = [(d(u, v), u)]: what the batch rows [n0, N) hold is what they proposed"""
    L, N = ex["deg"].shape
    P = [dict() for _ in range(L)]
    for l in range(L):
        for u in range(n0, N):
            for d, v in _row(ex, ed, l, u):
                P[l].setdefault(v, []).append((d, u))
    return P


def _pair_d(O, metric, vecs, xs, rs):
    """{(x, r): distance(x, r)}: candidate first, kept row second, as the commit evaluates it"""
    if not len(xs) or not len(rs):
        return {}
    ia = np.repeat(np.asarray(xs, np.int32), len(rs))
    ib = np.tile(np.asarray(rs, np.int32), len(xs))
    D = O.distance_pairs(metric, O.ORDER_DEV, vecs, ia, ib)
    return {(int(a), int(b)): D[i] for i, (a, b) in enumerate(zip(ia, ib))}


def commit(entries, mcap, heuristic, alpha, D, within):
    """the commit rule on [(distance, id)]: ranked by (distance, id); heuristic < 2 keeps the best
    mcap, heuristic 2 applies the diversity rule (always: the engine's commit of such a row was
    over the row's capacity whatever subset this is).  D holds d(candidate, kept row) for kept
    rows of `within` only: None as soon as the rule keeps a row outside it."""
    e = sorted(entries, key=_rank)
    if heuristic < 2:
        return e[:mcap]
    kept = []
    for d, c in e:
        if len(kept) == mcap:
            break
        if any(alpha * D[(c, r)] < d for _, r in kept):
            continue
        if c not in within:
            return None
        kept.append((d, c))
    return kept


def analyse_row(O, metric, vecs, old, prop, K, mcap, heuristic, alpha, inc_cap=INC_CAP):
    """A row past the cap: old and K as _row gives them, prop = P(l, v).  Asserts membership, own
    commit and slot count; returns (A, harmless, harmful): K's proposal sources, and the
    proposals outside K that could / could not have held a slot without changing K."""
    ids = [c for _, c in K]
    assert len(set(ids)) == len(ids), "a repeated id"
    pool = {c: d for d, c in old}
    assert not set(pool) & {u for _, u in prop}
    pool.update({u: d for d, u in prop})
    for d, c in K:
        assert c in pool, ("neither in the old row nor proposed", c)
        assert _bits(d) == _bits(pool[c]), ("distance bits", c)
    src = {u for _, u in prop}
    A = [(d, c) for d, c in K if c in src]
    assert len(A) <= inc_cap, "more proposals kept than slots"
    D = _pair_d(O, metric, vecs, sorted(pool), ids) if heuristic >= 2 else {}
    own = commit(old + A, mcap, heuristic, alpha, D, set(ids))  # (None: it kept a row that is not in K)
    assert own is not None and [(_bits(d), c) for d, c in own] == [(_bits(d), c) for d, c in K], "own commit"
    full = len(K) == mcap
    last = _rank(K[-1]) if K else None
    harmless, harmful = [], []
    inK = set(ids)
    for d, x in prop:
        if x in inK:
            continue
        ok = full and _rank((d, x)) > last
        if not ok and heuristic >= 2:
            ok = any(_rank(r) < _rank((d, x)) and alpha * D[(x, r[1])] < d for r in K)
        (harmless if ok else harmful).append((d, x))
    assert len(harmless) >= inc_cap - len(A), ("slot count", len(harmless), len(A))
    return A, harmless, harmful


def check_overflowed_batch(O, metric, E0, D0, full, got, got_d, n0, mcaps, heuristic, alpha, inc_cap=INC_CAP):
    """(got, got_d) is a valid outcome of adding the batch [n0, N) to (E0, D0) in one commit per
    layer with inc_cap slots per row; full = (export, edge distances) of the restatement that kept
    every proposal.  Returns dict(dropped, rows, light, tot_max): the drops the counter must show,
    the (layer, row) past the cap, those of layer 0 with 65 .. 72 proposals, and the largest commit."""
    fx, fd = full
    for f in ("keys", "entry", "dead"):
        assert np.array_equal(got[f], fx[f]), f
    assert got["deg"].shape == fx["deg"].shape and got["adj"].shape == fx["adj"].shape
    assert np.array_equal(got["vecs"].view(np.uint32), fx["vecs"].view(np.uint32))
    L, N = got["deg"].shape
    gb, fb = got_d.view(np.uint32), fd.view(np.uint32)
    # batch rows
    assert np.array_equal(got["deg"][:, n0:], fx["deg"][:, n0:]), "a batch row's degree"
    assert np.array_equal(got["adj"][:, n0:], fx["adj"][:, n0:]), "a batch row's neighbours"
    assert np.array_equal(gb[:, n0:], fb[:, n0:]), "a batch row's distances"
    P = proposals(got, got_d, n0)
    info = dict(dropped=0, rows=[], light=[], tot_max=0)
    for l in range(L):  # the rows past the cap
        assert all(0 <= v < n0 for v in P[l]), "a batch row proposed to a batch row"
        for v in range(n0):
            prop = P[l].get(v, [])
            if len(prop) <= inc_cap:
                continue
            old = _row(E0, D0, l, v)
            try:
                analyse_row(O, metric, got["vecs"], old, prop, _row(got, got_d, l, v), mcaps[l], heuristic, alpha,
                            inc_cap)
            except AssertionError as e:
                raise AssertionError(("layer", l, "row", v, "proposals", len(prop)) + e.args) from None
            info["dropped"] += len(prop) - inc_cap
            info["rows"].append((l, v))
            info["tot_max"] = max(info["tot_max"], len(old) + inc_cap)
            if l == 0 and inc_cap < len(prop) <= inc_cap + 8:
                info["light"].append(v)
    for l in range(L):  # within the cap, or untouched
        for v in range(n0):
            if len(P[l].get(v, [])) <= inc_cap:
                assert got["deg"][l, v] == fx["deg"][l, v], ("within the cap: degree", l, v)
                assert np.array_equal(got["adj"][l, v], fx["adj"][l, v]), ("within the cap: neighbours", l, v)
                assert np.array_equal(gb[l, v], fb[l, v]), ("within the cap: distances", l, v)
    return info


def check_well_formed(O, metric, ex, ed, mcaps):
    """every live member row of every layer: 0 <= deg <= mcap; ids in range, live, members of the
    layer, not the row itself, none repeated; every stored distance has the bits of the pair's
    distance"""
    L, N = ex["deg"].shape
    dead = ex["dead"].astype(bool)
    for l in range(L):
        rows = np.flatnonzero((ex["deg"][l] != -2) & ~dead)
        deg = ex["deg"][l][rows]
        assert ((deg >= 0) & (deg <= mcaps[l])).all(), ("degree", l)
        slot = np.arange(ex["adj"].shape[2])[None, :] < deg[:, None]
        src = rows[np.nonzero(slot)[0]]
        dst = ex["adj"][l][rows][slot]
        assert ((dst >= 0) & (dst < N)).all(), ("id out of range", l)
        assert not dead[dst].any(), ("edge to a deleted row", l)
        assert (ex["deg"][l][dst] >= 0).all(), ("edge to a row outside the layer", l)
        assert (src != dst).all(), ("self-loop", l)
        pair = src.astype(np.int64) * N + dst
        assert len(np.unique(pair)) == len(pair), ("repeated id", l)
        want = O.distance_pairs(metric, O.ORDER_DEV, ex["vecs"], src, dst)
        assert np.array_equal(want.view(np.uint32), ed[l][rows][slot].view(np.uint32)), ("distance bits", l)
