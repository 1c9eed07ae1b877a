"""CPU: the set-valued check of a batch that drops reverse proposals (tests/overflow_ref.py), on
the restatement alone.

1. Every case reaches what it is there for: the batch drops proposals, the pre-batch add dropped
   none, the light case has layer-0 rows with 65 .. 72 proposals, the dense case a commit of
   63 + 64 = 127 entries.
2. The restatement at inc_cap 64 taken in ascending and in descending order are two arrival
   orders: both pass the check, their graphs differ, and the check's drop count is the counter's.
3. The check rejects what is no valid commit: the same build with 48 slots, a kept proposal
   swapped for a dropped one that matters, a flipped distance bit, a repeated id, an altered batch
   row.
4. Graph.import_graph(edge_dist=): an imported overflowed graph continues the build bit for bit.
5. The link pass and the update reach the drop on the restatement (the conditions of
   test_gpu_batch_overflow.test_link_and_update_overflow).
"""
import copy

import numpy as np
import pytest

from tests import batch_ref as BR
from tests import overflow_ref as OR


@pytest.fixture(scope="module")
def runs(O):
    """(full, ascending) restatement runs per case, built once and left unchanged"""
    cache = {}

    def get(name, metric, h, kp):
        key = (name, metric, h, kp)
        if key not in cache:
            case = OR.CASES[name]
            cache[key] = (OR.Run(O, case, metric, h, kp, inc_cap=OR.FULL_CAP), OR.Run(O, case, metric, h, kp))
        return cache[key]

    return get


def _check(O, name, metric, h, full, r, ex=None, ed=None):
    case = OR.CASES[name]
    return OR.check_overflowed_batch(O, metric, r.E0, r.D0, (full.ex, full.ed), r.ex if ex is None else ex,
                                     r.ed if ed is None else ed, case["n0"], OR.mcaps_of(case), h, OR.alpha_of())


@pytest.mark.parametrize("name,metric,h,kp", OR.case_ids())
def test_both_arrival_orders_are_valid(O, runs, name, metric, h, kp):
    case = OR.CASES[name]
    full, asc = runs(name, metric, h, kp)
    desc = OR.Run(O, case, metric, h, kp, descending=True)
    assert full.cn["dropped_proposals"] == 0
    infos = []
    for r in (asc, desc):
        assert r.cn0["dropped_proposals"] == 0  # the pre-batch add
        assert r.cn["batches"] == 1 and r.cn["dropped_proposals"] > 0
        BR.same_export(r.E0, full.E0, r.D0, full.D0)
        OR.check_well_formed(O, metric, r.ex, r.ed, OR.mcaps_of(case))
        info = _check(O, name, metric, h, full, r)
        assert info["dropped"] == r.cn["dropped_proposals"]
        infos.append(info)
    assert infos[0] == infos[1]
    print(name, metric, h, kp, "dropped", infos[0]["dropped"], "rows past the cap", len(infos[0]["rows"]),
          "light", len(infos[0]["light"]), "largest commit", infos[0]["tot_max"])
    assert not np.array_equal(asc.ex["adj"], desc.ex["adj"])  # two different valid graphs
    if name == "light":
        assert infos[0]["light"]
    if name == "dense":
        assert infos[0]["tot_max"] == 127
    _check(O, name, metric, h, full, full)  # (nothing past the cap at 4000 slots: the plain comparison)


TIGHT = [i for i in OR.case_ids() if i[0] in ("heavy", "light")]


@pytest.mark.parametrize("name,metric,h,kp", TIGHT)
def test_fewer_slots_rejected(O, runs, name, metric, h, kp):
    """the same build with 48 slots per row is no valid commit at 64: a row past the cap kept too
    few (slot count, or a commit that more proposals would have changed), or a row that received
    49 .. 64 proposals lost some (where every row past the cap has harmless proposals to spare,
    as in the heavy case under cosine, only these rows can show it)"""
    full, _ = runs(name, metric, h, kp)
    r48 = OR.Run(O, OR.CASES[name], metric, h, kp, inc_cap=48)
    with pytest.raises(AssertionError, match="slot count|own commit|within the cap"):
        _check(O, name, metric, h, full, r48)


def _overflowed(O, name, metric, h, full, r):
    """(l, v, old, prop, K, A, harmless, harmful) of every row past the cap"""
    case = OR.CASES[name]
    P = OR.proposals(r.ex, r.ed, case["n0"])
    for l, v in _check(O, name, metric, h, full, r)["rows"]:
        old, K = OR._row(r.E0, r.D0, l, v), OR._row(r.ex, r.ed, l, v)
        A, harmless, harmful = OR.analyse_row(O, metric, r.ex["vecs"], old, P[l][v], K, OR.mcaps_of(case)[l], h,
                                              OR.alpha_of())
        yield l, v, old, P[l][v], K, A, harmless, harmful


@pytest.mark.parametrize("name,metric,h,kp", TIGHT)
def test_mutations_rejected(O, runs, name, metric, h, kp):
    case = OR.CASES[name]
    full, asc = runs(name, metric, h, kp)
    rows = list(_overflowed(O, name, metric, h, full, asc))

    def mutated():
        return copy.deepcopy(asc.ex), asc.ed.copy()

    def rejected(ex, ed, why):  # why: the rule of the check that the mutation breaks
        with pytest.raises(AssertionError, match=why):
            _check(O, name, metric, h, full, asc, ex, ed)

    # A kept proposal source swapped, in its place, for a dropped one that is not harmless.  (Which
    # proposals arrive first is free, so the swap can be the commit of another subset, and then it
    # is valid: with heuristic < 2 it always is once the row is put back in rank order, which is
    # asserted below.  The pair taken here leaves the row out of rank order.)
    def out_of_order(K, j, x):
        return (j > 0 and OR._rank(x) < OR._rank(K[j - 1])) or (j + 1 < len(K) and OR._rank(x) > OR._rank(K[j + 1]))

    l, v, K, j, x = next((l, v, K, j, x) for l, v, _, _, K, A, _, harmful in rows for a in A for x in harmful
                         for j in [K.index(a)] if out_of_order(K, j, x))
    ex, ed = mutated()
    ex["adj"][l, v, j], ed[l, v, j] = x[1], x[0]
    rejected(ex, ed, "own commit")
    if h < 2:
        K2 = sorted(K[:j] + K[j + 1:] + [x], key=OR._rank)
        ex["adj"][l, v, :len(K2)], ed[l, v, :len(K2)] = [c for _, c in K2], [d for d, _ in K2]
        _check(O, name, metric, h, full, asc, ex, ed)
    # one flipped bit in a stored distance of an overflowed row
    l, v = rows[0][:2]
    ex, ed = mutated()
    ed.view(np.uint32)[l, v, 0] ^= 1
    rejected(ex, ed, "distance bits")
    # a repeated id
    ex, ed = mutated()
    assert ex["deg"][l, v] >= 2
    ex["adj"][l, v, 1], ed[l, v, 1] = ex["adj"][l, v, 0], ed[l, v, 0]
    rejected(ex, ed, "a repeated id")
    # an altered batch row: two entries exchanged (still a well-formed row)
    u = next(u for u in range(case["n0"], len(asc.ex["keys"])) if asc.ex["deg"][0, u] >= 2)
    ex, ed = mutated()
    ex["adj"][0, u, [0, 1]], ed[0, u, [0, 1]] = ex["adj"][0, u, [1, 0]], ed[0, u, [1, 0]]
    OR.check_well_formed(O, metric, ex, ed, OR.mcaps_of(case))
    rejected(ex, ed, "a batch row's neighbours")


@pytest.mark.parametrize("name,metric,h,kp", [i for i in OR.case_ids() if i[2] == 2 and i[0] != "dense"])
def test_import_edge_dist_continues_the_build(O, runs, name, metric, h, kp):
    """an overflowed graph exported and imported into a fresh restatement: the next add gives
    the same graph on both, bit for bit, and drops nothing"""
    case = OR.CASES[name]
    a = OR.Run(O, case, metric, h, kp)
    b = OR.continue_from(O, case, metric, h, kp, a.ex, a.ed)
    BR.same_export(a.ex, b.export(), a.ed, b.export_edge_dist())
    lv, cn = a.add_next()
    n1 = case["n0"] + case["nb"]
    cnb = b.add_batch(a.keys[n1:n1 + OR.NEXT], a.X[n1:n1 + OR.NEXT], lv, **a.opts)
    assert cn["dropped_proposals"] == 0 and cn == cnb and cn["batches"] > 1
    BR.same_export(a.g.export(), b.export(), a.g.export_edge_dist(), b.export_edge_dist(), what=name)
    # without the distances the import is not enough: the next commits rank old rows by them
    c = O.Graph(metric=metric, order=O.ORDER_DEV, M=case["M"], M0=case["m0"], Ml=0.25, EfSearch=64, seed=BR.RNG_SEED)
    c.import_graph(a.ex["keys"], a.ex["vecs"], a.ex["deg"], a.ex["adj"], a.ex["entry"], a.ex["dead"])
    assert not c.export_edge_dist().any()


@pytest.mark.parametrize("metric", [0, 1])
def test_link_and_update_reach_the_drop(O, metric):
    """The conditions of the GPU test of the other two writers of the slots.  The insert phase of
    a layer does not read what the link pass of the layers above wrote, so the drops of a run
    with the link pass less those of the same run without it are the link pass's own: in the heavy
    case they may be 0 (link proposals go to batch-mates only), in OR.LINK they are not, in either
    arrival order."""
    heavy = OR.CASES["heavy"]
    r = OR.Run(O, heavy, metric, 2, 1, batch_link=1)
    assert r.cn["dropped_proposals"] >= OR.Run(O, heavy, metric, 2, 1).cn["dropped_proposals"] > 0
    assert r.cn["link_rows"] > 0 and r.cn0["dropped_proposals"] == 0
    OR.check_well_formed(O, metric, r.ex, r.ed, OR.mcaps_of(heavy))
    insert_only = OR.Run(O, OR.LINK, metric, 2, 1)
    assert insert_only.cn0["dropped_proposals"] == 0 and insert_only.cn["dropped_proposals"] > 0
    for desc in (False, True):
        r = OR.Run(O, OR.LINK, metric, 2, 1, batch_link=1, descending=desc)
        own = r.cn["dropped_proposals"] - insert_only.cn["dropped_proposals"]
        print("link pass", metric, "descending" if desc else "ascending", "insert phase",
              insert_only.cn["dropped_proposals"], "link pass's own", own)
        assert own > 0 and r.cn["link_rows"] > 0 and r.cn["batches"] == 1
        OR.check_well_formed(O, metric, r.ex, r.ed, OR.mcaps_of(OR.LINK))
        lv, cn = r.add_next()
        assert cn["dropped_proposals"] == 0
    u = OR.UPDATE
    keys, X, ukeys, V = OR.update_data(metric)
    g = O.Graph(metric=metric, order=O.ORDER_DEV, M=u["M"], M0=u["m0"], Ml=0.25, EfSearch=64, seed=BR.RNG_SEED)
    cn0 = g.add_batch(keys[:u["n"]], X[:u["n"]], g.preview_levels(u["n"]), **u["opts"])
    found, cn = g.update(ukeys, V, **u["opts"], **OR.one_batch(u["nu"]))
    assert cn0["dropped_proposals"] == 0 and found.all()
    assert cn["update_chunks"] == 1 and cn["dropped_proposals"] > 0
    OR.check_well_formed(O, metric, g.export(), g.export_edge_dist(), OR.mcaps_of(u))
    cn2 = g.add_batch(keys[u["n"]:], X[u["n"]:], g.preview_levels(OR.NEXT), **u["opts"])
    assert cn2["dropped_proposals"] == 0
