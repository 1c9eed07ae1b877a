"""GPU: the batched insert, its link pass and the update where a commit drops reverse proposals
(a row received more than inc_cap = 64 in one commit): the `slot >= inc_cap` branches of
batch_insert and k_batch_link, the `nin > inc_cap` clamps of k_batch_commit and
k_batch_link_apply, a commit of 63 + 64 = 127 entries, and the slots' state afterwards.

Which proposals survive depends on arrival order, so the engine's graph is compared with the set
of valid graphs (tests/overflow_ref.py; tests/test_batch_overflow.py shows on the CPU that the
check accepts two arrival orders and rejects what is no valid commit), the drop counter with the
exact count, and the next batch -- which drops nothing -- with the restatement continued from
the engine's export, bit for bit.  No tolerance anywhere.
"""
import numpy as np
import pytest

from tests import batch_ref as BR
from tests import compact_ref as CR
from tests import overflow_ref as OR
from tests.test_gpu_parity import _metric_fn

pytestmark = pytest.mark.gpu

# engine-only: they change how the engine runs, not what a commit may give.  screen 0 and the
# default reach k_batch_commit's candidate-major and row-major loops.
VARIANTS = ({}, dict(build_mw_max=0), dict(build_mw_max=1 << 30), dict(fuse_descent=0), dict(screen=0))
IDS = [i + (vi,) for i in OR.case_ids() for vi in range(len(VARIANTS))]


def _graph(H, shape, metric, **opts):
    return H.Graph(M=shape["M"], Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=BR.RNG_SEED,
                   build_mode=H.BUILD_BATCH, m0=shape["m0"], **opts)


def _dropped(g):
    return g.stats()["dropped_proposals"]


class Overflowed:
    """the engine after the case's two adds: n0 rows under the default schedule (no drop), then the
    nb rows as one batch, levels capped at the top layer"""

    def __init__(self, H, case, metric, h, kp, variant, batch_link=0):
        n0, nb = case["n0"], case["nb"]
        self.keys, self.X = OR.data_of(case, metric)
        self.g = g = _graph(H, case, metric, heuristic=h, keep_pruned=kp, **case["opts"], **variant)
        lv0 = g.preview_levels(n0)
        g.add_arrays(self.keys[:n0], self.X[:n0], levels=lv0)
        assert _dropped(g) == 0
        self.E0, self.D0 = g.export(), g.export_edge_dist()
        lvb = np.minimum(g.preview_levels(nb), self.E0["deg"].shape[0] - 1).astype(np.int32)
        self.levels = (lv0, lvb)
        for k, v in OR.one_batch(nb).items():
            g.set_option(k, v)
        g.set_option("batch_link", batch_link)
        g.add_arrays(self.keys[n0:n0 + nb], self.X[n0:n0 + nb], levels=lvb)
        self.dropped = _dropped(g)
        self.ex, self.ed = g.export(), g.export_edge_dist()


@pytest.fixture(scope="module")
def refs(O):
    """per case, the restatement runs with every proposal kept and with 64 slots, given the
    engine's levels: computed once for a case's variants (the levels do not depend on them)"""
    cache = {}

    def get(name, metric, h, kp, levels):
        key = (name, metric, h, kp)
        if key not in cache:
            case = OR.CASES[name]
            cache[key] = (OR.Run(O, case, metric, h, kp, levels=levels, inc_cap=OR.FULL_CAP),
                          OR.Run(O, case, metric, h, kp, levels=levels))
        full = cache[key][0]
        assert all(np.array_equal(a, b) for a, b in zip(full.levels, levels))
        return cache[key]

    return get


def _next_batch_exact(H, O, g, shape, metric, opts, keys, X, queries):
    """The state an overflowed commit leaves is clean: a fresh restatement holding the engine's
    export, and the engine, are given NEXT further rows under the default schedule; neither drops
    a proposal, and the exports, the edge distances and the searches on them are equal bit for
    bit.  (A stale inc_cnt, a stale slot or a corrupted row shows here.)"""
    ex, ed = g.export(), g.export_edge_dist()
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=shape["M"], M0=shape["m0"], Ml=0.25, EfSearch=64, seed=BR.RNG_SEED)
    o.import_graph(ex["keys"], ex["vecs"], ex["deg"], ex["adj"], ex["entry"], ex["dead"], edge_dist=ed)
    for k, v in OR.DEFAULT_SCHEDULE.items():
        g.set_option(k, v)
    g.set_option("batch_link", 0)
    before = _dropped(g)
    lv = g.preview_levels(len(keys))
    g.add_arrays(keys, X, levels=lv)
    cn = o.add_batch(keys, X, lv, **opts)
    assert cn["dropped_proposals"] == 0 and cn["batches"] > 1
    assert _dropped(g) == before
    BR.same_export(g.export(), o.export(), g.export_edge_dist(), o.export_edge_dist(), what="next batch")
    CR.same_lists(g.search_arrays(queries, 10, mode=H.MODE_BEAM, ef=64), o.search(queries, 10, mode=O.MODE_BEAM, ef=64))
    CR.same_lists(g.search_arrays(queries, 10, mode=H.MODE_EXACT), o.search(queries, 10, mode=O.MODE_EXACT))


def _finds_own_key(H, g, keys, V):
    k1, _, n1 = g.search_arrays(V, 1, mode=H.MODE_EXACT)
    assert (n1 == 1).all() and k1[:, 0].tolist() == keys.tolist()


def _queries(metric, d):
    return BR.Gen(101 + metric, d).rows(32)[0]


@pytest.mark.parametrize("name,metric,h,kp,vi", IDS, ids=lambda v: v if isinstance(v, str) else str(v))
def test_engine_overflow_is_a_valid_commit(H, O, refs, name, metric, h, kp, vi):
    """the engine's graph is a valid commit, and its drop counter is the exact count and the
    restatement's (the figures are printed: run with -s)"""
    case = OR.CASES[name]
    eng = Overflowed(H, case, metric, h, kp, VARIANTS[vi])
    full, ref = refs(name, metric, h, kp, eng.levels)
    assert full.cn0["dropped_proposals"] == 0 and full.cn["dropped_proposals"] == 0
    BR.same_export(eng.E0, full.E0, eng.D0, full.D0, what="pre-batch")  # exact while nothing is dropped
    caps = OR.mcaps_of(case)
    OR.check_well_formed(O, metric, eng.ex, eng.ed, caps)
    info = OR.check_overflowed_batch(O, metric, eng.E0, eng.D0, (full.ex, full.ed), eng.ex, eng.ed, case["n0"], caps,
                                     h, OR.alpha_of())
    print("overflow", name, metric, h, kp, vi, "engine dropped", eng.dropped, "expected", info["dropped"],
          "restatement", ref.cn["dropped_proposals"], "rows past the cap", len(info["rows"]),
          "largest commit", info["tot_max"])
    assert info["dropped"] > 0
    assert eng.dropped == info["dropped"] == ref.cn["dropped_proposals"]
    if name == "dense":
        assert info["tot_max"] == 127
    eng.g.close()


@pytest.mark.parametrize("name,metric,h,kp,vi", IDS, ids=lambda v: v if isinstance(v, str) else str(v))
def test_next_batch_after_overflow_is_exact(H, O, name, metric, h, kp, vi):
    case = OR.CASES[name]
    eng = Overflowed(H, case, metric, h, kp, VARIANTS[vi])
    assert eng.dropped > 0
    n1 = case["n0"] + case["nb"]
    opts = dict(case["opts"], heuristic=h, keep_pruned=kp)
    _next_batch_exact(H, O, eng.g, case, metric, opts, eng.keys[n1:], eng.X[n1:], _queries(metric, case["d"]))
    eng.g.close()


def _insert_only_drops(H, O, case, metric, h, kp):
    """the drops of the case's batch without the link pass, exactly: sum(max(0, |P| - inc_cap)),
    which the engine's counter equals.  The insert phase of a layer does not read what the link
    pass of the layers above wrote, so these are the insert phase's drops with the link pass on."""
    eng = Overflowed(H, case, metric, h, kp, {})
    full = OR.Run(O, case, metric, h, kp, levels=eng.levels, inc_cap=OR.FULL_CAP)
    info = OR.check_overflowed_batch(O, metric, eng.E0, eng.D0, (full.ex, full.ed), eng.ex, eng.ed, case["n0"],
                                     OR.mcaps_of(case), h, OR.alpha_of())
    assert eng.dropped == info["dropped"] > 0
    eng.g.close()
    return info["dropped"]


def _link_overflow(H, O, case, metric, own_drops):
    """own_drops: the link pass itself must drop proposals (a batch row received more than inc_cap
    of them: the `p >= inc_cap` branch of k_batch_link, the `nin` clamp of k_batch_link_apply),
    that is, the engine's counter exceeds the insert phase's exact count"""
    h, kp = 2, 1
    insert_only = _insert_only_drops(H, O, case, metric, h, kp)
    eng = Overflowed(H, case, metric, h, kp, {}, batch_link=1)
    print("overflow link", metric, "n0", case["n0"], "nb", case["nb"], "insert phase dropped", insert_only,
          "with the link pass", eng.dropped, "link rows", eng.g.get_option("last_link_rows"))
    assert eng.g.get_option("last_link_rows") > 0
    assert eng.dropped >= insert_only
    if own_drops:
        assert eng.dropped > insert_only
    OR.check_well_formed(O, metric, eng.ex, eng.ed, OR.mcaps_of(case))
    n0, n1 = case["n0"], case["n0"] + case["nb"]
    _finds_own_key(H, eng.g, eng.keys[n0:n1], eng.X[n0:n1])
    _next_batch_exact(H, O, eng.g, case, metric, dict(case["opts"], heuristic=h, keep_pruned=kp), eng.keys[n1:],
                      eng.X[n1:], _queries(metric, case["d"]))
    eng.g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_link_and_update_overflow(H, O, metric):
    """The other two writers of the slots.  After an overflowed insert commit the link search
    reads a layer that depends on arrival order, so there is no exact reference: the graph is well
    formed, the counter shows the drop, the next batch is exact again, and every added or updated
    row finds its own key.

    The heavy case with batch_link 1 runs the link pass over layers whose insert commit
    overflowed; whether its link pass drops a proposal of its own is not claimed (link proposals
    go to batch-mates only: on the restatement none is dropped there under cosine).  OR.LINK, a
    batch of 500 on 20 rows, is the case whose link pass itself overflows, under both metrics
    (tests/test_batch_overflow.py: on the restatement, in both arrival orders)."""
    _link_overflow(H, O, OR.CASES["heavy"], metric, own_drops=False)
    _link_overflow(H, O, OR.LINK, metric, own_drops=True)
    # the update: one chunk whose rows are moved next to two rows that stay
    u = OR.UPDATE
    keys, X, ukeys, V = OR.update_data(metric)
    g = _graph(H, u, metric, **u["opts"])
    g.add_arrays(keys[:u["n"]], X[:u["n"]], levels=g.preview_levels(u["n"]))
    assert _dropped(g) == 0
    for k, v in OR.one_batch(u["nu"]).items():
        g.set_option(k, v)
    assert g.update_arrays(ukeys, V).all()
    print("overflow update", metric, "engine dropped", _dropped(g))
    assert g.get_option("last_update_chunks") == 1 and _dropped(g) > 0
    OR.check_well_formed(O, metric, g.export(), g.export_edge_dist(), OR.mcaps_of(u))
    _finds_own_key(H, g, ukeys, V)
    _next_batch_exact(H, O, g, u, metric, u["opts"], keys[u["n"]:], X[u["n"]:], _queries(metric, u["d"]))
    g.close()


def test_caps_past_the_commit_arrays_are_refused(H):
    """k_batch_commit ranks a row and its slots in 128-entry arrays: a degree cap with
    cap + inc_cap > 128 is refused on the host before any kernel runs (63 is accepted: the dense
    case above)"""
    X = BR.Gen(3, 16).rows(8)[0]
    for M, m0 in ((8, 64), (64, 63)):
        g = _graph(H, dict(M=M, m0=m0), 0)
        with pytest.raises(H.HnswError, match="degree caps above 63 unsupported"):
            g.add_arrays(BR.keys_of(8), X)
        assert g.Len() == 0
        g.close()
