"""GPU: the batched list update (device_search.hpp bl_merge) on steps that flush
more than once, and the whole list it leaves.

The merge tests of test_gpu_merge.py compare the first 10 of a 256- or
512-entry list on graphs of degree <= 32.  A wrong entry in the list's tail
shows there only if its later expansion changes the top 10, and a step whose
second buffer is wholly worse than the list its first flush left does not
occur on such graphs.  Here every comparison is of the whole list (k = ef),
bit for bit against the oracle's one-at-a-time restatement, and of the number
of expansions:

  * the staircase graphs of tests/staircase.py, where that step is built by
    hand (tests/test_staircase.py checks without a GPU that it is), also with
    rows whose distance is +INF or NaN arriving while the list fills;
  * random graphs of degree 63, at the list sizes around 256 and 512, with
    visited sets that forget on every query;
  * the batched insert, whose one-wave kernel merges (bl_merge) and whose
    4-wave kernel inserts one at a time (bl_insert): the same graph from both,
    on the staircase and on random rows at efConstruction 256 / 512.
"""
import numpy as np
import pytest

from tests import staircase as sc
from tests.test_gpu_parity import _bit_equal, _clustered, _metric_fn, _same_graph, _same_results

pytestmark = pytest.mark.gpu


def _first_diff(gk, gd, gn, rk, rd, rn):
    """(query, position, engine key, oracle key) of the first difference, or None"""
    for b in range(len(rn)):
        if gn[b] != rn[b]:
            return b, "count", int(gn[b]), int(rn[b])
        for i in range(rn[b]):
            if gk[b, i] != rk[b, i] or not _bit_equal(gd[b, i: i + 1], rd[b, i: i + 1]):
                return b, i, (int(gk[b, i]), float(gd[b, i])), (int(rk[b, i]), float(rd[b, i]))
    return None


def _same(res, ref, what):
    d = _first_diff(*res, *ref)
    assert d is None, f"{what}: first difference (query, position, engine, oracle) = {d}"
    _same_results(*res, *ref)


def _set(g, **opts):
    old = {k: g.get_option(k) for k in opts}
    for k, v in opts.items():
        g.set_option(k, v)
    return old


def _engine(H, s, **opts):
    g = H.Graph(M=32, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, s["info"]["metric"]), Rng=1,
                build_mode=H.BUILD_BATCH, m0=63, **opts)
    g.import_graph(**s["graph"])
    return g


def _staircase_search(H, O, s, what):
    """whole list and expansions, screen x visited set x (one query, a batch of 3)"""
    ef, xw = s["info"]["ef"], s["info"]["xw"]
    o = sc.oracle_graph(O, s)
    rk, rd, rn, ox = sc.oracle_list(O, o, s)
    assert rn[0] == ef
    g = _engine(H, s, search_expand=xw)
    try:
        for screen in (1, 0):
            for compact in (1, 0):
                _set(g, screen=screen, vis_compact=compact)
                for B in (1, 3):
                    Q = np.repeat(s["query"][None], B, axis=0)
                    g.reset_stats()
                    res = g.search_arrays(Q, ef, mode=H.MODE_BEAM, ef=ef)
                    x = g.stats()["search_expansions"]
                    ref = (np.repeat(rk, B, axis=0), np.repeat(rd, B, axis=0), np.repeat(rn, B))
                    _same(res, ref, (what, "screen", screen, "vis_compact", compact, "B", B))
                    assert x == B * ox, (what, x, B, ox)
    finally:
        g.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 2, 4])
@pytest.mark.parametrize("ef", [256, 300, 512])
def test_staircase_whole_list(H, O, ef, xw, metric):
    """ef 256 / 512 at XW 2 / 4: the step's second buffer (G2) is wholly worse
    than the list the first flush left and must be dropped whole; ef 300 takes
    bl_merge's `lb >= ef` fallback; XW 1 never flushes twice (the control)."""
    for width in (64, 63):
        for origin in ((0.0, 16.0) if metric == 1 else (0.0,)):  # (a zero query is never screened)
            s = sc.staircase(ef, xw, metric, width=width, origin=origin)
            _staircase_search(H, O, s, ("width", width, "origin", origin))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 2, 4])
@pytest.mark.parametrize("ef", [256, 300, 512])
def test_staircase_non_finite(H, O, ef, xw, metric):
    """rows at +INF (Euclidean, squares that overflow) or NaN (cosine, zero
    rows) arrive while the list fills: +INF ties the empty list's worst and is
    ordered by id through bl_insert, NaN is never listed"""
    s = sc.staircase(ef, xw, metric, width=63, bad=5, origin=16.0 if metric == 1 else 0.0)
    _staircase_search(H, O, s, ("bad", 5))


# ---------------------------------------------------------------------------
# random graphs of degree 63
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense(H, O):
    """one batched graph per metric with m0 = 63, mirrored into the oracle"""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(91 + metric)
        n, d = 8000, 32
        X = _clustered(rng, n, d, intrinsic=12)
        Q = _clustered(rng, 32, d, intrinsic=12)
        g = H.Graph(M=32, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=7, build_mode=H.BUILD_BATCH,
                    ef_construction=100, heuristic=2, m0=63)
        g.add_arrays(np.arange(n) * 3 + 1, X)
        ex = g.export()
        assert ex["deg"][0].max() > 32
        o = O.Graph(metric=metric, order=O.ORDER_DEV, M=32, M0=63, Ml=0.25, EfSearch=64)
        o.import_graph(**ex)
        out[metric] = (g, o, Q, {})
    yield out
    for g, _, _, _ in out.values():
        g.close()


def _dense_ref(O, built, xw, ef):
    g, o, Q, memo = built
    if (xw, ef) not in memo:
        o.set_search_expand(xw)
        x0 = o.stats()[1]
        memo[(xw, ef)] = (o.search(Q, ef, mode=O.MODE_BEAM, ef=ef), o.stats()[1] - x0)
        o.set_search_expand(1)
    return memo[(xw, ef)]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 2, 4])
@pytest.mark.parametrize("ef", [255, 256, 257, 511, 512])
def test_dense_graph_whole_list(H, O, dense, metric, xw, ef):
    g, o, Q, _ = dense[metric]
    ref, ox = _dense_ref(O, dense[metric], xw, ef)
    old = _set(g, search_expand=xw)
    try:
        g.reset_stats()
        res = g.search_arrays(Q, ef, mode=H.MODE_BEAM, ef=ef)
        x = g.stats()["search_expansions"]
        _same(res, ref, ("dense", metric, xw, ef))
        assert x == ox, (x, ox)
    finally:
        _set(g, **old)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 2, 4])
@pytest.mark.parametrize("ef", [256, 512])
def test_dense_graph_forgetting(H, O, dense, metric, xw, ef):
    """visited sets of 64 / 256 entries forget on every query: listed rows are
    met again and reach the merge's equal-distance fallback; the oracle never
    forgets, the list and the expansions are the same"""
    g, o, Q, _ = dense[metric]
    ref, ox = _dense_ref(O, dense[metric], xw, ef)
    old = _set(g, search_expand=xw)
    try:
        for vis_log2 in (6, 8):
            _set(g, vis_log2=vis_log2)
            g.reset_stats()
            res = g.search_arrays(Q, ef, mode=H.MODE_BEAM, ef=ef)
            st = g.stats()
            assert st["visited_resets"] >= len(Q), st
            _same(res, ref, ("forgetting", metric, xw, ef, vis_log2))
            assert st["search_expansions"] == ox, (st, ox)
    finally:
        _set(g, vis_log2=12, **old)


# ---------------------------------------------------------------------------
# the batched insert: one-wave kernel (bl_merge) against 4-wave kernel (bl_insert)
# ---------------------------------------------------------------------------
def _expected_neighbours(O, s, lst_ids, alpha_pct, keep_pruned, mcap):
    """batch_insert's selection over the oracle's list (ids in list order):
    a row is kept unless a kept row r has alpha d(c, r) < d(u, c); then the
    nearest dropped rows fill up (keep_pruned)"""
    metric, vecs, q = s["info"]["metric"], s["graph"]["vecs"], s["query"]
    f32 = np.float32
    alpha = f32(alpha_pct) / f32(100)
    kept = []
    for c in lst_ids:
        if len(kept) == mcap:
            break
        dc = f32(O.distance(metric, O.ORDER_DEV, q, vecs[c]))
        if all(not (alpha * f32(O.distance(metric, O.ORDER_DEV, vecs[c], vecs[r])) < dc) for r in kept):
            kept.append(c)
    if keep_pruned:
        for c in lst_ids:
            if len(kept) == mcap:
                break
            if c not in kept:
                kept.append(c)
    return set(kept)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [2, 4])
@pytest.mark.parametrize("ef", [256, 300, 512])
def test_staircase_through_the_insert(H, O, ef, xw, metric):
    """one row inserted at the query's position into the width-63 staircase: its
    layer search is the staircase search, and the whole list feeds the
    neighbour selection, so a G2 row on the last entry would put the bait
    among the new row's neighbours"""
    s = sc.staircase(ef, xw, metric, width=63, origin=16.0 if metric == 1 else 0.0)
    info, graph = s["info"], s["graph"]
    n = len(graph["keys"])
    id_of = {int(k): i for i, k in enumerate(graph["keys"])}
    o = sc.oracle_graph(O, s)
    rk, _, rn, _ = sc.oracle_list(O, o, s)
    lst_ids = [id_of[int(k)] for k in rk[0, : rn[0]]]
    assert info["Z"] not in lst_ids
    for keep_pruned in (0, 1):
        ex = {}
        for mw in (0, 1 << 30):
            g = _engine(H, s, ef_construction=ef, build_expand=xw, heuristic=2, keep_pruned=keep_pruned,
                        build_mw_max=mw)
            alpha_pct = g.get_option("prune_alpha_pct")
            g.add_arrays(np.array([1 << 40]), s["query"][None], levels=np.array([0], np.int32))
            ex[mw] = g.export()
            g.close()
        _same_graph(ex[0], ex[1 << 30])
        for mw, e in ex.items():
            assert e["keys"][n] == 1 << 40
            nb = set(e["adj"][0, n, : e["deg"][0, n]].tolist())
            assert info["Z"] not in nb, (mw, "the bait is a neighbour of the new row")
            assert nb == _expected_neighbours(O, s, lst_ids, alpha_pct, keep_pruned, 63), (mw, keep_pruned)


@pytest.fixture(scope="module")
def build_rows():
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(55 + metric)
        out[metric] = _clustered(rng, 6000, 48, intrinsic=16)
    return out


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("expand", [4, 2])
@pytest.mark.parametrize("upper_efc", [0, 256])
@pytest.mark.parametrize("efc", [256, 512])
def test_wide_build_kernels_identical(H, build_rows, efc, upper_efc, expand, metric):
    """efConstruction at the list boundaries: the one-wave insert kernel on every
    launch, the 4-wave kernel on every launch and the default split build the
    same graph and drop the same number of proposals"""
    X = build_rows[metric]
    n = len(X)
    ex, dropped = {}, {}
    for mw in (0, 1 << 30, None):
        opts = {} if mw is None else dict(build_mw_max=mw)
        g = H.Graph(M=32, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=3, build_mode=H.BUILD_BATCH,
                    ef_construction=efc, upper_efc=upper_efc, build_expand=expand, heuristic=2, m0=63, **opts)
        g.add_arrays(np.arange(n // 3), X[: n // 3])  # two calls: the second descends a multi-layer graph
        g.add_arrays(np.arange(n // 3, n), X[n // 3:])
        dropped[mw] = g.stats()["dropped_proposals"]
        ex[mw] = g.export()
        g.close()
    print("dropped_proposals", dropped)
    _same_graph(ex[0], ex[1 << 30])
    _same_graph(ex[0], ex[None])
    assert dropped[0] == dropped[1 << 30] == dropped[None], dropped
