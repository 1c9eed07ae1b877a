"""GPU: the beam search past the register lists, 513 <= max(ef, k) <= 2048
(beam.hpp k_search_beam_lds: the layer-0 list in LDS, device_search.hpp LList).

The list is the same sorted list with the same operations, so every result is
compared bit for bit with the oracle's restatement of the search
(oracle.c beam_layer_search, any ef): both metrics, search_expand 1 / 2 / 4, the
fp16 screen on and off, the compact and the 32-bit visited set, sets small
enough to forget on every query, lists that never fill, tied distances (the
sequential fallback of the merge), deleted rows (unlinked by the batched
repair, and left inside the lists by reference-semantics deletes), small
batches and the negatives path.  Option beam_lds_min_ef lowers the tier's
threshold so that the LDS list also runs against the register lists at equal
ef.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import _clustered, _metric_fn, _same_results

pytestmark = pytest.mark.gpu


def _graph(H, O, metric, keys, X, seed=5):
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=seed, build_mode=H.BUILD_BATCH,
                ef_construction=100, heuristic=2, m0=32)
    g.add_arrays(keys, X)
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64)
    o.import_graph(**g.export())
    return g, o


@pytest.fixture(scope="module")
def built(H, O):
    """one batched graph per metric, mirrored into the oracle"""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(61 + metric)
        n, d = 20000, 96
        X = _clustered(rng, n, d, intrinsic=24)
        Q = _clustered(rng, 32, d, intrinsic=24)
        g, o = _graph(H, O, metric, np.arange(n) * 3 + 1, X)
        out[metric] = (g, o, Q)
    yield out
    for g, _, _ in out.values():
        g.close()


def _with(g, **opts):
    old = {k: g.get_option(k) for k in opts}
    for k, v in opts.items():
        g.set_option(k, v)
    return old


def _oracle(O, o, Q, k, ef, xw):
    o.set_search_expand(xw)
    try:
        return o.search(Q, k, mode=O.MODE_BEAM, ef=ef)
    finally:
        o.set_search_expand(1)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 2, 4])
@pytest.mark.parametrize("ef", [513, 576, 1000, 2048])
def test_wide_ef_matches_oracle(H, O, built, metric, xw, ef):
    """513 / 576: either side of a 64-entry chunk edge; 1000: a ragged last
    chunk; 2048: the full capacity (and the compact set resets)"""
    g, o, Q = built[metric]
    ref = {k: _oracle(O, o, Q, k, ef, xw) for k in (10, ef)}
    old = _with(g, search_expand=xw)
    try:
        for screen in (1, 0):
            for compact in (1, 0):
                _with(g, screen=screen, vis_compact=compact)
                for k in (10, ef):
                    gk, gd, gn = g.search_arrays(Q, k, mode=H.MODE_BEAM, ef=ef)
                    _same_results(gk, gd, gn, *ref[k])
    finally:
        _with(g, screen=1, vis_compact=1, **old)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 4])
@pytest.mark.parametrize("ef", [65, 128, 200, 256, 512])
def test_lds_tier_equals_register_tier(H, O, built, metric, xw, ef):
    g, o, Q = built[metric]
    old = _with(g, search_expand=xw)
    try:
        for k in (10, ef):
            ref = _oracle(O, o, Q, k, ef, xw)
            reg = g.search_arrays(Q, k, mode=H.MODE_BEAM, ef=ef)
            g.set_option("beam_lds_min_ef", 65)
            lds = g.search_arrays(Q, k, mode=H.MODE_BEAM, ef=ef)
            g.set_option("beam_lds_min_ef", 513)
            _same_results(*lds, *reg)
            _same_results(*lds, *ref)
    finally:
        _with(g, beam_lds_min_ef=513, **old)


@pytest.mark.parametrize("ef", [1024, 2048])
def test_list_never_fills(H, O, ef):
    rng = np.random.default_rng(9)
    n, d = 700, 24
    X = _clustered(rng, n, d)
    Q = _clustered(rng, 32, d)
    g, o = _graph(H, O, 0, np.arange(n) * 2 + 7, X, seed=2)
    try:
        gk, gd, gn = g.search_arrays(Q, ef, mode=H.MODE_BEAM, ef=ef)
        rk, rd, rn = o.search(Q, ef, mode=O.MODE_BEAM, ef=ef)
        assert (gn < ef).all() and (gn > 0).all()
        _same_results(gk, gd, gn, rk, rd, rn)
        for b in range(len(Q)):
            assert (gk[b, gn[b]:] == -1).all(), b
            assert np.isposinf(gd[b, gn[b]:]).all(), b
    finally:
        g.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 4])
def test_ties_and_sequential_fallback(H, O, metric, xw):
    """1,500 rows are exact copies of other rows (equal distances, distinct
    ids: the merge's sequential path) and one row is all zero (NaN under
    cosine: never listed)"""
    rng = np.random.default_rng(23 + metric)
    n, d = 6000, 40
    X = _clustered(rng, n, d)
    src = rng.choice(4500, 1500, replace=False)
    X[4500:] = X[src]
    X[77] = 0.0
    Q = _clustered(rng, 32, d)
    Q[:8] = X[src[:8]]  # queries on duplicated rows: ties at the head of the list
    g, o = _graph(H, O, metric, np.arange(n) * 5 + 2, X, seed=4)
    old = _with(g, search_expand=xw)
    try:
        gk, gd, gn = g.search_arrays(Q, 600, mode=H.MODE_BEAM, ef=600)
        _same_results(gk, gd, gn, *_oracle(O, o, Q, 600, 600, xw))
        if metric == 0:  # cosine: the zero row's distance is NaN
            assert 77 * 5 + 2 not in set(gk.ravel().tolist())
    finally:
        _with(g, **old)
        g.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 4])
def test_wide_ef_forgetting(H, O, built, metric, xw):
    """32-bit visited sets far smaller than the list: every step forgets, the
    results are still the oracle's (which never forgets)"""
    g, o, Q = built[metric]
    ref = _oracle(O, o, Q, 10, 600, xw)
    old = _with(g, search_expand=xw, vis_compact=0, vis_entries=0)
    try:
        for ve in (64, 256):
            g.set_option("vis_entries", ve)
            g.reset_stats()
            gk, gd, gn = g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=600)
            assert g.stats()["visited_resets"] >= len(Q)
            _same_results(gk, gd, gn, *ref)
    finally:
        g.set_option("vis_entries", 0)
        _with(g, **{k: v for k, v in old.items() if k != "vis_entries"})


def test_wide_ef_auto_visited_size(H, O, built):
    """the automatically sized 32-bit set grows with the list inside the
    launch only: the option reads back unchanged and the lists are the
    oracle's"""
    g, o, Q = built[0]
    old = _with(g, vis_compact=0)
    try:
        g.set_option("vis_entries", 0)
        before = g.get_option("vis_entries")
        gk, gd, gn = g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=2048)
        assert g.get_option("vis_entries") == before
        _same_results(gk, gd, gn, *_oracle(O, o, Q, 10, 2048, 1))
    finally:
        _with(g, **old)


def test_wide_ef_after_deletes(H, O):
    """deleted rows route the search but are never returned"""
    rng = np.random.default_rng(5)
    n, d = 6000, 40
    X = _clustered(rng, n, d)
    Q = _clustered(rng, 32, d)
    g = H.Graph(M=12, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=3, build_mode=H.BUILD_BATCH,
                ef_construction=80, heuristic=2, m0=24)
    try:
        g.add_arrays(np.arange(n), X)
        g.BatchDelete(list(range(0, n, 7)))
        o = O.Graph(metric=O.COSINE, order=O.ORDER_DEV, M=12, M0=24, Ml=0.25, EfSearch=64)
        o.import_graph(**g.export())
        g.set_option("search_expand", 4)
        for k in (10, 700):
            gk, gd, gn = g.search_arrays(Q, k, mode=H.MODE_BEAM, ef=700)
            _same_results(gk, gd, gn, *_oracle(O, o, Q, k, 700, 4))
            assert not (set(gk[gk >= 0].tolist()) & set(range(0, n, 7)))
    finally:
        g.close()


@pytest.fixture(scope="module")
def dangling(H, O):
    """per metric: a reference-semantics graph whose deletes leave dangling
    edges (BatchDelete on a compat build isolates the rows but live rows keep
    their edges to them, so deleted rows enter the layer-0 lists), mirrored
    into the oracle, and a second oracle copy with the dead flags cleared,
    which returns the lists as they stand before the dead rows are dropped"""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(17)
        n, d = 1500, 24
        X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
        Q = rng.uniform(-1, 1, (32, d)).astype(np.float32)
        keys = np.arange(n, dtype=np.int64) * 3 + 1
        g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), Rng=11)
        g.add_arrays(keys, X)
        gone = [int(x) for x in keys[::4]]
        assert all(g.BatchDelete(gone))
        ex = g.export()
        o = O.Graph(metric=metric, order=O.ORDER_DEV, M=8, Ml=0.25, EfSearch=20)
        o.import_graph(**ex)
        raw = O.Graph(metric=metric, order=O.ORDER_DEV, M=8, Ml=0.25, EfSearch=20)
        raw.import_graph(**dict(ex, dead=np.zeros_like(ex["dead"])))
        out[metric] = (g, o, raw, Q, set(gone))
    yield out
    for g, *_ in out.values():
        g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_dead_rows_sit_in_the_lists(O, dangling, metric):
    """the fixture is worth something: with the dead flags cleared, at least
    half of the queries hold a deleted key among the first 64 entries of their
    ef = 200 list and another past entry 64 (both chunks of the register list,
    the first and a later chunk of the LDS list)"""
    _, _, raw, Q, gone = dangling[metric]
    rk, _, rn = raw.search(Q, 200, mode=O.MODE_BEAM, ef=200)
    both = 0
    for b in range(len(Q)):
        head = any(int(x) in gone for x in rk[b, :min(rn[b], 64)])
        tail = any(int(x) in gone for x in rk[b, 64:rn[b]])
        both += head and tail
    assert both >= len(Q) // 2, both


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 4])
def test_wide_ef_dead_rows_in_list(H, O, dangling, metric, xw):
    """deleted rows inside the list, ef = 200 on both tiers, fused and ordered
    launch: the first k live entries are the oracle's for k inside the first
    chunk, on a chunk edge, past it and at k = ef, where the list runs out of
    live rows and the tail is padded"""
    g, o, _, Q, gone = dangling[metric]
    ef = 200
    ks = (10, 64, 65, 130, 200)
    ref = {k: _oracle(O, o, Q, k, ef, xw) for k in ks}
    old = _with(g, search_expand=xw, search_order=0, search_order_min_b=1, beam_lds_min_ef=513)
    try:
        for order in (0, 1):
            g.set_option("search_order", order)
            for k in ks:
                g.set_option("beam_lds_min_ef", 513)
                reg = g.search_arrays(Q, k, mode=H.MODE_BEAM, ef=ef)
                g.set_option("beam_lds_min_ef", 65)
                lds = g.search_arrays(Q, k, mode=H.MODE_BEAM, ef=ef)
                _same_results(*lds, *reg)
                _same_results(*lds, *ref[k])
                for gk, gd, gn in (reg, lds):
                    assert not (set(gk[gk >= 0].tolist()) & gone), (order, k)
                    if k == ef:
                        assert (gn < ef).all() and (gn > 0).all()
                        for b in range(len(Q)):
                            assert (gk[b, gn[b]:] == -1).all(), b
                            assert np.isposinf(gd[b, gn[b]:]).all(), b
    finally:
        _with(g, **old)


def test_wide_ef_small_batches(H, O, built):
    """B = 1 and B = 7 equal the same queries inside the 32-query batch"""
    g, o, Q = built[1]
    fk, fd, fn = g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=1024)
    _same_results(fk, fd, fn, *_oracle(O, o, Q, 10, 1024, 1))
    for lo, hi in ((0, 1), (5, 12)):
        gk, gd, gn = g.search_arrays(Q[lo:hi], 10, mode=H.MODE_BEAM, ef=1024)
        _same_results(gk, gd, gn, fk[lo:hi], fd[lo:hi], fn[lo:hi])


@pytest.mark.parametrize("metric", [0, 1])
def test_wide_ef_expansion_counts(H, O, built, metric):
    g, o, Q = built[metric]
    old = _with(g, search_expand=1)
    try:
        for xw in (1, 2, 4):
            g.set_option("search_expand", xw)
            g.reset_stats()
            g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=1024)
            xs = g.stats()["search_expansions"]
            x0 = o.stats()[1]
            _oracle(O, o, Q, 10, 1024, xw)
            assert o.stats()[1] - x0 == xs, (xw, o.stats()[1] - x0, xs)
    finally:
        _with(g, **old)


@pytest.mark.parametrize("metric", [0, 1])
def test_wide_ef_negatives(H, O, built, metric):
    g, o, Q = built[metric]
    rng = np.random.default_rng(3)
    negs = [_clustered(rng, 2, Q.shape[1], intrinsic=24) for _ in range(8)]
    for k, w in ((10, 0.5), (40, 0.9)):
        gk, gs, gn = g.search_negatives_arrays(Q[:8], negs, k, w, mode=H.MODE_BEAM, ef=1024)
        rk, rs, rn = o.search_negatives(Q[:8], negs, k, w, mode=O.MODE_BEAM, ef=1024)
        _same_results(gk, gs, gn, rk, rs, rn)


def test_wide_ef_limits(H, built):
    g, _, Q = built[0]
    with pytest.raises(H.HnswError, match=r"max\(ef,k\) <= 2048"):
        g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=2049)
    with pytest.raises(H.HnswError, match=r"max\(ef,k\) <= 2048"):
        g.search_arrays(Q, 2049, mode=H.MODE_BEAM, ef=64)
    # an explicit visited set that does not fit a workgroup's LDS, next to the
    # list, is refused on the host, not launched: by the fused launch and, on the
    # ordered path, by the pre-pass in front of it (the same check)
    old = _with(g, vis_compact=0, vis_entries=32768, search_order=0, search_order_min_b=1)
    try:
        for order in (0, 1):
            g.set_option("search_order", order)
            with pytest.raises(H.HnswError, match="LDS budget exceeded"):
                g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=600)
    finally:
        g.set_option("vis_entries", 0)
        _with(g, **{k: v for k, v in old.items() if k != "vis_entries"})
    for k, v in old.items():
        if k != "vis_entries":
            assert g.get_option(k) == v
    assert g.get_option("beam_lds_min_ef") == 513
    for bad in (64, 514):
        with pytest.raises(H.HnswError, match=r"beam_lds_min_ef must be in \[65, 513\]"):
            g.set_option("beam_lds_min_ef", bad)
    assert g.get_option("beam_lds_min_ef") == 513
