"""GPU: the ordered beam search (option "search_order"; beam.hpp k_beam_descend,
order.hip, search_host.cpp).

Large batches run the greedy descent as a pre-pass, sort the queries by their
descent path and search layer 0 in that order, each workgroup writing at its
query's original index.  Every query's search is independent of the others, so
the lists are the fused single-launch search's bit for bit (and the oracle's
MODE_BEAM lists), and the five search counters are the same sums.

Every call writes into output tensors pre-filled with a sentinel (key -7,
distance NaN, count -7): a query the permutation skipped shows up as a sentinel,
not as an earlier call's answer left in reused memory.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import _clustered, _metric_fn, _same_results

pytestmark = pytest.mark.gpu

COUNTERS = ("search_dist_evals", "search_expansions", "search_screened", "search_f32_evals", "visited_resets")
NQ = 1200


@pytest.fixture(scope="module")
def built(H, O):
    """one batched graph per metric, mirrored into the oracle; every batch size is ordered"""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(141 + metric)
        n, d = 20000, 96
        X = _clustered(rng, n, d, intrinsic=24)
        Q = _clustered(rng, NQ, d, intrinsic=24)
        g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=5, build_mode=H.BUILD_BATCH,
                    ef_construction=100, heuristic=2, m0=32)
        g.add_arrays(np.arange(n) * 3 + 1, X)
        g.set_option("search_order_min_b", 1)
        o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64)
        o.import_graph(**g.export())
        out[metric] = (g, o, Q, X)
    yield out
    for g, _, _, _ in out.values():
        g.close()


def _with(g, **opts):
    old = {k: g.get_option(k) for k in opts}
    for k, v in opts.items():
        g.set_option(k, v)
    return old


def _enqueue(torch, g, Qd, k, ef, stream=0):
    B, d = Qd.shape
    ok = torch.full((B, k), -7, dtype=torch.int64, device="cuda")
    od = torch.full((B, k), float("nan"), dtype=torch.float32, device="cuda")
    on = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    g.search_device(Qd.data_ptr(), B, d, k, ok.data_ptr(), od.data_ptr(), on.data_ptr(), mode=1, ef=ef, stream=stream)
    return ok, od, on


def _fetch(out):
    return tuple(x.cpu().numpy() for x in out)


def _no_sentinel(r):
    k, d, n = r
    assert (n != -7).all() and (n >= 0).all()
    assert (k != -7).all()
    assert not np.isnan(d).any()


def _identical(a, b):
    assert np.array_equal(a[2], b[2])
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _search(torch, g, Qd, k, ef, order):
    """one search_device call with search_order = order -> (lists, the five counters)"""
    g.set_option("search_order", order)
    g.reset_stats()
    out = _enqueue(torch, g, Qd, k, ef)
    torch.cuda.synchronize()
    g.device_status()
    st = g.stats()
    return _fetch(out), tuple(st[c] for c in COUNTERS)


def _check(torch, g, Q, k, ef, ref=None):
    """ordered == fused (lists and counters), no sentinel left, and == ref (the oracle's lists) when given"""
    Qd = torch.tensor(Q, device="cuda")
    old = g.get_option("search_order")
    try:
        r0, c0 = _search(torch, g, Qd, k, ef, 0)
        r1, c1 = _search(torch, g, Qd, k, ef, 1)
    finally:
        g.set_option("search_order", old)
    _no_sentinel(r0)
    _no_sentinel(r1)
    _identical(r1, r0)
    assert c1 == c0, (dict(zip(COUNTERS, c1)), dict(zip(COUNTERS, c0)))
    assert c1[0] > 0 and c1[1] >= len(Q)
    if ref is not None:
        _same_results(*r1, *ref)
    return r1


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("xw", [1, 2, 4])
@pytest.mark.parametrize("ef", [10, 64, 200, 600])
def test_ordered_matches_fused_and_oracle(H, O, built, metric, xw, ef):
    """B = 513 (just above the small-batch kernel): every list width (register
    lists, bl_merge lists, the LDS list), every XW, the screen on and off"""
    import torch

    g, o, Q, _ = built[metric]
    B = 513
    ks = (10, ef) if (ef == 200 and xw == 1) else (10,)  # k = ef once, on a wide list
    o.set_search_expand(xw)
    ref = {k: o.search(Q[:B], k, mode=O.MODE_BEAM, ef=ef) for k in ks}
    o.set_search_expand(1)
    old = _with(g, search_expand=xw)
    try:
        for screen in (1, 0):
            _with(g, screen=screen)
            for k in ks:
                _check(torch, g, Q[:B], k, ef, ref[k])
    finally:
        _with(g, screen=1, **old)


@pytest.mark.parametrize("B", [8, 9, 15, 17, 23, 1])
def test_ragged_and_empty_chunks(H, O, built, B):
    """fewer queries than 8 chunks can share evenly: B % 8 in {0, 1, 7}, chunks
    of one query, empty trailing chunks.  With the small-batch kernel off the
    one-wave kernel runs the ordered path; with it on, the fused path runs."""
    import torch

    g, o, Q, _ = built[0]
    ref = o.search(Q[100 : 100 + B], 10, mode=O.MODE_BEAM, ef=64)
    for mw in (0, 512):
        old = _with(g, beam_mw_max_b=mw)
        try:
            _check(torch, g, Q[100 : 100 + B], 10, 64, ref)
        finally:
            _with(g, **old)


@pytest.mark.parametrize("top,fields,mapping", [(0, 0, 1), (1, 1, 0), (2, 2, 1), (3, 8, 0), (31, 8, 1), (31, 3, 0)])
def test_key_and_mapping_variants(H, O, built, top, fields, mapping):
    """the plain mapping (workgroup i takes sorted position i) and the chunked
    one, keys of one to eight layers from any top layer (past the graph's top:
    clamped), node ids whole (wide fields) and hashed (narrow fields): the
    order changes, the results do not"""
    import torch

    g, o, Q, _ = built[0]
    ref = o.search(Q[:521], 10, mode=O.MODE_BEAM, ef=64)
    old = _with(g, search_order_top=top, search_order_fields=fields, search_order_map=mapping)
    try:
        _check(torch, g, Q[:521], 10, 64, ref)
        _check(torch, g, Q[300:311], 10, 200)  # (ordered against fused: ragged chunks on a bl_merge list)
    finally:
        _with(g, **old)


def test_threshold(H, O, built):
    """B exactly at search_order_min_b (ordered) and one below it (fused)"""
    import torch

    g, o, Q, _ = built[1]
    old = _with(g, search_order_min_b=600)
    try:
        assert g.get_option("search_order_min_b") == 600
        ref = o.search(Q[:600], 10, mode=O.MODE_BEAM, ef=64)
        _check(torch, g, Q[:600], 10, 64, ref)
        _check(torch, g, Q[:599], 10, 64, tuple(x[:599] for x in ref))
    finally:
        _with(g, **old)


@pytest.mark.parametrize("metric", [0, 1])
def test_equal_keys_and_stored_rows(H, O, built, metric):
    """all queries identical (every sort key equal), and every query a stored row"""
    import torch

    g, o, Q, X = built[metric]
    same = np.repeat(Q[7:8], 520, axis=0)
    r = _check(torch, g, same, 10, 64, o.search(same, 10, mode=O.MODE_BEAM, ef=64))
    assert (r[0] == r[0][0]).all()
    rows = X[np.arange(0, 20000, 37)[:530]]
    r = _check(torch, g, rows, 10, 200, o.search(rows, 10, mode=O.MODE_BEAM, ef=200))
    assert np.mean(r[0][:, 0] == (np.arange(0, 20000, 37)[:530] * 3 + 1)) > 0.9


def test_after_deletes(H, O):
    """the top layer's entry row and a few hundred others deleted, among them
    every other row of the upper layers (rows the descent lands on): the
    deg == -2 restart and the layer_entry[0] fallback of the descent pre-pass"""
    import torch

    rng = np.random.default_rng(15)
    n, d = 6000, 40
    X = _clustered(rng, n, d)
    Q = _clustered(rng, 530, d)
    g = H.Graph(M=12, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=3, build_mode=H.BUILD_BATCH,
                ef_construction=80, heuristic=2, m0=24)
    g.add_arrays(np.arange(n), X)
    g.set_option("search_order_min_b", 1)
    ex = g.export()
    upper = np.flatnonzero(ex["deg"][1] != -2)
    gone = sorted({int(ex["entry"][-1])} | set(upper[::2].tolist()) | set(range(0, n, 23)))
    assert len(gone) > 300
    g.BatchDelete(gone)
    o = O.Graph(metric=O.COSINE, order=O.ORDER_DEV, M=12, M0=24, Ml=0.25, EfSearch=64)
    o.import_graph(**g.export())
    for ef in (32, 150):
        r = _check(torch, g, Q, 10, ef, o.search(Q, 10, mode=O.MODE_BEAM, ef=ef))
        assert not (set(r[0][r[0] >= 0].tolist()) & set(gone))
    g.close()


def test_layer0_only_graph(H, O):
    """a graph whose only layer is 0: no descent, every query has the same key"""
    import torch

    rng = np.random.default_rng(16)
    n, d = 300, 32
    X = _clustered(rng, n, d)
    Q = _clustered(rng, 40, d)
    g = H.Graph(M=8, Ml=0.25, EfSearch=64, Distance=H.EuclideanDistance, Rng=3, build_mode=H.BUILD_BATCH,
                ef_construction=40, heuristic=2, m0=16)
    g.add_arrays(np.arange(n), X, levels=np.zeros(n, np.int32))
    assert g.export()["deg"].shape[0] == 1
    g.set_option("search_order_min_b", 1)
    g.set_option("beam_mw_max_b", 0)
    o = O.Graph(metric=O.EUCLIDEAN, order=O.ORDER_DEV, M=8, M0=16, Ml=0.25, EfSearch=64)
    o.import_graph(**g.export())
    for B in (40, 9):
        _check(torch, g, Q[:B], 5, 64, o.search(Q[:B], 5, mode=O.MODE_BEAM, ef=64))
    g.close()


def test_buffer_growth_and_reuse(H, O, built):
    """larger, then smaller, then larger batches on one handle"""
    import torch

    g, o, Q, _ = built[0]
    ref = o.search(Q, 10, mode=O.MODE_BEAM, ef=64)
    for B in (600, 40, NQ, 513):
        old = _with(g, beam_mw_max_b=0)
        try:
            _check(torch, g, Q[:B], 10, 64, tuple(x[:B] for x in ref))
        finally:
            _with(g, **old)


def test_two_handles_one_stream(H, O, built):
    """two handles searched alternately on one stream, nothing waited for in between"""
    import torch

    (g0, _, Q0, _), (g1, _, Q1, _) = built[0], built[1]
    Qa, Qb = torch.tensor(Q0[:700], device="cuda"), torch.tensor(Q1[:520], device="cuda")
    want_a, _ = _search(torch, g0, Qa, 10, 64, 0)
    want_b, _ = _search(torch, g1, Qb, 10, 200, 0)
    g0.set_option("search_order", 1)
    g1.set_option("search_order", 1)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        for _ in range(3):
            outs.append((_enqueue(torch, g0, Qa, 10, 64, s.cuda_stream), want_a))
            outs.append((_enqueue(torch, g1, Qb, 10, 200, s.cuda_stream), want_b))
    torch.cuda.synchronize()
    g0.device_status()
    g1.device_status()
    for out, want in outs:
        got = _fetch(out)
        _no_sentinel(got)
        _identical(got, want)


def test_option_values(H):
    g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=H.CosineDistance)
    assert g.get_option("search_order") in (0, 1)
    assert g.get_option("search_order_min_b") >= 1
    with pytest.raises(H.HnswError, match="search_order must be 0 or 1"):
        g.set_option("search_order", 2)
    with pytest.raises(H.HnswError, match="search_order_min_b must be >= 1"):
        g.set_option("search_order_min_b", 0)
    for v in (0, 1):
        g.set_option("search_order", v)
        assert g.get_option("search_order") == v
    g.set_option("search_order_min_b", 4096)
    assert g.get_option("search_order_min_b") == 4096
    g.close()
