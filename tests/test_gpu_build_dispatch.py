"""The insert and delete entry points reach the right kernel for every
dimension configuration: a wrong configuration behind a dimension reads rows at
the wrong pitch, and a wrong kernel of the batched insert's set (list width,
fp16 screen, expansion width, narrow launch) builds another graph.  Small
inputs throughout: the mistakes these tests look for show at any size."""
import numpy as np
import pytest

from tests.test_gpu_parity import _adds_agree, _clustered, _levels, _metric_fn, _same_graph, _same_results

pytestmark = pytest.mark.gpu

# one dimension per configuration of the table (lanes per row x float4 per lane)
ALL_DIMS = [48, 96, 200, 400, 768, 1000, 1536, 2048, 3072, 4096]


def _metric_of(d):
    return 0 if d in (48, 200, 400, 1536, 3072) else 1


# ---------------------------------------------------------------- compat insert / delete
# After deletes the reference's Add fails when a dangling edge leads it to a
# deleted elevator (graph.go:489-505), which these small M = 6 graphs do for
# most inputs; the seeds are ones for which the oracle takes all ten Adds.
COMPAT_SEED = {(400, 0): 422, (400, 1): 1400, (1000, 0): 1002, (1000, 1): 2002, (2048, 0): 2055, (2048, 1): 3053}


@pytest.mark.parametrize("waves", [1, 8])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [400, 1000, 2048])  # 64x2, 64x4, 64x8: the configurations no other compat test builds
def test_compat_insert_delete_configs(H, O, d, metric, waves):
    rng = np.random.default_rng(COMPAT_SEED[d, metric])
    n, M, ef = 200, 6, 16
    X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    keys = rng.permutation(5 * n)[:n].astype(np.int64) - n
    lv = _levels(O, metric, M, 0.25, ef, 19, n)
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=M, Ml=0.25, EfSearch=ef)
    g = H.Graph(M=M, Ml=0.25, EfSearch=ef, Distance=_metric_fn(H, metric), compat_waves=waves)
    o.add(keys, X, lv)
    g.add_arrays(keys, X, levels=lv)
    _same_graph(g.export(), o.export())
    gone = [int(x) for x in rng.choice(keys, 40, replace=False)]
    gone += gone[:1] + [10**7]  # one repeat and one missing key -> False
    assert g.BatchDelete(gone) == o.delete(gone) == [True] * 40 + [False] * 2
    _same_graph(g.export(), o.export())
    Q = rng.uniform(-1, 1, (16, d)).astype(np.float32)
    assert _adds_agree(H, O, g, o, rng.uniform(-1, 1, (10, d)).astype(np.float32), 10**6, Q) == 10
    g.close()


# ---------------------------------------------------------------- batched insert
N_BATCH = 600
VARIANTS = [dict(screen=0, build_mw_max=0),        # k_batch_search without the fp16 screen
            dict(screen=1, build_mw_max=0),        # ... with it
            dict(screen=1, build_mw_max=1 << 30)]  # every launch narrow: k_batch_search_mw from build_expand 2


def _batch_inputs(d):
    rng = np.random.default_rng(100 + d)
    return _clustered(rng, N_BATCH, d), _clustered(rng, 32, d)


def _batch_graph(H, d, X, efc, m0, expand, **options):
    """the batched build of X in two calls; no dropped proposal (with drops the
    graph depends on the order the proposals arrive in)"""
    g = H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=_metric_fn(H, _metric_of(d)), Rng=7, build_mode=H.BUILD_BATCH,
                m0=m0, ef_construction=efc, heuristic=2, keep_pruned=1, build_expand=expand, **options)
    half = N_BATCH // 2
    g.add_arrays(np.arange(half), X[:half])
    g.add_arrays(np.arange(half, N_BATCH), X[half:])
    assert g.stats()["dropped_proposals"] == 0
    return g


BATCH_CASES = [(d, 40, 16, xw) for d in ALL_DIMS for xw in (1, 4)]
BATCH_CASES += [(48, 40, 16, 2), (48, 40, 16, 3)]
# the wider candidate lists (2, 4 and 8 registers)
BATCH_CASES += [(48, efc, 32, xw) for efc in (100, 200, 400) for xw in (1, 2, 3, 4)]


@pytest.mark.parametrize("d,efc,m0,expand", BATCH_CASES)
def test_batch_insert_kernel_set(H, O, d, efc, m0, expand):
    X, Q = _batch_inputs(d)
    o, first = None, None
    for options in VARIANTS:
        g = _batch_graph(H, d, X, efc, m0, expand, **options)
        ex = g.export()
        if o is None:
            first = ex
            o = O.Graph(metric=_metric_of(d), order=O.ORDER_DEV, M=8, M0=m0, Ml=0.25, EfSearch=32)
            o.import_graph(**ex)
            want = o.search(Q, 10, mode=O.MODE_BEAM, ef=32)
        else:
            _same_graph(ex, first)
        _same_results(*g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=32), *want)
        g.close()


# ---------------------------------------------------------------- repair delete
@pytest.mark.parametrize("d", [400, 2048])
def test_repair_delete_configs(H, O, d):
    X, Q = _batch_inputs(d)
    g = _batch_graph(H, d, X, 40, 16, 1)
    o = O.Graph(metric=_metric_of(d), order=O.ORDER_DEV, M=8, M0=16, Ml=0.25, EfSearch=32)
    ex0 = g.export()
    o.import_graph(**ex0)
    top = ex0["deg"].shape[0] - 1
    rng = np.random.default_rng(d)
    gone = [int(ex0["keys"][ex0["entry"][top]])] + [int(x) for x in rng.permutation(N_BATCH)]
    gone = list(dict.fromkeys(gone))[:80]
    assert g.BatchDelete(gone) == o.delete(gone, mode=1, heuristic=2, keep_pruned=1) == [True] * 80
    _same_graph(g.export(), o.export())
    _same_results(*g.search_arrays(Q, 10, mode=H.MODE_EXACT), *o.search(Q, 10, mode=O.MODE_EXACT))
    _same_results(*g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=32), *o.search(Q, 10, mode=O.MODE_BEAM, ef=32))
    g.close()
