"""CPU: the plain-Python restatement of the filtered beam search
(tests/filtered_ref.py) is pinned to the oracle, which the GPU tests then use
it against (tests/test_gpu_filtered.py).

With every row allowed and none deleted the filtered search IS the unfiltered
beam search at ef = E, whatever the route width W >= E: an entry that the result
list R evicts is worse than R's worst entry from then on, so it is never
expanded, and the rows the bound of R keeps out of the route list L would not
have entered the unfiltered list either.  That ties the restatement to
oracle.c's beam search.  The arrival order of a step's neighbours must not
change results or expansion counts: both lists keep the best of everything
offered, and the offer test uses the bounds from before the step.
"""
import numpy as np
import pytest

from tests import filtered_ref as FR
from tests.test_gpu_parity import _clustered, _same_results

N, D, B = 4000, 32, 32


def _build(O, metric, X):
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, Ml=0.25, EfSearch=64, seed=3)
    o.add(np.arange(len(X)) * 3 + 1, X)
    return o


@pytest.fixture(scope="module")
def built(O):
    out = {}
    for metric in (O.COSINE, O.EUCLIDEAN):
        rng = np.random.default_rng(301 + metric)
        X = _clustered(rng, N, D)
        Q = _clustered(rng, B, D)
        o = _build(O, metric, X)
        ex = o.export()
        out[metric] = (o, ex, FR.Graph(ex), Q, FR.distance_table(O, ex, metric, Q))
    return out


@pytest.fixture(scope="module")
def tied(O):
    """1000 rows are exact copies of other rows: equal distances, distinct ids"""
    out = {}
    for metric in (O.COSINE, O.EUCLIDEAN):
        rng = np.random.default_rng(311 + metric)
        X = _clustered(rng, N, D)
        src = rng.choice(N - 1000, 1000, replace=False)
        X[N - 1000:] = X[src]
        Q = _clustered(rng, B, D)
        Q[:8] = X[src[:8]]
        o = _build(O, metric, X)
        ex = o.export()
        out[metric] = (ex, FR.Graph(ex), Q, FR.distance_table(O, ex, metric, Q))
    return out


def test_distance_table_is_the_oracles(O, built):
    o, ex, g, Q, T = built[O.COSINE]
    for b in (0, 7):
        for i in (0, 1, N // 2, N - 1):
            want = np.float32(O.distance(O.COSINE, O.ORDER_DEV, ex["vecs"][i], Q[b]))
            assert T[b, i].view(np.uint32) == want.view(np.uint32), (b, i)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("ef", [10, 64])
@pytest.mark.parametrize("wide", [1, 4])
def test_every_row_allowed_is_the_unfiltered_beam(O, built, metric, ef, wide):
    o, ex, g, Q, T = built[metric]
    for k in (1, 10):
        want = o.search(Q, k, mode=O.MODE_BEAM, ef=ef)
        for allow in (None, np.ones(N, bool)):
            gk, gd, gn, _ = FR.search_batch(g, T, [allow] * B, ex["keys"], k, ef, wide * ef)
            _same_results(gk, gd, gn, *want)


@pytest.mark.parametrize("metric", [0, 1])
def test_expansions_are_the_oracles_when_unfiltered(O, built, metric):
    """the count the GPU tests compare with the engine's counter: descent included"""
    o, ex, g, Q, T = built[metric]
    x0 = o.stats()[1]
    o.search(Q, 10, mode=O.MODE_BEAM, ef=64)
    want = o.stats()[1] - x0
    for route in (64, 256):
        assert FR.search_batch(g, T, [None] * B, ex["keys"], 10, 64, route)[3] == want


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("pct", [100, 20, 2])
def test_arrival_order_does_not_matter(O, tied, metric, pct):
    ex, g, Q, T = tied[metric]
    rng = np.random.default_rng(5 + pct)
    allow = rng.random(N) < pct / 100.0
    for ef, route in ((10, 10), (10, 40), (64, 64), (64, 256), (64, 2048)):
        plain = FR.search_batch(g, T, [allow] * B, ex["keys"], 10, ef, route)
        srng = np.random.default_rng(17)

        def shuffled(nb):
            nb.extend(nb[:3])  # (some rows arrive twice)
            srng.shuffle(nb)

        mixed = FR.search_batch(g, T, [allow] * B, ex["keys"], 10, ef, route, arrival=shuffled)
        _same_results(*mixed[:3], *plain[:3])
        assert mixed[3] == plain[3]


def test_filtered_results_are_allowed_sorted_and_bounded(O, built):
    o, ex, g, Q, T = built[0]
    rng = np.random.default_rng(9)
    allow = rng.random(N) < 0.1
    allowed_keys = set(ex["keys"][allow].tolist())
    gk, gd, gn, _ = FR.search_batch(g, T, [allow] * B, ex["keys"], 10, 64, 1024)
    assert (gn > 0).all() and gn.max() == 10  # (a route too narrow for a query returns fewer than k)
    for b in range(B):
        assert set(gk[b, : gn[b]].tolist()) <= allowed_keys
        assert (np.diff(gd[b, : gn[b]]) >= 0).all()
    # no row allowed: nothing returned, and the walk ends when the route list is exhausted
    gk, gd, gn, _ = FR.search_batch(g, T, [np.zeros(N, bool)] * B, ex["keys"], 10, 64, 64)
    assert (gn == 0).all() and (gk == -1).all() and np.isposinf(gd).all()
