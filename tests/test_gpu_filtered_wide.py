"""GPU: the filtered beam search past 128 results (option filter_wide; beam.hpp
k_search_beam_filt_wide, R in LDS and merged once per step).  The semantics are
those of tests/filtered_ref.py at any result width, so everything here is
compared with it (or with the oracle's unfiltered search) bit for bit through
test_gpu_filtered.py's Case.check: keys, counts, distance bits, padding and the
number of expansions.
"""
import numpy as np
import pytest

from tests.test_gpu_filtered import B, D, N, Case, _batched, _with
from tests.test_gpu_filtered import dangling  # noqa: F401  (fixture)
from tests.test_gpu_parity import _clustered, _same_results

pytestmark = pytest.mark.gpu

ES = (129, 192, 256, 512, 513, 1024, 2048)


@pytest.fixture(scope="module")
def built(H, O):
    """one batched N x D graph per metric (m0 32), filter_wide on, with filters
    of 100 / 50 / 5 / 1 % random rows"""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(171 + metric)
        X = _clustered(rng, N, D)
        Q = _clustered(rng, B, D)
        c = Case(H, O, _batched(H, metric, np.arange(N) * 3 + 1, X), metric, Q, M=16, M0=32)
        c.g.set_option("filter_wide", 1)
        c.masks = {100: np.ones(N, bool)}
        for pct in (50, 5, 1):
            c.masks[pct] = rng.random(N) < pct / 100.0
        c.filters = {pct: c.mask_filter(m) for pct, m in c.masks.items()}
        out[metric] = c
    yield out
    for c in out.values():
        c.g.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("pct", [100, 50, 5, 1])
@pytest.mark.parametrize("E", ES)
def test_restatement_parity(built, metric, pct, E):
    """the first width past the register list, one that is no multiple of 64, the
    64 R boundaries of the merge's search and the maximum; at 50 % R fills, at
    1 % (about 60 rows) it never does"""
    c = built[metric]
    old = _with(c.g, screen=1, vis_compact=1)
    try:
        # (the kernels without the fp16 screen and the 32-bit visited set: at one width, the answers are cached)
        for screen, compact in ((1, 1), (0, 1), (1, 0), (0, 0)) if E == 256 else ((1, 1),):
            _with(c.g, screen=screen, vis_compact=compact)
            for W in (E, 2048):
                for k in (E, 10):
                    c.check(pct, [c.masks[pct]] * B, c.filters[pct], k, E, W)
    finally:
        _with(c.g, **old)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("E", [256, 512, 2048])
def test_against_the_oracle_alone(O, built, metric, E):
    """every row allowed, W = E: the oracle's unfiltered beam search at ef = E"""
    c = built[metric]
    want = c.o.search(c.Q, E, mode=O.MODE_BEAM, ef=E)
    for flt in (c.filters[100], None):
        _same_results(*c.g.search_filtered_arrays(c.Q, E, flt, ef=E, route=E), *want)


@pytest.mark.parametrize("metric", [0, 1])
def test_duplicated_rows_with_different_bits(H, O, metric):
    """test_gpu_filtered.py's recipe at E = 256: 1500 rows are exact copies of
    other rows and of each pair one is allowed -- equal distances inside a
    step's buffer and against both lists, the merge's sequential path"""
    rng = np.random.default_rng(23 + metric)
    X = _clustered(rng, N, D)
    src = rng.choice(4500, 1500, replace=False)
    X[4500:] = X[src]
    Q = _clustered(rng, B, D)
    Q[:8] = X[src[:8]]
    c = Case(H, O, _batched(H, metric, np.arange(N) * 5 + 2, X, seed=4), metric, Q, M=16, M0=32)
    try:
        c.g.set_option("filter_wide", 1)
        first = np.ones(N, bool)
        first[4500:] = False  # the copies are not allowed
        second = ~first
        second[:4500] = rng.random(4500) < 0.5
        second[src] = False  # the originals of the copies are not
        for name, m in (("first", first), ("second", second)):
            f = c.mask_filter(m)
            for W in (256, 1024):
                c.check(name, [m] * B, f, 256, 256, W)
            f.close()
    finally:
        c.g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_forgetting_visited_sets(built, metric):
    """a 32-bit visited set far smaller than the route list: every query forgets,
    and rows come back to both lists; results and expansions are the restatement's"""
    c = built[metric]
    old = _with(c.g, vis_compact=0, vis_entries=256)
    try:
        for pct in (50, 5):
            c.g.reset_stats()
            c.g.search_filtered_arrays(c.Q, 10, c.filters[pct], ef=512, route=2048)
            assert c.g.stats()["visited_resets"] >= 4 * B
            c.check(pct, [c.masks[pct]] * B, c.filters[pct], 512, 512, 2048)
    finally:
        c.g.set_option("vis_entries", 0)
        c.g.set_option("vis_compact", old["vis_compact"])


@pytest.mark.parametrize("metric", [0, 1])
def test_deleted_rows_inside_the_route_list(dangling, metric):  # noqa: F811
    """the 1500-row graph whose live rows keep their edges to the deleted quarter"""
    c = dangling[metric]
    old = _with(c.g, filter_wide=1)
    try:
        for name, flt in (("every", c.every), ("none", None)):
            gk, _, _ = c.check((name, metric), [np.ones(c.n, bool)] * len(c.Q), flt, 256, 256, 1024)
            assert not (set(gk[gk >= 0].tolist()) & c.gone)
    finally:
        _with(c.g, **old)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("per_query", [False, True])
def test_filtered_range_search_beam_mode(H, built, metric, per_query):
    """ef = 512 against the restatement's list cut at the radius, which sits at
    each query's 200th allowed distance: more than 128 hits a query"""
    c = built[metric]
    pcts = [(50, 100)[b % 2] for b in range(B)] if per_query else [50] * B
    masks = [c.masks[p] for p in pcts]
    rad = np.array([np.sort(c.T[b][masks[b]])[199] for b in range(B)], np.float32)
    rk, rd, rn, _ = c.ref(("range", per_query), masks, 512, 512, 2048)
    keep = [rd[b, : rn[b]] <= rad[b] for b in range(B)]
    assert min(int(m.sum()) for m in keep) > 128
    flts = [c.filters[p] for p in pcts] if per_query else c.filters[50]
    lims, keys, dist = c.g.range_search_arrays(c.Q, rad, filters=flts, mode=H.MODE_BEAM, ef=512, route=2048)
    assert lims.tolist() == np.concatenate([[0], np.cumsum([m.sum() for m in keep])]).tolist()
    assert keys.tolist() == np.concatenate([rk[b, : rn[b]][keep[b]] for b in range(B)]).tolist()
    want = np.concatenate([rd[b, : rn[b]][keep[b]] for b in range(B)])
    assert np.array_equal(dist.view(np.uint32), want.view(np.uint32))


def test_interface(H, built):
    c = built[0]
    g, Q, f = c.g, c.Q, c.filters[50]
    assert g.get_option("filter_wide") == 1
    # up to 128 results the option changes nothing: the same results and counters
    runs = {}
    for on in (1, 0):
        g.set_option("filter_wide", on)
        for ef, W in ((64, 200), (128, 2048)):
            g.reset_stats()
            runs[on, ef] = (g.search_filtered_arrays(Q, 10, f, ef=ef, route=W), g.stats()["search_expansions"])
    for ef in (64, 128):
        _same_results(*runs[1, ef][0], *runs[0, ef][0])
        assert runs[1, ef][1] == runs[0, ef][1] > 0
    # option off: the refusal as it was, for the search and the range search's beam mode
    for call in (lambda ef: g.search_filtered_arrays(Q, 10, f, ef=ef),
                 lambda ef: g.range_search_arrays(Q, 1.0, filters=f, mode=H.MODE_BEAM, ef=ef)):
        with pytest.raises(H.HnswError, match=r"filtered search supports max\(ef,k\) <= 128") as e:
            call(129)
        assert e.value.code == H._lib.EUNSUPPORTED
    g.set_option("filter_wide", 1)
    for call in (lambda: g.search_filtered_arrays(Q, 10, f, ef=2049), lambda: g.search_filtered_arrays(Q, 2049, f),
                 lambda: g.range_search_arrays(Q, 1.0, filters=f, mode=H.MODE_BEAM, ef=2049)):
        with pytest.raises(H.HnswError, match=r"filtered search supports max\(ef,k\) <= 2048") as e:
            call()
        assert e.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match="filter_wide must be 0 or 1"):
        g.set_option("filter_wide", 2)
    # the LDS budget names the result width; an automatically sized 32-bit set gives way instead
    old = _with(g, vis_compact=0, vis_entries=8192)
    try:
        with pytest.raises(H.HnswError, match=r"LDS budget exceeded \(route=2048, results=2048, vis_entries=8192\)"):
            g.search_filtered_arrays(Q, 10, f, ef=2048, route=2048)
        g.set_option("vis_entries", 0)
        c.check(50, [c.masks[50]] * B, f, 10, 2048, 2048)
    finally:
        g.set_option("vis_entries", 0)
        g.set_option("vis_compact", old["vis_compact"])
