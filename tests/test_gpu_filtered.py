"""GPU: the filtered beam search (beam.hpp k_search_beam_filt; mhnsw_filter_*,
mhnsw_search_filtered*; Graph.Filter / search_filtered_arrays; hnsw_amd.facets).

The semantics are restated in plain Python (tests/filtered_ref.py, pinned to
the oracle by tests/test_filtered_ref.py): every result is compared with it bit
for bit -- keys, counts, distance bits -- and so is the number of expansions,
which shows that the kernel really stops early and really goes wide.  With
every row allowed the search is the unfiltered beam search (the oracle's and
the engine's own), and with at most 128 rows allowed and a route list that
never fills it is the oracle's whole list with the other keys removed.
"""
import numpy as np
import pytest

from tests import filtered_ref as FR
from tests.test_gpu_parity import _clustered, _metric_fn, _same_results

pytestmark = pytest.mark.gpu

N, D, B = 6000, 40, 32
WS = (64, 65, 200, 1024, 2048)
EFS = (1, 10, 64, 65, 128)


def _with(g, **opts):
    old = {k: g.get_option(k) for k in opts}
    for k, v in opts.items():
        g.set_option(k, v)
    return old


class Case:
    """a graph, its export mirrored into the oracle and the restatement, the
    queries' distance table, and a cache of the restatement's answers"""

    def __init__(self, H, O, g, metric, Q, **okw):
        self.g, self.Q, self.metric = g, Q, metric
        self.ex = g.export()
        self.o = O.Graph(metric=metric, order=O.ORDER_DEV, Ml=0.25, EfSearch=64, **okw)
        self.o.import_graph(**self.ex)
        self.rg = FR.Graph(self.ex)
        self.T = FR.distance_table(O, self.ex, metric, Q)
        self.keys = self.ex["keys"]
        self.n = len(self.keys)
        self._memo = {}

    def mask_filter(self, mask):
        return self.g.Filter(self.keys[np.asarray(mask, bool)].tolist())

    def ref(self, name, masks, k, ef, route):
        """the restatement for per-query masks (cached under `name`); one run at
        k = E serves every k <= E of the same (E, W)"""
        E, W = max(ef, k), max(route, ef, k)
        key = (name, E, W)
        if key not in self._memo:
            self._memo[key] = FR.search_batch(self.rg, self.T, masks, self.keys, E, E, W)
        rk, rd, rn, nx = self._memo[key]
        return rk[:, :k], rd[:, :k], np.minimum(rn, k), nx

    def check(self, name, masks, filters, k, ef, route, expansions=True):
        self.g.reset_stats()
        got = self.g.search_filtered_arrays(self.Q, k, filters, ef=ef, route=route)
        xs = self.g.stats()["search_expansions"]
        rk, rd, rn, nx = self.ref(name, masks, k, ef, route)
        _same_results(*got, rk, rd, rn)
        for b in range(len(self.Q)):  # the padding
            assert (got[0][b, got[2][b]:] == -1).all() and np.isposinf(got[1][b, got[2][b]:]).all(), b
        if expansions:
            assert xs == nx, (name, k, ef, route, xs, nx)
        return got


def _batched(H, metric, keys, X, seed=5):
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=seed, build_mode=H.BUILD_BATCH,
                ef_construction=100, heuristic=2, m0=32)
    g.add_arrays(keys, X)
    return g


@pytest.fixture(scope="module")
def built(H, O):
    """one batched graph per metric with filters of 100 / 50 / 5 / 1 % random rows"""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(71 + metric)
        X = _clustered(rng, N, D)
        Q = _clustered(rng, B, D)
        c = Case(H, O, _batched(H, metric, np.arange(N) * 3 + 1, X), metric, Q, M=16, M0=32)
        c.masks = {100: np.ones(N, bool)}
        for pct in (50, 5, 1):
            c.masks[pct] = rng.random(N) < pct / 100.0
        c.filters = {pct: c.mask_filter(m) for pct, m in c.masks.items()}
        out[metric] = c
    yield out
    for c in out.values():
        c.g.close()


@pytest.fixture(scope="module")
def dangling(H, O):
    """per metric: the 1500 x 24 uniform reference-semantics graph with a quarter
    of the keys deleted -- the live rows keep their edges to the deleted ones, so
    deleted rows sit inside the route list"""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(17)
        n, d = 1500, 24
        X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
        Q = rng.uniform(-1, 1, (B, d)).astype(np.float32)
        keys = np.arange(n, dtype=np.int64) * 3 + 1
        g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), Rng=11)
        g.add_arrays(keys, X)
        every = g.Filter(keys.tolist())  # before the deletes: the bits stay set on the deleted rows
        assert all(g.BatchDelete([int(x) for x in keys[::4]]))
        c = Case(H, O, g, metric, Q, M=8)
        c.every = every
        c.gone = set(int(x) for x in keys[::4])
        out[metric] = c
    yield out
    for c in out.values():
        c.g.close()


# ---------------------------------------------------------------- 1. restatement parity
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("pct", [100, 50, 5, 1])
def test_restatement_parity(built, metric, pct):
    c = built[metric]
    masks = [c.masks[pct]] * B
    old = _with(c.g, screen=1, vis_compact=1)
    try:
        for screen in (1, 0):
            for compact in (1, 0):
                _with(c.g, screen=screen, vis_compact=compact)
                for W in WS:
                    for ef in EFS:
                        for k in sorted({1, 10, ef}):
                            c.check(pct, masks, c.filters[pct], k, ef, W)
    finally:
        _with(c.g, **old)


def test_the_walk_stops_early_and_goes_wide(built):
    """what the expansion counts of the parity test show, said directly: at
    equal route width, the fewer rows match the longer the walk, and with every
    row allowed the route width does not matter at all"""
    c = built[0]
    xs = {pct: c.ref(pct, [c.masks[pct]] * B, 10, 64, 2048)[3] for pct in (100, 50, 5, 1)}
    assert xs[100] < xs[50] < xs[5] < xs[1], xs
    assert c.ref(100, [c.masks[100]] * B, 10, 64, 64)[3] == xs[100]


# ---------------------------------------------------------------- 2. unfiltered equivalence
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("ef", [10, 64, 128])
def test_unfiltered_equivalence(H, O, built, metric, ef):
    c = built[metric]
    for k in sorted({1, 10, ef}):
        want = c.o.search(c.Q, k, mode=O.MODE_BEAM, ef=ef)
        own = c.g.search_arrays(c.Q, k, mode=H.MODE_BEAM, ef=ef)
        _same_results(*own, *want)
        for W in (ef, 2048):
            for flt in (c.filters[100], None):
                got = c.g.search_filtered_arrays(c.Q, k, flt, ef=ef, route=W)
                _same_results(*got, *want)
                _same_results(*got, *own)


# ---------------------------------------------------------------- 3. against the C oracle alone
@pytest.fixture(scope="module")
def small(H, O):
    """the 1500-row uniform graph (M 16, the reference's build, no deletions)"""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(19)
        n, d = 1500, 24
        X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
        Q = rng.uniform(-1, 1, (B, d)).astype(np.float32)
        keys = np.arange(n, dtype=np.int64) * 3 + 1
        g = H.Graph(M=16, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), Rng=11)
        g.add_arrays(keys, X)
        o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, Ml=0.25, EfSearch=20)
        o.import_graph(**g.export())
        whole = o.search(Q, 2048, mode=O.MODE_BEAM, ef=2048)
        assert (whole[2] < 2048).all()  # neither list is ever bounded
        out[metric] = (g, keys, Q, whole)
    yield out
    for g, *_ in out.values():
        g.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("allowed", [128, 40, 1])
def test_against_the_oracle_alone(small, metric, allowed):
    g, keys, Q, (wk, wd, wn) = small[metric]
    rng = np.random.default_rng(allowed)
    chosen = set(int(x) for x in rng.choice(keys, allowed, replace=False))
    f = g.Filter(sorted(chosen))
    try:
        assert f.count() == allowed
        for k in (1, 10, 128):
            gk, gd, gn = g.search_filtered_arrays(Q, k, f, ef=128, route=2048)
            for b in range(B):
                keep = [i for i in range(wn[b]) if int(wk[b, i]) in chosen][:k]
                assert gn[b] == len(keep), (b, k)
                assert gk[b, : gn[b]].tolist() == wk[b, keep].tolist(), (b, k)
                assert np.array_equal(gd[b, : gn[b]].view(np.uint32), wd[b, keep].view(np.uint32)), (b, k)
    finally:
        f.close()


# ---------------------------------------------------------------- 4. edges
def test_no_row_allowed(built):
    c = built[0]
    f = c.g.Filter([])
    try:
        assert f.count() == 0
        for W in (64, 2048):
            gk, gd, gn = c.check("none", [np.zeros(N, bool)] * B, f, 10, 64, W)
            assert (gn == 0).all() and (gk == -1).all() and np.isposinf(gd).all()
    finally:
        f.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_one_row_and_word_edges(built, metric):
    """one allowed row; rows at ids 0, 31, 32 and N - 1 (N is no multiple of 32)"""
    c = built[metric]
    assert N % 32 != 0
    for name, rows in (("one", [4321]), ("edges", [0, 31, 32, N - 1])):
        m = np.zeros(N, bool)
        m[rows] = True
        f = c.mask_filter(m)
        try:
            assert f.count() == len(rows)
            for W in (64, 2048):
                c.check((name, metric), [m] * B, f, 10, 64, W)
        finally:
            f.close()


def test_word_edges_are_reached(small):
    """where a route list holds the whole graph, every allowed row is reached"""
    g, keys, Q, _ = small[0]
    n = len(keys)
    assert n % 32 != 0
    rows = [0, 31, 32, n - 1]
    f = g.Filter([int(keys[r]) for r in rows])
    try:
        gk, gd, gn = g.search_filtered_arrays(Q, 10, f, ef=64, route=2048)
        assert (gn == 4).all()
        for b in range(B):
            assert sorted(gk[b, :4].tolist()) == sorted(int(keys[r]) for r in rows)
            assert (np.diff(gd[b, :4]) >= 0).all()
    finally:
        f.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_duplicated_rows_with_different_bits(H, O, metric):
    """1500 rows are exact copies of other rows, and of each pair one is
    allowed: ties at both bounds, and the merge's sequential path"""
    rng = np.random.default_rng(23 + metric)
    X = _clustered(rng, N, D)
    src = rng.choice(4500, 1500, replace=False)
    X[4500:] = X[src]
    Q = _clustered(rng, B, D)
    Q[:8] = X[src[:8]]
    c = Case(H, O, _batched(H, metric, np.arange(N) * 5 + 2, X, seed=4), metric, Q, M=16, M0=32)
    try:
        first = np.ones(N, bool)
        first[4500:] = False  # the copies are not allowed
        second = ~first
        second[: 4500] = rng.random(4500) < 0.5
        second[src] = False  # the originals of the copies are not
        for name, m in (("first", first), ("second", second)):
            f = c.mask_filter(m)
            for ef, W in ((1, 64), (10, 64), (64, 64), (64, 200), (128, 1024)):
                c.check(name, [m] * B, f, min(ef, 10), ef, W)
            f.close()
    finally:
        c.g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_entry_allowed_and_not(built, metric):
    """the layer-0 entry of a query is where its descent ends: exactly those
    rows allowed, then all rows but those"""
    c = built[metric]
    ids = {FR.descend(c.rg, c.T[b].tolist())[0] for b in range(B)}
    only = np.zeros(N, bool)
    only[sorted(ids)] = True
    for name, m in (("entry", only), ("not-entry", ~only)):
        f = c.mask_filter(m)
        try:
            for ef, W in ((1, 64), (10, 200), (64, 64)):
                c.check((name, metric), [m] * B, f, min(ef, 10), ef, W)
        finally:
            f.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_deleted_rows_are_never_returned(H, O, dangling, metric):
    """bits set on deleted rows: on the dangling-edge graph (deleted rows inside
    the route list) and after the batched repair"""
    c = dangling[metric]
    every = np.ones(c.n, bool)
    f = c.every
    half = np.random.default_rng(3).random(c.n) < 0.5
    fh = c.mask_filter(half)
    try:
        assert f.count() == c.n - len(c.gone)
        for name, m, flt in (("every", every, f), ("half", half, fh), ("none", every, None)):
            for ef, W in ((10, 64), (64, 200), (128, 2048)):
                gk, _, _ = c.check((name, metric), [m] * B, flt, min(ef, 10), ef, W)
                assert not (set(gk[gk >= 0].tolist()) & c.gone)
    finally:
        fh.close()


def test_deleted_rows_after_batched_repair(H, O):
    rng = np.random.default_rng(5)
    X = _clustered(rng, N, D)
    Q = _clustered(rng, B, D)
    g = H.Graph(M=12, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=3, build_mode=H.BUILD_BATCH,
                ef_construction=80, heuristic=2, m0=24)
    g.add_arrays(np.arange(N), X)
    f = g.Filter(range(0, N, 2))  # created before the deletes: bits stay set on the rows deleted below
    gone = list(range(0, N, 6))
    g.BatchDelete(gone)
    c = Case(H, O, g, 0, Q, M=12, M0=24)
    try:
        assert f.count() == N // 2 - len(gone)
        m = np.zeros(N, bool)
        m[::2] = True
        for ef, W in ((10, 64), (64, 1024)):
            gk, _, _ = c.check("repair", [m] * B, f, 10, ef, W)
            assert not (set(gk[gk >= 0].tolist()) & set(gone))
    finally:
        g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_forgetting_visited_sets(built, metric):
    """32-bit visited sets far smaller than the route list: every step forgets;
    the results and the expansions are still the restatement's, which never forgets"""
    c = built[metric]
    old = _with(c.g, vis_compact=0, vis_entries=0)
    try:
        for ve in (64, 256):
            c.g.set_option("vis_entries", ve)
            for pct in (50, 5):
                for ef, W in ((10, 200), (64, 1024)):
                    c.g.reset_stats()
                    c.g.search_filtered_arrays(c.Q, 10, c.filters[pct], ef=ef, route=W)
                    # a walk forgets once it has met 3/4 of `ve` rows.  To collect 64 of the
                    # 5 % it must meet 1280 rows or more, so every query forgets, several
                    # times; the short walks (half the rows match) forget now and then
                    resets = c.g.stats()["visited_resets"]
                    assert resets >= (4 * B if (pct, ef) == (5, 64) else 1), (ve, pct, ef, W, resets)
                    c.check(pct, [c.masks[pct]] * B, c.filters[pct], 10, ef, W)
    finally:
        c.g.set_option("vis_entries", 0)
        _with(c.g, **{k: v for k, v in old.items() if k != "vis_entries"})


def test_mixed_batch_and_single_query(built):
    """a batch mixing three filters and "every live row"; B = 1 equals the same
    query inside the batch"""
    c = built[1]
    pcts = [(50, 5, 1, None)[b % 4] for b in range(B)]
    masks = [None if p is None else c.masks[p] for p in pcts]
    flts = [None if p is None else c.filters[p] for p in pcts]
    for ef, W in ((10, 64), (64, 1024)):
        gk, gd, gn = c.check("mixed", masks, flts, 10, ef, W)
        for b in (0, 1, 2, 3, 30):
            c.g.reset_stats()
            sk, sd, sn = c.g.search_filtered_arrays(c.Q[b], 10, flts[b], ef=ef, route=W)
            _same_results(sk, sd, sn, gk[b:b + 1], gd[b:b + 1], gn[b:b + 1])


# ---------------------------------------------------------------- 5. lifecycle and errors
def test_lifecycle(H, O):
    rng = np.random.default_rng(41)
    n0, n1, d = 700, 1500, 24
    X = _clustered(rng, n1, d)
    g = _batched(H, 0, np.arange(n0), X[:n0])
    try:
        f = g.Filter(range(n0))
        assert f.count() == n0
        assert g.get_option("capacity") < n1
        g.add_arrays(np.arange(n0, n1), X[n0:])  # the row capacity grows: the bitmap grows zero-filled
        assert g.get_option("capacity") >= n1
        assert f.count() == n0
        Q = X[n0:n0 + B]  # queries ON rows added after the filter: their own keys are the nearest
        own = np.arange(n0, n0 + B)
        gk, _, gn = g.search_filtered_arrays(Q, 5, f, ef=64, route=2048)
        assert (gn == 5).all() and (gk < n0).all()
        f.add(own.tolist())
        assert f.count() == n0 + B
        gk, gd, gn = g.search_filtered_arrays(Q, 5, f, ef=64, route=2048)
        assert gk[:, 0].tolist() == own.tolist()
        f.remove(own[:4].tolist())
        assert f.count() == n0 + B - 4
        gk, _, _ = g.search_filtered_arrays(Q, 5, f, ef=64, route=2048)
        assert not (set(gk[:4].ravel().tolist()) & set(own[:4].tolist()))
        assert gk[4:, 0].tolist() == own[4:].tolist()
        f.add([10 ** 9])  # an absent key is ignored
        assert f.count() == n0 + B - 4
        # destroy, then EINVAL -- from the handle and from the engine
        fid = f.id
        f.close()
        with pytest.raises(H.HnswError, match=f"unknown filter {fid}") as e:
            f.count()
        assert e.value.code == H._lib.EINVAL
        fo = np.full(B, fid, np.int32)
        ok, od, on = np.zeros((B, 5), np.int64), np.zeros((B, 5), np.float32), np.zeros(B, np.int32)
        import ctypes as C
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        rc = H.load().mhnsw_search_filtered(g._h, P(np.ascontiguousarray(Q), C.c_float), B, d, 5, 64, 0,
                                            P(fo, C.c_int32), P(ok, C.c_int64), P(od, C.c_float), P(on, C.c_int32))
        assert rc == H._lib.EINVAL
        assert H.load().mhnsw_last_error(g._h).decode() == f"unknown filter {fid}"
        n = C.c_int64()
        assert H.load().mhnsw_filter_count(g._h, fid, C.byref(n)) == H._lib.EINVAL
        assert H.load().mhnsw_filter_destroy(g._h, fid) == H._lib.EINVAL
        # Import drops every filter: the row ids are the import's
        f2 = g.Filter(range(0, n1, 3))
        ex = g.export()
        g2 = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance)
        f3 = g2.Filter([])
        g2.import_graph(**ex)
        with pytest.raises(H.HnswError, match=f"unknown filter {f3.id}"):
            f3.count()
        with pytest.raises(H.HnswError, match=f"unknown filter {f3.id}"):
            g2.search_filtered_arrays(Q, 5, f3)
        f4 = g2.Filter(range(0, n1, 3))
        _same_results(*g2.search_filtered_arrays(Q, 5, f4, ef=64), *g.search_filtered_arrays(Q, 5, f2, ef=64))
        data = g.export_bytes()
        g2.import_bytes(data)
        with pytest.raises(H.HnswError, match=f"unknown filter {f4.id}"):
            f4.count()
        g2.close()
        # a filter of another graph, and the wrong number of filters
        with pytest.raises(H.HnswError, match="filter of another graph"):
            g.search_filtered_arrays(Q, 5, f4)
        with pytest.raises(H.HnswError, match="filters for"):
            g.search_filtered_arrays(Q, 5, [f2] * 3)
    finally:
        g.close()


def test_errors_and_defaults(H, built):
    c = built[0]
    g, Q, f = c.g, c.Q, c.filters[50]
    with pytest.raises(H.HnswError, match=r"filtered search supports max\(ef,k\) <= 128") as e:
        g.search_filtered_arrays(Q, 10, f, ef=129)
    assert e.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match=r"filtered search supports max\(ef,k\) <= 128"):
        g.search_filtered_arrays(Q, 129, f, ef=10)
    with pytest.raises(H.HnswError, match=r"filtered search supports route <= 2048") as e:
        g.search_filtered_arrays(Q, 10, f, ef=64, route=2049)
    assert e.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match="k must be greater than 0"):
        g.search_filtered_arrays(Q, 0, f)
    # ef <= 0 is EfSearch; route <= 0 is the option filter_route (default 1024); a route below max(ef, k) is raised
    assert g.get_option("filter_route") == 1024
    m = [c.masks[50]] * B
    _same_results(*g.search_filtered_arrays(Q, 10, f), *c.ref(50, m, 10, 64, 1024)[:3])
    _same_results(*g.search_filtered_arrays(Q, 10, f, ef=64, route=3), *c.ref(50, m, 10, 64, 64)[:3])
    old = _with(g, filter_route=200)
    try:
        _same_results(*g.search_filtered_arrays(Q, 10, f, ef=10), *c.ref(50, m, 10, 10, 200)[:3])
    finally:
        _with(g, **old)
    for bad in (0, 2049):
        with pytest.raises(H.HnswError, match=r"filter_route must be in \[1, 2048\]"):
            g.set_option("filter_route", bad)
    # the LDS budget: an explicit visited set that does not fit next to the route list is refused on the host
    old = _with(g, vis_compact=0, vis_entries=32768)
    try:
        with pytest.raises(H.HnswError, match="LDS budget exceeded") as e:
            g.search_filtered_arrays(Q, 10, f, ef=64, route=1024)
        assert e.value.code == H._lib.EUNSUPPORTED
    finally:
        g.set_option("vis_entries", 0)
        g.set_option("vis_compact", old["vis_compact"])
    _same_results(*g.search_filtered_arrays(Q, 10, f), *c.ref(50, m, 10, 64, 1024)[:3])


def test_empty_index(H):
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance)
    try:
        f = g.Filter([1, 2, 3])
        assert f.count() == 0
        gk, gd, gn = g.search_filtered_arrays(np.zeros((3, 8), np.float32), 5, f)
        assert (gn == 0).all()
        assert g.SearchFiltered(np.zeros(8, np.float32), 5, None) == []
    finally:
        g.close()


@pytest.mark.parametrize("kind", ["str", "float"])
def test_string_and_float_keys(H, kind):
    """keys travel encoded like every other key.  With at most 128 rows allowed,
    ef 128 and a route list wider than the graph, neither list is ever bounded:
    the result is the graph's own unfiltered list (k = ef = 512 > n) with the
    other keys removed"""
    rng = np.random.default_rng(8)
    n, d = 300, 16
    X = rng.normal(size=(n, d)).astype(np.float32)
    names = [f"doc-{i:04d}" for i in range(n)] if kind == "str" else [i * 0.5 - 20.0 for i in range(n)]
    g = H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=H.EuclideanDistance, Rng=2)
    try:
        g.BatchAdd([H.MakeNode(k, x) for k, x in zip(names, X)])
        allowed = set(names[1::3])
        f = g.Filter(sorted(allowed) + ["no such doc" if kind == "str" else 1e9])
        assert f.count() == len(allowed) == 100

        def check():
            for i in (1, 2, 77):
                whole = [x.Key for x in g.Search(X[i], 512, mode=H.MODE_BEAM)]
                assert len(whole) < 512
                res = g.SearchFiltered(X[i], 5, f, ef=128, route=512)
                assert [r.Key for r in res] == [k for k in whole if k in allowed][:5]
                assert all(np.array_equal(r.Value, X[names.index(r.Key)]) for r in res)
                assert res, "the walk reaches allowed rows"

        check()
        f.remove([names[1], names[4]])
        allowed -= {names[1], names[4]}
        assert f.count() == 98
        check()
        f.add([names[2], names[77]])
        allowed |= {names[2], names[77]}
        assert f.count() == 100
        check()
    finally:
        g.close()


def _host_filtered(H, g, Q, filter_of, k=5):
    """mhnsw_search_filtered with a raw filter_of -> its return code"""
    import ctypes as C

    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    Bq, d = Q.shape
    ok, od, on = np.zeros((Bq, k), np.int64), np.zeros((Bq, k), np.float32), np.zeros(Bq, np.int32)
    return H.load().mhnsw_search_filtered(g._h, P(np.ascontiguousarray(Q), C.c_float), Bq, d, k, 64, 0,
                                          P(np.ascontiguousarray(filter_of), C.c_int32), P(ok, C.c_int64),
                                          P(od, C.c_float), P(on, C.c_int32))


def test_device_search_then_add(H):
    """the ordering of test_gpu_streams.py: a filtered *_device search enqueued
    on a non-default stream, then an Add and a filter update, which must wait"""
    import torch

    rng = np.random.default_rng(4)
    n, d, Bq, k = 20000, 64, 4096, 10
    X = rng.normal(size=(n + 2000, d)).astype(np.float32)
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.EuclideanDistance, build_mode=H.BUILD_BATCH,
                ef_construction=64)
    try:
        g.add_arrays(np.arange(n), X[:n])
        f = g.Filter(range(0, n, 3))
        Qh = rng.normal(size=(Bq, d)).astype(np.float32)
        fo_h = np.where(np.arange(Bq) % 2 == 0, f.id, -1).astype(np.int32)
        want = g.search_filtered_arrays(Qh, k, [f if x >= 0 else None for x in fo_h], ef=64, route=256)
        Q = torch.tensor(Qh, device="cuda")
        fo = torch.tensor(fo_h, device="cuda")
        ok = torch.empty(Bq, k, dtype=torch.int64, device="cuda")
        od = torch.empty(Bq, k, dtype=torch.float32, device="cuda")
        on = torch.empty(Bq, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g.search_filtered_device(Q.data_ptr(), Bq, d, k, fo.data_ptr(), ok.data_ptr(), od.data_ptr(), on.data_ptr(),
                                 ef=64, route=256, stream=s.cuda_stream)
        g.add_arrays(np.arange(n, n + 2000), X[n:])  # must wait for the enqueued search
        f.add(range(n, n + 2000))
        g.BatchDelete(list(range(0, n, 7)))
        torch.cuda.synchronize()
        g.device_status()
        assert np.array_equal(on.cpu().numpy(), want[2])
        assert np.array_equal(ok.cpu().numpy(), want[0])
        assert np.array_equal(od.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
        # a filter id that names no filter reaches the kernel only here: reported by device_status
        for bad in (777, 5000, -2):  # a free slot, past the table, below "every live row" (the host path's EINVAL)
            fo.fill_(bad)
            on.fill_(99)
            g.search_filtered_device(Q.data_ptr(), Bq, d, k, fo.data_ptr(), ok.data_ptr(), od.data_ptr(),
                                     on.data_ptr(), ef=64, route=256, stream=s.cuda_stream)
            with pytest.raises(H.HnswError, match="unknown filter in filter_of") as e:
                g.device_status()
            assert e.value.code == H._lib.EINVAL
            assert (on.cpu().numpy() == 0).all()
            g.device_status()  # (cleared)
        with pytest.raises(H.HnswError, match="unknown filter -2"):
            H.load()  # (the host path names the entry)
            g._check(_host_filtered(H, g, Qh[:4], np.full(4, -2, np.int32)))
    finally:
        g.close()


# ---------------------------------------------------------------- 6. facets
def _catalogue(H, F, rng, n=400, d=16):
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=5)
    fg = F.FacetedGraph(g, F.MemoryFacetStore())
    X = rng.normal(size=(n, d)).astype(np.float32)
    cats = ["Electronics", "Books", "Garden tools", "Toys"]
    fg.BatchAdd([F.NewFacetedNode(H.MakeNode(i, X[i]), [F.BasicFacet("category", cats[i % 4]),
                                                         F.BasicFacet("price", float(10 + (i * 37) % 500))])
                 for i in range(n)])
    return fg, X


def test_facets_compat_is_the_literal_procedure(H):
    from hnsw_amd import facets as F

    rng = np.random.default_rng(12)
    fg, X = _catalogue(H, F, rng)
    g = fg.Graph
    try:
        cases = [([F.EqualityFilter("category", "Books")], 5, 2),
                 ([F.EqualityFilter("category", "Books"), F.RangeFilter("price", 100, 200)], 5, 3),
                 ([F.StringContainsFilter("category", "TOOLS")], 3, 0),
                 (None, 4, 2)]
        for filters, k, xf in cases:
            for q in X[:6] + 0.01:
                got = [n.Node.Key for n in fg.Search(q, filters, k, xf)]
                # search.go:15-88 by hand over g.Search
                wide = k * (xf if xf > 0 else 3)
                cand = g.Search(q, wide)
                match = lambda n: all(fg.Store.Get(n.Key)[0].MatchesFilter(f) for f in (filters or ()))  # noqa: E731
                found = [n for n in cand if match(n)]
                if len(found) < k and len(cand) == wide:
                    found += [n for n in g.Search(q, wide * 2)[wide:] if match(n)]
                found.sort(key=lambda n: g.Distance(n.Value, q))
                assert got == [n.Key for n in found[:k]], (filters, k, xf)
    finally:
        fg.close()
        g.close()


def test_facets_beam_is_the_filtered_search(H):
    from hnsw_amd import facets as F

    rng = np.random.default_rng(13)
    fg, X = _catalogue(H, F, rng)
    g = fg.Graph
    try:
        filters = [F.EqualityFilter("category", "Books"), F.RangeFilter("price", 100, 300)]
        keys = [n.Node.Key for n in fg.Store.Filter(filters)]
        assert 0 < len(keys) < 100
        f = g.Filter(keys)
        for q in X[:6] + 0.01:
            got = fg.Search(q, filters, 5, mode=F.MODE_BEAM, ef=64, route=512)
            wk, _, wn = g.search_filtered_arrays(q, 5, f, ef=64, route=512)
            assert [n.Node.Key for n in got] == wk[0, : wn[0]].tolist() and len(got) == 5
            assert all(n.MatchesAllFilters(filters) for n in got)
        # the device filter is cached per filter list, and rebuilt when the store changes
        assert len(fg._filters) == 1
        fid = next(iter(fg._filters.values()))[1].id
        fg.Search(X[0], [F.EqualityFilter("category", "Books"), F.RangeFilter("price", 100, 300)], 5, mode=F.MODE_BEAM)
        assert len(fg._filters) == 1 and next(iter(fg._filters.values()))[1].id == fid
        best = fg.Search(X[1] + 0.01, filters, 1, mode=F.MODE_BEAM, route=512)[0].Node.Key
        assert fg.Delete(best)
        assert fg.Search(X[1] + 0.01, filters, 1, mode=F.MODE_BEAM, route=512)[0].Node.Key != best
        # a filter object of another class has nothing to key a cache on: two predicates, one after
        # the other (the second may sit at the first's address), each get their own rows
        class PriceBelow:
            def __init__(self, limit):
                self.limit = limit

            def Name(self):
                return "price"

            def Matches(self, v):
                return v < self.limit

        for limit in (60.0, 400.0, 60.0):
            got = fg.Search(X[2] + 0.01, [PriceBelow(limit)], 5, mode=F.MODE_BEAM, route=512)
            assert got and all(n.GetFacet("price").Value() < limit for n in got)
            want = g.Filter([n.Node.Key for n in fg.Store.Filter([PriceBelow(limit)])])
            wk, _, wn = g.search_filtered_arrays(X[2] + 0.01, 5, want, route=512)
            assert [n.Node.Key for n in got] == wk[0, : wn[0]].tolist()
            want.close()
        assert len(fg._filters) == 1
        # an Import drops the engine's filters: the cached one is rebuilt, not reported
        assert len(fg.Search(X[3] + 0.01, filters, 5, mode=F.MODE_BEAM, route=512)) == 5
        stale = next(iter(fg._filters.values()))[1]
        g.import_bytes(g.export_bytes())
        got = fg.Search(X[3] + 0.01, filters, 5, mode=F.MODE_BEAM, route=512)
        assert len(got) == 5 and all(n.MatchesAllFilters(filters) for n in got)
        assert next(iter(fg._filters.values()))[1] is not stale
        stale.close()  # (closing a filter the engine has dropped leaves it closed)
        assert stale.id is None
        with pytest.raises(H.HnswError, match="unknown filter"):
            stale.count()
        # FacetError texts
        for mode in (F.MODE_COMPAT, F.MODE_BEAM):
            with pytest.raises(F.FacetError) as e:
                fg.Search(X[0], filters, 0, 2, mode=mode)
            assert str(e.value) == "facet error: k must be greater than 0"
        agg = fg.GetFacetAggregations(X[0], None, ["category", "nope"], 10, 2)
        assert sum(agg["category"].Values.values()) == len(g.Search(X[0], 20)) and agg["nope"].Values == {}
    finally:
        fg.close()
        g.close()


def test_faceted_graph_of_the_reference(H):
    """facets_test.go TestFacetedGraph"""
    from hnsw_amd import facets as F

    g = H.NewGraph()
    fg = F.FacetedGraph(g, F.MemoryFacetStore())
    try:
        fg.Add(F.NewFacetedNode(H.MakeNode(1, [0.1, 0.2, 0.3]), [F.BasicFacet("category", "Electronics"),
                                                                 F.BasicFacet("price", 150.0)]))
        fg.Add(F.NewFacetedNode(H.MakeNode(2, [0.2, 0.3, 0.4]), [F.BasicFacet("category", "Electronics"),
                                                                 F.BasicFacet("price", 200.0)]))
        q = [0.1, 0.2, 0.3]
        for mode in (F.MODE_COMPAT, F.MODE_BEAM):
            res = fg.Search(q, None, 1, 2, mode=mode)
            assert [n.Node.Key for n in res] == [1]
        assert fg.Delete(1)
        for mode in (F.MODE_COMPAT, F.MODE_BEAM):
            res = fg.Search(q, None, 1, 2, mode=mode)
            assert [n.Node.Key for n in res] == [2]
    finally:
        fg.close()
        g.close()
