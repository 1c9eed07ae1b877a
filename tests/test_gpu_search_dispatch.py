"""The search entry points reach the right kernel for every dimension
configuration (engine.hpp pick_cfg: ten pairs of lanes per row and float4 per
lane, each with its own group width G).  Every row-touching search kernel is
compiled once per configuration -- per configuration beam.hpp alone holds
k_search_beam for four register lists at three expansion widths with the fp16
screen on and off, the four-wave small-batch kernel, the LDS-list kernel at
three expansion widths, the filtered walk and the ordered path's descent
pre-pass -- and a wrong configuration behind a dimension, an LDS or register
budget that holds only for short rows, or an expansion width that breaks at
G = 1 or G = 8 shows at no other configuration than its own.

Two dimension lists: ALL_DIMS, one dimension per configuration (the
build-dispatch test's), and RAGGED_DIMS, the first dimension of each
configuration, where almost a whole stripe of the padded row is zeros and the
dimension is no multiple of 4.  ALL_DIMS run every family below, RAGGED_DIMS a
reduced set.  test_pitch_covers_the_table holds both lists to the table.

One small batch-built graph per (dimension, metric), exported once into the
oracle; rows 1 and 2 are exact duplicates (ties by id) and under cosine one row
and one query are all zero (NaN distances).  Every comparison is bit equality
-- keys, counts, distance bits -- against the oracle's restatement of the
search on that export, tests/filtered_ref.py for the filtered walk, or a list
already compared that way.  Every case also asserts what shows that it reached
the kernel it is there for.
"""
import numpy as np
import pytest

from tests import filtered_ref as FR
from tests.test_gpu_build_dispatch import ALL_DIMS
from tests.test_gpu_parity import _clustered, _metric_fn, _same_results
from tests.test_gpu_query_order import COUNTERS, _identical, _search

pytestmark = pytest.mark.gpu

# the first dimension of each configuration: the most padding
RAGGED_DIMS = [3, 65, 129, 257, 513, 769, 1025, 1537, 2049, 3073]

# engine.hpp pick_cfg, restated: (largest dimension, lanes per row, float4 per lane)
CFG_TABLE = [(64, 16, 1), (128, 32, 1), (256, 64, 1), (512, 64, 2), (768, 64, 3), (1024, 64, 4), (1536, 64, 6),
             (2048, 64, 8), (3072, 64, 12), (4096, 64, 16)]

N_ROWS = 1500  # more than twice the widest list that must fill and evict (ef 600)
B = 32
K = 10
ZERO_ROW, ZERO_QUERY = 5, 2  # cosine only


def _pitch(d):
    return next(lanes * 4 * v for hi, lanes, v in CFG_TABLE if d <= hi)


def _with(g, **opts):
    old = {k: g.get_option(k) for k in opts}
    for k, v in opts.items():
        g.set_option(k, v)
    return old


class Case:
    """a graph, its export mirrored into the oracle, the queries, and the caches of the
    oracle's and the filtered restatement's answers"""

    def __init__(self, H, O, d, metric):
        rng = np.random.default_rng(7000 * metric + d)
        n = N_ROWS
        X = _clustered(rng, n, d)
        X[2] = X[1]  # exact duplicates: equal distances, order by id
        Q = _clustered(rng, B, d)
        Q[0] = X[40]  # a stored row
        Q[1] = X[1]   # the duplicate pair's vector
        if metric == 0:
            X[ZERO_ROW] = 0.0    # NaN cosine distance: never listed
            Q[ZERO_QUERY] = 0.0  # NaN everywhere: no results
        self.H, self.O, self.d, self.metric, self.n, self.Q = H, O, d, metric, n, Q
        self.live_q = np.array([not (metric == 0 and b == ZERO_QUERY) for b in range(B)])
        self.g = H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=_metric_fn(H, metric), Rng=7, build_mode=H.BUILD_BATCH,
                         m0=16, ef_construction=40, heuristic=2, keep_pruned=1)
        half = n // 2
        self.g.add_arrays(np.arange(half) * 3 + 1, X[:half])
        self.g.add_arrays(np.arange(half, n) * 3 + 1, X[half:])
        self.g.set_option("beam_mw_max_b", 0)  # the one-wave kernels, unless a test says otherwise
        self.ex = self.g.export()
        self.keys = self.ex["keys"]
        assert self.ex["deg"].shape[0] >= 2  # there is a descent
        self.o = O.Graph(metric=metric, order=O.ORDER_DEV, M=8, M0=16, Ml=0.25, EfSearch=32)
        self.o.import_graph(**self.ex)
        self._oracle, self._fref, self._fr = {}, {}, None
        self.negs = [_clustered(rng, b % 3, d) for b in range(B)]

    def oracle(self, mode, k, ef, xw=1):
        """the oracle's lists; the register and the LDS list share an entry (the same
        lists at equal ef)"""
        key = (mode, k, ef, xw)
        if key not in self._oracle:
            self.o.set_search_expand(xw)
            try:
                self._oracle[key] = self.o.search(self.Q, k, mode=mode, ef=ef)
            finally:
                self.o.set_search_expand(1)
        return self._oracle[key]

    def beam(self, k, ef, Q=None):
        return self.g.search_arrays(self.Q if Q is None else Q, k, mode=self.H.MODE_BEAM, ef=ef)

    def full_counts(self, got, k):
        """every query that has distances returns k results"""
        assert (got[2][self.live_q] == k).all(), got[2]

    # -- the filtered walk: two filters, about 50 % and 5 % of the rows, and none, mixed per query
    def filtered_setup(self):
        if self._fr is None:
            rng = np.random.default_rng(31 + self.d)
            masks = []
            for pct in (50, 5):
                m = rng.random(self.n) < pct / 100.0
                m[[64, 95]] = True  # a row id that is a multiple of 32 and one that is 31 mod 32
                masks.append(m)
            self.masks = masks
            self.filters = [self.g.Filter(self.keys[m].tolist()) for m in masks]
            assert [f.count() for f in self.filters] == [int(m.sum()) for m in masks]
            pick = [b % 3 for b in range(B)]
            self.mask_of = [None if p == 2 else masks[p] for p in pick]
            self.filter_of = [None if p == 2 else self.filters[p] for p in pick]
            self._fr = (FR.Graph(self.ex), FR.distance_table(self.O, self.ex, self.metric, self.Q))
        return self._fr

    def filtered_ref(self, k, ef, route):
        """tests/filtered_ref.py over the export and the masks; one run at k = E serves every
        k <= E of the same (E, W)"""
        rg, T = self.filtered_setup()
        E, W = max(ef, k), max(route, ef, k)
        if (E, W) not in self._fref:
            self._fref[E, W] = FR.search_batch(rg, T, self.mask_of, self.keys, E, E, W)
        rk, rd, rn, nx = self._fref[E, W]
        return (rk[:, :k], rd[:, :k], np.minimum(rn, k)), nx

    def wide_descent_ref(self, k, ef, upper_ef):
        """the unfiltered search of tests/filtered_ref.py with a descent `upper_ef` wide"""
        rg, T = self.filtered_setup()
        return FR.search_batch(rg, T, [None] * B, self.keys, k, ef, ef, upper_ef=upper_ef)[:3]

    def filtered(self, k, ef, route):
        self.filtered_setup()
        return self.g.search_filtered_arrays(self.Q, k, self.filter_of, ef=ef, route=route)


@pytest.fixture(scope="module")
def cases(H, O):
    """case(d, metric): built on first use, kept for the module"""
    built = {}

    def case(d, metric):
        if (d, metric) not in built:
            built[d, metric] = Case(H, O, d, metric)
        return built[d, metric]

    yield case
    for c in built.values():
        c.g.close()


EVERY = [(d, m) for d in ALL_DIMS + RAGGED_DIMS for m in (0, 1)]
FULL = [(d, m) for d in ALL_DIMS for m in (0, 1)]
every_config = pytest.mark.parametrize("d,metric", EVERY)
full_set = pytest.mark.parametrize("d,metric", FULL)


def _ragged(d):
    return d in RAGGED_DIMS


# ---------------------------------------------------------------- the lists cover the table
def test_pitch_covers_the_table(H):
    """each list holds exactly one dimension per configuration, and the engine pads every one
    of them to that configuration's pitch"""
    for dims in (ALL_DIMS, RAGGED_DIMS):
        assert sorted(_pitch(d) for d in dims) == sorted(lanes * 4 * v for _, lanes, v in CFG_TABLE)
        assert len({_pitch(d) for d in dims}) == len(CFG_TABLE)
        for d in dims:
            g = H.Graph(M=4, Ml=0.25, EfSearch=8)
            g.add_arrays(np.arange(2), np.ones((2, d), np.float32))
            assert g.get_option("pitch") == _pitch(d), d
            g.close()
    lo = 1
    for d, (hi, _, _) in zip(RAGGED_DIMS, CFG_TABLE):  # the first dimension of each (3: d 1 and 2 pad alike)
        assert d == max(lo, 3) and d % 4 != 0
        lo = hi + 1


# ---------------------------------------------------------------- register lists
@every_config
def test_register_lists(cases, d, metric):
    """k_search_beam: BList<1> (ef 10), <2> (100), <4> (200) and <8> (400, the list whose G
    MH_BEAM_WIDE_G may lower), search_expand 1 / 2 / 4, the fp16 screen on and off, one wave per
    query"""
    c = cases(d, metric)
    H, g = c.H, c.g
    efs, xws = ((10, 200), (1, 4)) if _ragged(d) else ((10, 100, 200, 400), (1, 2, 4))
    old = _with(g, screen=1, search_expand=1, beam_mw_max_b=0)
    try:
        for screen in (1, 0):
            g.set_option("screen", screen)
            for xw in xws:
                g.set_option("search_expand", xw)
                for ef in efs:
                    g.reset_stats()
                    got = c.beam(K, ef)
                    st = g.stats()
                    print(d, metric, "screen", screen, "xw", xw, "ef", ef, {k: st[k] for k in COUNTERS})
                    _same_results(*got, *c.oracle(H.MODE_BEAM, K, ef, xw))
                    c.full_counts(got, K)
                    if screen:
                        assert st["search_screened"] > 0, (xw, ef)
                        assert st["search_f32_evals"] < st["search_dist_evals"], (xw, ef)
                    else:
                        assert st["search_screened"] == 0, (xw, ef)
    finally:
        _with(g, **old)


# ---------------------------------------------------------------- four-wave small-batch kernel
@full_set
def test_small_batch_kernel(cases, d, metric):
    """k_search_beam_mw (R <= 2, XW 1): the one-wave kernel's lists, for the whole batch and
    for B = 1"""
    c = cases(d, metric)
    H, g = c.H, c.g
    old = _with(g, search_expand=1, beam_mw_max_b=0, screen=1)
    try:
        for ef in (10, 100):
            g.set_option("beam_mw_max_b", 0)
            one = c.beam(K, ef)
            _same_results(*one, *c.oracle(H.MODE_BEAM, K, ef))
            g.set_option("beam_mw_max_b", 2 * B)
            for screen in (1, 0):
                g.set_option("screen", screen)
                g.reset_stats()
                _same_results(*c.beam(K, ef), *one)
                assert (g.stats()["search_screened"] > 0) == bool(screen)
                for b in (0, 7):
                    _same_results(*c.beam(K, ef, c.Q[b:b + 1]), *(x[b:b + 1] for x in one))
    finally:
        _with(g, **old)


# ---------------------------------------------------------------- LDS list
@every_config
def test_lds_list(cases, d, metric):
    """k_search_beam_lds: ef 600 and 2048 at every expansion width, ef 200 on both lists, and
    a 64-entry visited set that forgets at every step"""
    c = cases(d, metric)
    H, g = c.H, c.g
    old = _with(g, search_expand=1, beam_lds_min_ef=513, vis_compact=1)
    assert g.get_option("vis_compact") == 1
    try:
        for xw in (1,) if _ragged(d) else (1, 2, 4):
            g.set_option("search_expand", xw)
            got = c.beam(K, 600)
            _same_results(*got, *c.oracle(H.MODE_BEAM, K, 600, xw))
            c.full_counts(got, K)
            if _ragged(d):
                continue
            # the list never fills: every count is the number of rows reachable, the oracle's
            got = c.beam(2048, 2048)
            want = c.oracle(H.MODE_BEAM, 2048, 2048, xw)
            _same_results(*got, *want)
            assert (got[2] == want[2]).all() and (got[2] <= c.n).all() and (got[2][c.live_q] > 600).all()
            # ef 200 on the LDS list: the register list's result
            g.set_option("beam_lds_min_ef", 513)
            reg = c.beam(K, 200)
            g.set_option("beam_lds_min_ef", 65)
            lds = c.beam(K, 200)
            g.set_option("beam_lds_min_ef", 513)
            _same_results(*lds, *reg)
            _same_results(*lds, *c.oracle(H.MODE_BEAM, K, 200, xw))
        # resets may change the counters, never the lists
        for xw in (1,) if _ragged(d) else (1, 4):
            g.set_option("search_expand", xw)
            g.set_option("vis_entries", 64)
            try:
                g.reset_stats()
                got = c.beam(K, 600)
                assert g.stats()["visited_resets"] > 0
            finally:
                g.set_option("vis_entries", 0)
            _same_results(*got, *c.oracle(H.MODE_BEAM, K, 600, xw))
    finally:
        _with(g, **old)


# ---------------------------------------------------------------- filtered walk
@every_config
def test_filtered_walk(cases, d, metric):
    """k_search_beam_filt against tests/filtered_ref.py: lists and the number of expansions
    (the walk stops early and goes wide exactly as restated)"""
    c = cases(d, metric)
    g = c.g
    for ef, route in ((64, 200),) if _ragged(d) else ((10, 64), (64, 200), (128, 2048)):
        want, nx = c.filtered_ref(K, ef, route)
        g.reset_stats()
        got = c.filtered(K, ef, route)
        xs = g.stats()["search_expansions"]
        print(d, metric, "ef", ef, "route", route, "expansions", xs, nx)
        _same_results(*got, *want)
        assert xs == nx, (ef, route, xs, nx)
        for b in range(B):  # the padding
            assert (got[0][b, got[2][b]:] == -1).all() and np.isposinf(got[1][b, got[2][b]:]).all(), b
    # the filters bite: a filtered query's list differs from the unfiltered one of the same query
    plain = c.beam(K, 64)
    assert any(got[0][b].tolist() != plain[0][b].tolist() for b in range(B) if c.mask_of[b] is not None)


# ---------------------------------------------------------------- ordered path
@full_set
def test_ordered_path(cases, d, metric):
    """k_beam_descend and the layer-0 launch from `order`, through the device entry: the fused
    launch's lists and counters and the oracle's lists, with the pre-pass on its own 1,024-entry
    visited set (upper_ef 1) and on the launch's (upper_ef 64: beam_desc_vis)"""
    import torch

    c = cases(d, metric)
    H, g = c.H, c.g
    Qd = torch.tensor(c.Q, device="cuda")
    old = _with(g, search_order=0, search_order_min_b=1, beam_mw_max_b=0, search_expand=1, upper_ef=1)
    try:
        for upper_ef in (1, 64):
            g.set_option("upper_ef", upper_ef)
            for xw in (1, 4):
                g.set_option("search_expand", xw)
                for ef in (10, 64, 600):
                    r0, c0 = _search(torch, g, Qd, K, ef, 0)
                    r1, c1 = _search(torch, g, Qd, K, ef, 1)
                    _identical(r1, r0)
                    assert (r1[2] != -7).all() and (r1[0] != -7).all()  # no query skipped by the permutation
                    if c1 != c0:
                        # beam.hpp, beam_desc_vis: the pre-pass's small set may reset where the
                        # launch's own does not, which changes the counters and never the lists
                        assert upper_ef <= 4 and c1[4] > c0[4], (dict(zip(COUNTERS, c1)), dict(zip(COUNTERS, c0)))
                    assert c1[0] > 0 and c1[1] >= c.live_q.sum()
                    if upper_ef == 1:  # (the oracle descends with ef 1)
                        _same_results(*r1, *c.oracle(H.MODE_BEAM, K, ef, xw))
                    elif xw == 1 and ef <= 64:
                        # tests/filtered_ref.py descends with any width, and with every row
                        # allowed and route = ef its walk is the plain one-entry-per-step search
                        _same_results(*r1, *c.wide_descent_ref(K, ef, upper_ef))
    finally:
        _with(g, **old)


# ---------------------------------------------------------------- compat search and negatives
@every_config
def test_compat_and_negatives(cases, d, metric):
    """walks_units.hip: the reference-semantics search and the negatives re-ranking, one wave
    and eight waves per query"""
    c = cases(d, metric)
    H, O, g = c.H, c.O, c.g
    want = c.oracle(O.MODE_COMPAT, K, 16)
    neg = {m: c.o.search_negatives(c.Q, c.negs, K, 0.5, mode=m, ef=ef)
           for m, ef in ((O.MODE_COMPAT, 16), (O.MODE_BEAM, 40))}
    old = _with(g, compat_waves=1)
    try:
        for waves in (1, 8):
            g.set_option("compat_waves", waves)
            _same_results(*g.search_arrays(c.Q, K, mode=H.MODE_COMPAT, ef=16), *want)
            for m, ef in ((H.MODE_COMPAT, 16), (H.MODE_BEAM, 40)):
                _same_results(*g.search_negatives_arrays(c.Q, c.negs, K, 0.5, mode=m, ef=ef), *neg[m])
    finally:
        _with(g, **old)
    assert (want[2][c.live_q] == K).all()


# ---------------------------------------------------------------- exact
@every_config
def test_exact(cases, d, metric):
    c = cases(d, metric)
    H, g = c.H, c.g
    want = c.oracle(c.O.MODE_EXACT, K, 0)
    old = _with(g, exact_precision=3)
    try:
        for precision in (3, 0):
            g.set_option("exact_precision", precision)
            got = g.search_arrays(c.Q, K, mode=H.MODE_EXACT)
            _same_results(*got, *want)
            c.full_counts(got, K)
    finally:
        _with(g, **old)
    assert want[0][0, 0] == c.keys[40] and want[0][1, :2].tolist() == c.keys[[1, 2]].tolist()  # the tie, by id


# ---------------------------------------------------------------- range, beam mode
def _cut(lists, rad):
    keys, dist, lims = [], [], [0]
    rk, rd, rn = lists
    for b in range(len(rn)):
        dd = rd[b, : rn[b]]
        with np.errstate(invalid="ignore"):
            m = np.isfinite(dd) & (dd <= rad[b])
        keys.append(rk[b, : rn[b]][m])
        dist.append(dd[m])
        lims.append(lims[-1] + int(m.sum()))
    return np.asarray(lims, np.int64), np.concatenate(keys), np.concatenate(dist)


def _same_range(got, want):
    assert got[0].tolist() == want[0].tolist()
    assert got[1].tolist() == want[1].tolist()
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


@full_set
def test_range_beam(cases, d, metric):
    """the radius cut of the two walks' lists (the walks are the cases above), the radius at
    each query's exact 5th distance"""
    c = cases(d, metric)
    H, g = c.H, c.g
    ek, ed, en = c.oracle(c.O.MODE_EXACT, K, 0)
    rad = np.where(en >= 5, ed[:, 4], np.float32(np.nan)).astype(np.float32)
    lists = c.beam(64, 64)
    _same_results(*lists, *c.oracle(H.MODE_BEAM, 64, 64))
    want = _cut(lists, rad)
    _same_range(g.range_search_arrays(c.Q, rad, mode=H.MODE_BEAM, ef=64), want)
    hits = np.diff(want[0])
    assert (hits[c.live_q] >= 1).all() and (hits < 64).all() and (hits[~c.live_q] == 0).all()
    flists = c.filtered(64, 64, 200)
    _same_results(*flists, *c.filtered_ref(64, 64, 200)[0])
    fwant = _cut(flists, rad)
    _same_range(g.range_search_arrays(c.Q, rad, mode=H.MODE_BEAM, ef=64, filters=c.filter_of, route=200), fwant)
    assert 0 < fwant[0][-1] < want[0][-1]
