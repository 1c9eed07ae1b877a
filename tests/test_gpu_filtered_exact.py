"""GPU: the filtered exact search (rowset.hip; mhnsw_search_filtered_exact*;
Graph.search_filtered_arrays(mode=MODE_EXACT) / search_filtered_exact_device).

One contract: keys, distance bits and counts equal the oracle's MODE_EXACT
search on a copy of the graph imported with dead[i] = 1 for every row that is
deleted or not allowed (the construction of tests/filtered_ref.py
distance_table, with the mask in the dead flags).
"""
import numpy as np
import pytest

from tests.test_gpu_parity import _bit_equal, _metric_fn

pytestmark = pytest.mark.gpu

N, B, K = 1531, 48, 10  # 1531 = 47 * 32 + 27 = 5 * 256 + 251: a tail bitmap word and a tail row tile
EDGES = (0, 31, 32, 63, 64, N - 1)  # both sides of the first bitmap word boundaries, and the tail word's last row
SIZES = (0, 1, K - 1, 255, 256, 257, 513, N - 1, N)  # around the fused path's row tile (256) and the list edges


def _same(got, want):
    gk, gd, gn = got
    rk, rd, rn = want
    assert np.array_equal(gn, rn), (gn, rn)
    for b in range(len(gn)):
        n = gn[b]
        assert gk[b, :n].tolist() == rk[b, :n].tolist(), b
        assert _bit_equal(gd[b, :n], rd[b, :n]), b


class Case:
    """a graph, its queries, and the oracle's masked exact search of its export (cached)"""

    def __init__(self, H, O, g, metric, Q):
        self.H, self.O, self.g, self.metric, self.Q = H, O, g, metric, Q
        self.refresh()

    def refresh(self):
        self.ex = self.g.export()
        self.keys = self.ex["keys"]
        self.n = len(self.keys)
        self._memo = {}

    def ref(self, mask, k, Q=None):
        """the oracle's exact search with `mask` (bool [n], None: every row) in the dead flags"""
        mask = np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)
        key = (mask.tobytes(), k, None if Q is None else Q.tobytes())
        if key not in self._memo:
            O, ex = self.O, self.ex
            o = O.Graph(metric=self.metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64)
            dead = (ex["dead"].astype(bool) | ~mask).astype(np.uint8)
            if dead.all():  # nothing to search: no row, no error
                q = self.Q if Q is None else Q
                self._memo[key] = (np.zeros((len(q), k), np.int64), np.zeros((len(q), k), np.float32),
                                   np.zeros(len(q), np.int32))
            else:
                o.import_graph(ex["keys"], ex["vecs"], ex["deg"], ex["adj"], ex["entry"], dead)
                self._memo[key] = o.search(self.Q if Q is None else Q, k, mode=O.MODE_EXACT)
        return self._memo[key]

    def filter(self, mask):
        return self.g.Filter(self.keys[np.asarray(mask, bool)].tolist())

    def check(self, mask, k=K, f=None):
        own = f is None
        f = self.filter(mask) if own else f
        try:
            got = self.g.search_filtered_arrays(self.Q, k, f, mode=self.H.MODE_EXACT)
        finally:
            if own:
                f.close()
        _same(got, self.ref(mask, k))
        return got


def _mask(rng, n, m):
    """m allowed rows of n: the rows around the bitmap word boundaries first"""
    mask = np.zeros(n, bool)
    if m >= n - 1:
        mask[:] = True
        if m == n - 1:
            mask[777] = False
        return mask
    edges = [e if e >= 0 else n + e for e in (0, 31, 32, 63, 64, -1)]
    take = edges[: min(m, len(edges))]
    mask[take] = True
    rest = np.setdiff1d(np.arange(n), take)
    mask[rng.choice(rest, m - len(take), replace=False)] = True
    assert mask.sum() == m
    return mask


def _data(metric, d, n=N):
    rng = np.random.default_rng(100 * metric + d)
    X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    X[100:110] = X[5]  # duplicates: equal distances come out in row order
    X[900] = X[64]
    Q = rng.uniform(-1, 1, (B, d)).astype(np.float32)
    Q[0] = X[5]
    Q[1] = X[64] * 1.5
    return rng, X, Q


def _batch_graph(H, metric, X, **kw):
    g = H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=_metric_fn(H, metric), Rng=3, build_mode=H.BUILD_BATCH,
                ef_construction=40, **kw)
    g.add_arrays(np.arange(len(X), dtype=np.int64) * 3 + 1, X)
    return g


@pytest.fixture(scope="module")
def built(H, O):
    """BUILD_BATCH graphs per (metric, dimension): 20 is no multiple of the row pitch
    unit, 100 spans several K-blocks of 16"""
    out = {}
    for metric in (0, 1):
        for d in (20, 100):
            rng, X, Q = _data(metric, d)
            out[metric, d] = Case(H, O, _batch_graph(H, metric, X), metric, Q)
    yield out
    for c in out.values():
        c.g.close()


# ---------------------------------------------------------------- allow-set sizes, metrics, dimensions
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_allow_set_sizes(built, metric, d):
    c = built[metric, d]
    for m in SIZES:
        mask = _mask(np.random.default_rng(1000 * metric + d + m), N, m)
        got = c.check(mask)
        assert (got[2] == min(K, m)).all(), m
        if m >= 16:  # the duplicates of row 5 are allowed or not at random: the allowed ones, in row order
            dup = [r for r in [5] + list(range(100, 110)) if mask[r]]
            n = min(len(dup), K)
            assert got[0][0, :n].tolist() == c.keys[dup[:n]].tolist(), m


@pytest.mark.parametrize("k", [1, 10, 256])
@pytest.mark.parametrize("precision", [0, 1, 2, 3])
def test_k_and_precision(built, k, precision):
    """exact_precision 2 and 3 score the gathered fp16 plane; 0 and 1 keep none, and the call
    scores at 3: the same results every time"""
    for key in ((0, 100), (1, 20)):
        c = built[key]
        old = c.g.get_option("exact_precision")
        c.g.set_option("exact_precision", precision)
        try:
            for m in (257, 700):  # k = 256 among 257 rows: all but one
                c.check(_mask(np.random.default_rng(m), N, m), k=k)
        finally:
            c.g.set_option("exact_precision", old)


def test_duplicates_in_row_order(built):
    c = built[0, 20]
    mask = np.zeros(N, bool)
    mask[[5, 64, 900] + list(range(100, 110))] = True
    mask[300:400] = True
    got = c.check(mask)
    assert got[0][0, :10].tolist() == c.keys[[5] + list(range(100, 109))].tolist()
    assert got[0][1, :2].tolist() == c.keys[[64, 900]].tolist()


# ---------------------------------------------------------------- certificate fallback
@pytest.mark.parametrize("m", [100, 600])  # the 2-product path of small sets, and the fused path
@pytest.mark.parametrize("metric", [0, 1])
def test_certificate_fallback(H, O, metric, m):
    """near-duplicate rows and a preselection of exactly k: the k-th score sits on the bound, the
    certificate fails and the canonical sweep over the allowed rows answers -- the same bytes"""
    rng, X, Q = _data(metric, 24)
    X[200:900] = X[200] * (1 + 1e-7 * rng.normal(size=(700, 1))).astype(np.float32) + \
        (1e-6 * rng.normal(size=(700, 24))).astype(np.float32)
    g = _batch_graph(H, metric, X, exact_kk=K)
    try:
        c = Case(H, O, g, metric, Q)
        mask = np.zeros(N, bool)
        mask[200:200 + m - 6] = True
        mask[list(EDGES)] = True
        g.reset_stats()
        c.check(mask)
        assert g.stats()["exact_uncertified"] > 0
    finally:
        g.close()


# ---------------------------------------------------------------- row state
@pytest.mark.parametrize("metric", [0, 1])
def test_row_state_compat_build(H, O, metric):
    """a BUILD_COMPAT graph: rows added after the filter was made (not returned until an update
    names them), deleted rows inside the filter"""
    rng, X, Q = _data(metric, 20, n=1100)
    keys = np.arange(1100, dtype=np.int64) * 3 + 1
    g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), Rng=11)
    g.add_arrays(keys[:1000], X[:1000])
    try:
        c = Case(H, O, g, metric, Q)
        mask = rng.random(1000) < 0.5
        mask[list(EDGES[:5]) + [999]] = True
        f = c.filter(mask)
        c.check(mask, f=f)
        # 100 more rows (a bitmap word boundary among them): not allowed yet
        g.add_arrays(keys[1000:], X[1000:])
        c.refresh()
        old = np.concatenate([mask, np.zeros(c.n - 1000, bool)])
        assert np.isin(c.keys, keys[1000:]).sum() == 100
        Qn = X[1000:1048].copy()  # queries sitting on the new rows
        got = c.g.search_filtered_arrays(Qn, K, f, mode=H.MODE_EXACT)
        _same(got, c.ref(old, K, Qn))
        assert not set(got[0].ravel().tolist()) & set(keys[1000:].tolist())
        f.add(keys[1000:1060].tolist())
        named = old | np.isin(c.keys, keys[1000:1060])
        got = c.g.search_filtered_arrays(Qn, K, f, mode=H.MODE_EXACT)
        _same(got, c.ref(named, K, Qn))
        assert got[0][:, 0].tolist() == keys[1000:1048].tolist()
        # deleted rows, inside the filter and outside it: their bits stay, they are not returned
        gone = np.flatnonzero(named)[::7].tolist() + np.flatnonzero(~named)[::9].tolist()
        assert all(g.BatchDelete([int(c.keys[i]) for i in gone]))
        gone_keys = {int(c.keys[i]) for i in gone}
        c.refresh()
        got = c.check(named, f=f)
        assert not set(got[0].ravel().tolist()) & gone_keys
        f.close()
    finally:
        g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_flat_index_and_zero_vector(H, O, metric):
    """BUILD_FLAT (exact search only); under cosine a zero vector inside the allow-set has a
    NaN distance and is never returned"""
    rng, X, Q = _data(metric, 72)
    X[[31, 500]] = 0
    g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), build_mode=H.BUILD_FLAT)
    g.add_arrays(np.arange(N, dtype=np.int64) * 3 + 1, X)
    try:
        c = Case(H, O, g, metric, Q)
        for m in (9, 300, N):
            mask = _mask(rng, N, m)
            mask[500] = True
            got = c.check(mask)
            if metric == 0:
                assert not set(got[0].ravel().tolist()) & {31 * 3 + 1, 500 * 3 + 1}
        mask = np.zeros(N, bool)
        mask[[31, 500, 7]] = True
        got = c.check(mask)
        if metric == 0:
            assert (got[2] == 1).all() and (got[0][:, 0] == 7 * 3 + 1).all()
    finally:
        g.close()


def test_exact_index_adapters(H):
    """ExactIndex / ExactAdapter (a flat index) search among a filter's keys"""
    rng = np.random.default_rng(4)
    X = rng.normal(size=(400, 12)).astype(np.float32)
    ix = H.ExactIndex(H.EuclideanDistance)
    ix.BatchAdd(list(range(400)), list(X))
    f = ix.Filter(list(range(0, 400, 5)))
    want = sorted(range(0, 400, 5), key=lambda i: (float(np.sum((X[i] - X[3]) ** 2)), i))[:4]
    assert [n.Key for n in ix.SearchFiltered(X[3], 4, f)] == want
    ks, ds = H.ExactAdapter(ix).SearchFiltered(X[3], 4, f)
    assert ks == want and len(ds) == 4
    ks, _, n = ix.search_filtered_batch(X[:3], 4, [f, None, f])
    assert ks[1][0] == 1 and ks[0][0] == 0 and ks[2] == sorted(
        range(0, 400, 5), key=lambda i: (float(np.sum((X[i] - X[2]) ** 2)), i))[:4]
    ix.Close()


# ---------------------------------------------------------------- host batch, device entry
def test_mixed_host_batch(built):
    """filter_of interleaves three filters and -1: every query's list at its own position"""
    c, H = built[1, 100], built[1, 100].H
    masks = [_mask(np.random.default_rng(s), N, m) for s, m in ((1, 40), (2, 300), (3, 1000))]
    fs = [c.filter(m) for m in masks]
    order = np.random.default_rng(9).integers(-1, 3, B)
    order[:5] = [2, -1, 0, 1, -1]
    got = c.g.search_filtered_arrays(c.Q, K, [None if i < 0 else fs[i] for i in order], mode=H.MODE_EXACT)
    refs = {i: c.ref(None if i < 0 else masks[i], K) for i in (-1, 0, 1, 2)}
    for b in range(B):
        rk, rd, rn = refs[int(order[b])]
        assert got[2][b] == rn[b]
        assert got[0][b, : rn[b]].tolist() == rk[b, : rn[b]].tolist(), b
        assert _bit_equal(got[1][b, : rn[b]], rd[b, : rn[b]]), b
    # filter -1 alone is the plain exact search, byte for byte
    a = c.g.search_filtered_arrays(c.Q, K, None, mode=H.MODE_EXACT)
    p = c.g.search_arrays(c.Q, K, mode=H.MODE_EXACT)
    for x, y in zip(a, p):
        assert x.tobytes() == y.tobytes()
    for f in fs:
        f.close()


def test_device_entry(built):
    """the device entry on a non-null stream == the host entry; the status word stays clean"""
    import torch

    c, H = built[0, 100], built[0, 100].H
    dev = torch.device("cuda:0")
    q = torch.from_numpy(c.Q).to(dev)
    for m in (9, 257, N):
        mask = _mask(np.random.default_rng(m), N, m)
        f = c.filter(mask)
        host = c.g.search_filtered_arrays(c.Q, K, f, mode=H.MODE_EXACT)
        s = torch.cuda.Stream()
        ok = torch.full((B, K), -7, dtype=torch.int64, device=dev)
        od = torch.zeros((B, K), dtype=torch.float32, device=dev)
        on = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            c.g.search_filtered_exact_device(q.data_ptr(), B, c.Q.shape[1], K, f, ok.data_ptr(), od.data_ptr(),
                                             on.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        c.g.device_status()
        _same((ok.cpu().numpy(), od.cpu().numpy(), on.cpu().numpy()), host)
        _same(host, c.ref(mask, K))
        f.close()
    with torch.cuda.stream(s):  # None: the plain exact search on the stream
        c.g.search_filtered_exact_device(q.data_ptr(), B, c.Q.shape[1], K, None, ok.data_ptr(), od.data_ptr(),
                                         on.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    c.g.device_status()
    _same((ok.cpu().numpy(), od.cpu().numpy(), on.cpu().numpy()), c.g.search_arrays(c.Q, K, mode=H.MODE_EXACT))


def test_stage_times(built):
    c, H = built[0, 100], built[0, 100].H
    f = c.filter(_mask(np.random.default_rng(1), N, 600))
    c.g.search_filtered_arrays(c.Q, K, f, mode=H.MODE_EXACT)
    total = c.g.last_kernel_ms() * 1e6
    parts = [c.g.get_option(f"last_fx_{s}_ns") for s in ("compact", "gather", "select", "rerank", "fallback")]
    assert all(p > 0 for p in parts) and sum(parts) <= total * 1.001
    f.close()


# ---------------------------------------------------------------- the walk agrees
@pytest.mark.parametrize("metric", [0, 1])
def test_walk_recall_with_every_row_allowed(H, metric):
    """every row allowed and a route list wider than the index: the filtered walk finds the
    exact call's keys.  A subset check on an index of its own, without `built`'s repeated
    vectors: a walk returns only rows its edges reach (on `built` at L2 it misses 1 key of 480)."""
    rng = np.random.default_rng(60 + metric)
    X = rng.uniform(-1, 1, (N, 20)).astype(np.float32)
    Q = rng.uniform(-1, 1, (B, 20)).astype(np.float32)
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=5, build_mode=H.BUILD_BATCH,
                ef_construction=100)
    keys = np.arange(N, dtype=np.int64) * 3 + 1
    g.add_arrays(keys, X)
    try:
        f = g.Filter(keys.tolist())
        ek, _, en = g.search_filtered_arrays(Q, K, f, mode=H.MODE_EXACT)
        wk, _, wn = g.search_filtered_arrays(Q, K, f, ef=64, route=2048)
        miss = {b: sorted(set(ek[b, : en[b]].tolist()) - set(wk[b, : wn[b]].tolist())) for b in range(B)}
        miss = {b: m for b, m in miss.items() if m}
        print("walk misses", miss)
        assert (en == K).all() and not miss
    finally:
        g.close()


# ---------------------------------------------------------------- errors
def test_errors(built):
    c, H = built[0, 20], built[0, 20].H
    g = c.g
    f = c.filter(_mask(np.random.default_rng(2), N, 300))
    ex = dict(mode=H.MODE_EXACT)
    with pytest.raises(H.HnswError, match="exact mode supports k <= 256") as e:
        g.search_filtered_arrays(c.Q, 257, f, **ex)
    assert e.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match="k must be greater than 0, got 0") as e:
        g.search_filtered_arrays(c.Q, 0, f, **ex)
    assert e.value.code == H._lib.EK
    with pytest.raises(H.HnswError, match="embedding dimension mismatch") as e:
        g.search_filtered_arrays(c.Q[:, :7], K, f, **ex)
    assert e.value.code == H._lib.EDIM
    with pytest.raises(H.HnswError, match="MODE_BEAM and MODE_EXACT"):
        g.search_filtered_arrays(c.Q, K, f, mode=H.MODE_COMPAT)
    other = built[1, 20]
    fo = other.filter(np.ones(N, bool))
    with pytest.raises(H.HnswError, match="filter of another graph"):
        g.search_filtered_arrays(c.Q, K, fo, **ex)
    fo.close()
    # an id that names no filter, in a one-filter batch and in a mixed one, and a destroyed one
    import ctypes as C

    lib = H.load()
    ok, od, on = np.zeros((B, K), np.int64), np.zeros((B, K), np.float32), np.full(B, -3, np.int32)

    def call(fo):
        fo = np.ascontiguousarray(fo, np.int32)
        return lib.mhnsw_search_filtered_exact(g._h, c.Q.ctypes.data_as(C.POINTER(C.c_float)), B, c.Q.shape[1], K,
                                               fo.ctypes.data_as(C.POINTER(C.c_int32)),
                                               ok.ctypes.data_as(C.POINTER(C.c_int64)),
                                               od.ctypes.data_as(C.POINTER(C.c_float)),
                                               on.ctypes.data_as(C.POINTER(C.c_int32)))

    fid = f.id
    assert call(np.full(B, 999)) == H._lib.EINVAL
    assert lib.mhnsw_last_error(g._h).decode() == "unknown filter 999"
    mixed = np.full(B, fid)
    mixed[7], mixed[8] = -1, 1000
    assert call(mixed) == H._lib.EINVAL
    assert lib.mhnsw_last_error(g._h).decode() == "unknown filter 1000"
    assert (on == -3).all()  # refused before the first pass wrote a result
    f.close()
    assert call(np.full(B, fid)) == H._lib.EINVAL
    assert lib.mhnsw_last_error(g._h).decode() == f"unknown filter {fid}"
    with pytest.raises(H.HnswError, match="unknown filter"):
        g.search_filtered_arrays(c.Q, K, f, **ex)
    rc = lib.mhnsw_search_filtered_exact_device(g._h, None, B, c.Q.shape[1], K, fid, None, None, None, None)
    assert rc == H._lib.EINVAL and lib.mhnsw_last_error(g._h).decode() == f"unknown filter {fid}"
