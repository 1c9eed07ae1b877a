"""GPU: the range search (range.hip; mhnsw_range_search*; Graph.range_search_arrays /
range_search_device / RangeSearch, ExactIndex.RangeSearch).

One contract: lims, keys and distance bits equal the oracle's MODE_EXACT search at
k = number of rows on an export of the graph, cut with isfinite(d) & (d <= r); beam
mode equals the oracle's beam search at k = ef cut the same way.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import _metric_fn

pytestmark = pytest.mark.gpu

N, B = 1531, 48  # 1531 = 5 * 256 + 251: five full row tiles and a tail
DEL = (7, 300, 1200, 1530)  # deleted rows (a tail-tile row among them)


def _data(metric, d, n=N, nq=B, edge=False):
    """tests/test_gpu_filtered_exact.py _data (duplicates of rows 5 and 64, Q[0] = X[5],
    Q[1] = 1.5 X[64]) with one zero row; edge: also a zero query and finite rows outside the
    fp16 bound (tests/test_gpu_parity.py test_exact_h16_outside_bound)"""
    rng = np.random.default_rng(100 * metric + d)
    X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    X[100:110] = X[5]
    if n > 900:
        X[900] = X[64]
    X[31] = 0
    Q = rng.uniform(-1, 1, (nq, d)).astype(np.float32)
    Q[0] = X[5]
    Q[1] = X[64] * 1.5
    if edge:
        Q[2] = 0
        X[120] *= np.float32(1e15)
        X[121] *= np.float32(1e-15)
        X[122] *= np.float32(2.0 ** 39)
        X[123] *= np.float32(2.0 ** -39)
        Q[5] *= np.float32(1e-15)
    return X, Q


class Case:
    """a graph, its queries, and the oracle's full sorted distance lists of its export"""

    def __init__(self, H, O, g, metric, Q):
        self.H, self.O, self.g, self.metric, self.Q = H, O, g, metric, Q
        ex = g.export()
        self.keys = ex["keys"]
        self.n = len(self.keys)
        self.o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64)
        self.o.import_graph(ex["keys"], ex["vecs"], ex["deg"], ex["adj"], ex["entry"], ex["dead"])
        self.rk, self.rd, self.rn = self.o.search(Q, self.n, mode=O.MODE_EXACT)
        self._beam = {}

    def nth(self, j, default=0.5):
        """per query the j-th smallest distance (default where fewer rows are usable)"""
        return np.array([self.rd[b, j - 1] if self.rn[b] >= j else default for b in range(len(self.Q))], np.float32)

    def cut(self, rad, lists=None):
        rk, rd, rn = lists or (self.rk, self.rd, self.rn)
        rad = np.broadcast_to(np.asarray(rad, np.float32), (len(rn),))
        keys, dist, lims = [], [], [0]
        for b in range(len(rn)):
            d = rd[b, : rn[b]]
            with np.errstate(invalid="ignore"):
                m = np.isfinite(d) & (d <= rad[b])
            keys.append(rk[b, : rn[b]][m])
            dist.append(d[m])
            lims.append(lims[-1] + int(m.sum()))
        return np.asarray(lims, np.int64), np.concatenate(keys), np.concatenate(dist)

    def beam(self, ef):
        if ef not in self._beam:
            self._beam[ef] = self.o.search(self.Q, ef, mode=self.O.MODE_BEAM, ef=ef)
        return self._beam[ef]

    def run(self, rad, **kw):
        return self.g.range_search_arrays(self.Q, rad, **kw)

    def check(self, rad, **kw):
        got, want = self.run(rad, **kw), self.cut(rad)
        _same(got, want)
        return got


def _same(got, want):
    assert got[0].tolist() == want[0].tolist()
    assert got[1].tolist() == want[1].tolist()
    assert got[2].view(np.uint32).tolist() == want[2].view(np.uint32).tolist()


def _graph(H, metric, X, flat=False):
    if flat:
        g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), build_mode=H.BUILD_FLAT)
    else:
        g = H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=_metric_fn(H, metric), Rng=3, build_mode=H.BUILD_BATCH,
                    ef_construction=40)
    keys = np.arange(len(X), dtype=np.int64) * 3 + 1
    g.add_arrays(keys, X)
    gone = [int(keys[i]) for i in DEL if i < len(X)]
    assert all(g.BatchDelete(gone))
    return g


@pytest.fixture(scope="module")
def built(H, O):
    """BUILD_BATCH graphs of in-bound data per (metric, dimension), B = 48 queries"""
    out = {}
    for metric in (0, 1):
        for d in (20, 100):
            X, Q = _data(metric, d)
            out[metric, d] = Case(H, O, _graph(H, metric, X), metric, Q)
    yield out
    for c in out.values():
        c.g.close()


def _mixed(c):
    """0 hits, 1 hit (or the rows tying it), 10 and 300 in one batch"""
    r = np.where(np.arange(len(c.Q)) % 4 == 0, np.float32(-1), c.nth(1))
    r = np.where(np.arange(len(c.Q)) % 4 == 2, c.nth(10), r)
    return np.where(np.arange(len(c.Q)) % 4 == 3, c.nth(300), r).astype(np.float32)


def _radii(c):
    r10 = c.nth(10)
    return {
        "tenth": r10,
        "below_tenth": np.nextafter(r10, np.float32(-np.inf)),
        "below_nearest": np.nextafter(c.nth(1), np.float32(-np.inf)),
        "mixed": _mixed(c),
    }


def _fused(c, got):
    """the path assertion of radii 1-4: the filter answered, and passed at least the hits on"""
    assert c.g.get_option("last_range_fallback_queries") == 0
    assert c.g.get_option("last_range_candidates") >= int(got[0][-1])


# ---------------------------------------------------------------- exact mode: radii, metrics, dimensions
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_radii(built, metric, d):
    c = built[metric, d]
    assert c.g.get_option("range_expect") == 64
    for name, rad in _radii(c).items():
        got = c.check(rad)
        counts = np.diff(got[0])
        print(name, "hits", int(got[0][-1]), "candidates", c.g.get_option("last_range_candidates"))
        _fused(c, got)
        if name == "tenth":  # a row at the boundary is a hit
            assert set(counts.tolist()) <= {10, 11}, counts
            assert got[2][0] == 0.0 or metric == 0
            # the eleven copies of row 5 at Q[0], in row order
            assert got[1][:11].tolist() == c.keys[[5] + list(range(100, 110))].tolist()
        if name == "below_nearest":
            assert int(got[0][-1]) == 0


@pytest.mark.parametrize("metric", [0, 1])
def test_everything_and_nothing(built, metric):
    c = built[metric, 20]
    got = c.check(np.float32(3e38))  # every usable row of every query: past the sub-buckets, the sweep
    assert np.array_equal(np.diff(got[0]), c.rn)
    assert c.g.get_option("last_range_fallback_queries") == B
    for rad in (np.float32(np.nan), np.float32(-1)):
        got = c.check(rad)
        assert got[0].tolist() == [0] * (B + 1) and len(got[1]) == 0
    got = c.check(np.float32(np.inf))
    assert np.array_equal(np.diff(got[0]), c.rn)


@pytest.mark.parametrize("metric", [0, 1])
def test_forced_fallback_and_precisions(built, metric):
    """the sweep equals the fused path bit for bit; exact_precision does not matter (the call
    scores at 3)"""
    c = built[metric, 100]
    rads = _radii(c)
    fused = {k: c.check(r) for k, r in rads.items()}
    c.g.set_option("range_force_fallback", 1)
    try:
        for k, r in rads.items():
            got = c.run(r)
            assert c.g.get_option("last_range_fallback_queries") == B
            assert c.g.get_option("last_range_candidates") == 0
            for x, y in zip(got, fused[k]):
                assert x.tobytes() == y.tobytes()
    finally:
        c.g.set_option("range_force_fallback", 0)
    old = c.g.get_option("exact_precision")
    try:
        for p in (0, 1, 2, 3):
            c.g.set_option("exact_precision", p)
            got = c.check(rads["mixed"])
            _fused(c, got)
            for x, y in zip(got, fused["mixed"]):
                assert x.tobytes() == y.tobytes()
            # the top-k search still answers at this precision afterwards
            k10 = c.g.search_arrays(c.Q, 10, mode=c.H.MODE_EXACT)
            assert k10[0][:, 0].tolist() == c.rk[:, 0].tolist()
    finally:
        c.g.set_option("exact_precision", old)


@pytest.mark.parametrize("metric", [0, 1])
def test_second_query_tile(H, O, metric):
    """B = 300: a second, ragged query tile"""
    X, Q = _data(metric, 20, nq=300)
    g = _graph(H, metric, X)
    try:
        c = Case(H, O, g, metric, Q)
        for name, rad in _radii(c).items():
            _fused(c, c.check(rad))
        got = c.check(np.float32(3e38))
        assert g.get_option("last_range_fallback_queries") == 300
    finally:
        g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_small_index_sweep_only(H, O, metric):
    """N = 200: no full row tile, the sweep is the whole path"""
    X, Q = _data(metric, 20, n=200)
    g = _graph(H, metric, X)
    try:
        c = Case(H, O, g, metric, Q)
        for name, rad in _radii(c).items():
            if name == "mixed":
                rad = np.where(np.arange(B) % 4 == 3, c.nth(150), rad).astype(np.float32)
            c.check(rad)
            # (a negative radius has no hit under L2 and is not swept; under cosine it is a radius)
            assert g.get_option("last_range_fallback_queries") == (B if metric == 0 else int((rad >= 0).sum()))
            assert g.get_option("last_range_candidates") == 0
        c.check(np.float32(3e38))
    finally:
        g.close()


@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_edge_data_flat_index(H, O, metric, d):
    """a flat index with a zero query and rows and a query outside the fp16 bound: parity on
    whichever path answers"""
    X, Q = _data(metric, d, edge=True)
    g = _graph(H, metric, X, flat=True)
    try:
        c = Case(H, O, g, metric, Q)
        for name, rad in _radii(c).items():
            c.check(rad)
        if metric == 0:  # every distance of the zero query is NaN
            assert c.rn[2] == 0
        c.check(np.float32(3e38))
        with pytest.raises(H.HnswError, match="flat index") as e:
            c.run(c.nth(10), mode=H.MODE_BEAM, ef=64)
        assert e.value.code == H._lib.EUNSUPPORTED
    finally:
        g.close()


def test_stage_times(built):
    c = built[0, 100]
    c.run(c.nth(10))
    total = c.g.last_kernel_ms() * 1e6
    parts = [c.g.get_option(f"last_range_{s}_ns") for s in ("filter", "refine", "sweep", "order")]
    assert all(p > 0 for p in parts) and sum(parts) <= total * 1.001
    assert 0 < c.g.get_option("last_gemm_ns") <= parts[0]
    c.run(c.nth(10), mode=c.H.MODE_BEAM, ef=64)  # beam mode has no such stages
    with pytest.raises(c.H.HnswError):
        c.g.get_option("last_range_refine_ns")


# ---------------------------------------------------------------- device entry
def test_device_entry_cap_and_streams(built):
    import torch

    c = built[1, 100]
    H, g = c.H, c.g
    dev = torch.device("cuda:0")
    rad = _mixed(c)
    host = c.check(rad)
    total = int(host[0][-1])
    q = torch.from_numpy(c.Q).to(dev)
    r = torch.from_numpy(rad).to(dev)
    GUARD = 64

    def call(cap, stream, radius=r):
        lims = torch.full((B + 1,), -5, dtype=torch.int64, device=dev)
        keys = torch.full((cap + GUARD,), -7, dtype=torch.int64, device=dev)
        dist = torch.full((cap + GUARD,), -9.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            g.range_search_device(q.data_ptr(), B, c.Q.shape[1], radius.data_ptr(), cap, lims.data_ptr(),
                                  keys.data_ptr(), dist.data_ptr(), stream=stream.cuda_stream)
        return lims, keys, dist

    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for cap in (total, total + 100, total // 2, 7, 0):
        lims, keys, dist = call(cap, sa)
        sa.synchronize()
        g.device_status()
        lims, keys, dist = lims.cpu().numpy(), keys.cpu().numpy(), dist.cpu().numpy()
        m = min(cap, total)
        assert lims.tolist() == host[0].tolist(), cap  # the true prefix whatever fits
        assert keys[:m].tolist() == host[1][:m].tolist(), cap
        assert dist[:m].view(np.uint32).tolist() == host[2][:m].view(np.uint32).tolist(), cap
        assert (keys[m:] == -7).all() and (dist[m:] == -9.0).all(), cap  # nothing past the hits or the buffer
    # two streams back to back on one handle: the second waits for the scratch of the first
    r2 = torch.from_numpy(c.nth(10)).to(dev)
    want2 = c.cut(c.nth(10))
    for _ in range(2):
        a = call(total, sa)
        b = call(int(want2[0][-1]), sb, r2)
        torch.cuda.synchronize()
        for got, want in ((a, host), (b, want2)):
            n = int(want[0][-1])
            assert got[0].cpu().numpy().tolist() == want[0].tolist()
            assert got[1].cpu().numpy()[:n].tolist() == want[1].tolist()
            assert got[2].cpu().numpy()[:n].view(np.uint32).tolist() == want[2].view(np.uint32).tolist()
    g.device_status()
    # beam mode on a stream
    lims = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    keys = torch.full((B * 64,), -7, dtype=torch.int64, device=dev)
    dist = torch.zeros(B * 64, dtype=torch.float32, device=dev)
    with torch.cuda.stream(sa):
        g.range_search_device(q.data_ptr(), B, c.Q.shape[1], r2.data_ptr(), B * 64, lims.data_ptr(), keys.data_ptr(),
                              dist.data_ptr(), mode=H.MODE_BEAM, ef=64, stream=sa.cuda_stream)
    sa.synchronize()
    want = c.cut(c.nth(10), c.beam(64))
    n = int(want[0][-1])
    assert lims.cpu().numpy().tolist() == want[0].tolist()
    assert keys.cpu().numpy()[:n].tolist() == want[1].tolist()


# ---------------------------------------------------------------- beam mode
@pytest.mark.parametrize("ef", [64, 768])  # the register list and the LDS list
@pytest.mark.parametrize("metric", [0, 1])
def test_beam_mode(built, metric, ef):
    c = built[metric, 20]
    H = c.H
    lists = c.beam(ef)
    for rad in (c.nth(10), _mixed(c)):
        got = c.run(rad, mode=H.MODE_BEAM, ef=ef)
        _same(got, c.cut(rad, lists))
        exact = c.cut(rad)
        for b in range(B):  # a subset of the exact hits
            assert set(got[1][got[0][b]:got[0][b + 1]].tolist()) <= set(exact[1][exact[0][b]:exact[0][b + 1]].tolist())
    got = c.run(np.float32(3e38), mode=H.MODE_BEAM, ef=ef)  # the radius covers the whole list
    _same(got, c.cut(np.float32(3e38), lists))
    assert np.array_equal(np.diff(got[0]), lists[2]) and (np.diff(got[0]) == ef).all()


# ---------------------------------------------------------------- keys, hosts, errors
def test_string_keys(H):
    rng = np.random.default_rng(8)
    X = rng.normal(size=(300, 16)).astype(np.float32)
    g = H.Graph(M=8, Ml=0.25, EfSearch=32, Distance=H.EuclideanDistance, Rng=1, build_mode=H.BUILD_BATCH)
    names = [f"row-{i:04d}" for i in range(300)]
    g.BatchAdd([H.MakeNode(k, v) for k, v in zip(names, X)])
    try:
        d = np.sqrt(((X - X[17]) ** 2).sum(1))
        order = sorted(range(300), key=lambda i: (d[i], i))
        rad = float(np.float32(d[order[12]]) * np.float32(1.0001))
        got = [n.Key for n in g.RangeSearch(X[17], rad)]
        assert got[:12] == [names[i] for i in order[:12]] and names[order[12]] in got and len(got) < 40
        lims, keys, dist = g.range_search_arrays(X[:5], rad)
        per = H.split_ragged(lims, g.decode_keys(keys), dist)
        assert [p[0][0] for p in per] == names[:5] and all((np.diff(p[1]) >= 0).all() for p in per)
    finally:
        g.close()


def test_exact_index_after_replace_and_delete(H):
    rng = np.random.default_rng(4)
    X = rng.normal(size=(400, 12)).astype(np.float32)
    ix = H.ExactIndex(H.EuclideanDistance)
    ix.BatchAdd(list(range(400)), list(X))
    X[9] = X[3] + np.float32(1e-3)  # a replacement moves key 9 next to key 3
    ix.Add(9, X[9])
    assert ix.Delete(11)

    def want(q, r):
        d = np.array([np.sqrt(np.sum((x - q) ** 2, dtype=np.float32)) for x in X], np.float32)
        return [i for i in sorted(range(400), key=lambda i: (d[i], i)) if i != 11 and d[i] <= r]

    d3 = np.sort(np.sqrt(((X - X[3]) ** 2).sum(1)))
    rad = float(d3[20] + d3[21]) / 2
    got = [n.Key for n in ix.RangeSearch(X[3], rad)]
    assert got[:2] == [3, 9] and 11 not in got and got == want(X[3], rad)
    lims, keys, dist = ix.range_search_batch(X[:3], rad)
    assert keys[lims[0]] == 0 and len(keys) == lims[-1] == len(dist)
    ix.Close()


def test_empty_and_errors(built):
    c = built[0, 20]
    H, g = c.H, c.g
    e = H.Graph(M=8, Ml=0.25, EfSearch=20)
    lims, keys, dist = e.range_search_arrays(np.zeros((3, 5), np.float32), 1.0)
    assert lims.tolist() == [0, 0, 0, 0] and len(keys) == 0 and len(dist) == 0
    e.close()
    with pytest.raises(H.HnswError, match="range search supports beam and exact mode") as err:
        g.range_search_arrays(c.Q, 0.5, mode=H.MODE_COMPAT)
    assert err.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match="embedding dimension mismatch") as err:
        g.range_search_arrays(c.Q[:, :7], 0.5)
    assert err.value.code == H._lib.EDIM
    with pytest.raises(H.HnswError, match=r"beam mode supports max\(ef,k\) <= 2048") as err:
        g.range_search_arrays(c.Q, 0.5, mode=H.MODE_BEAM, ef=2049)
    assert err.value.code == H._lib.EUNSUPPORTED
    import ctypes as C

    lib = H.load()
    got = g.range_search_arrays(c.Q, c.nth(10))
    total = int(got[0][-1])
    keys, dist = np.zeros(total, np.int64), np.zeros(total, np.float32)
    rc = lib.mhnsw_range_results(g._h, keys.ctypes.data_as(C.POINTER(C.c_int64)),
                                 dist.ctypes.data_as(C.POINTER(C.c_float)), total - 1)
    assert rc == H._lib.EINVAL and "is below the" in lib.mhnsw_last_error(g._h).decode()
    rc = lib.mhnsw_range_search_device(g._h, None, B, 7, None, H.MODE_EXACT, 0, 10, None, None, None, None)
    assert rc == H._lib.EDIM
    rc = lib.mhnsw_range_search_device(g._h, None, B, 20, None, 0, 0, 10, None, None, None, None)
    assert rc == H._lib.EUNSUPPORTED
    assert g.last_kernel_ms() > 0
