"""GPU: the filtered range search (range.hip over a gathered row set; mhnsw_range_search_filtered*;
Graph.range_search_arrays(filters=) / range_search_filtered_device / RangeSearch(filter=)).

One contract: lims, keys and distance bits equal the oracle's MODE_EXACT search at k = rows
on a copy of the graph's export imported with dead |= ~mask (the Case of
tests/test_gpu_filtered_exact.py), cut with isfinite(d) & (d <= r) (the cut of
tests/test_gpu_range.py).  Beam mode equals tests/filtered_ref.py search_batch at k = ef, cut
the same way.
"""
import numpy as np
import pytest

from tests import filtered_ref as FR
from tests.test_gpu_filtered_exact import Case as MaskedCase
from tests.test_gpu_filtered_exact import _mask
from tests.test_gpu_range import DEL, _data, _graph, _same

pytestmark = pytest.mark.gpu

N, B = 1531, 48  # 1531 = 5 * 256 + 251 = 47 * 32 + 27: a tail row tile and a tail bitmap word
SIZES = (0, 1, 255, 256, 257, 513, N - 1, N)  # around the fused path's row tile (256)


def _cut(lists, rad):
    rk, rd, rn = lists
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


class Case(MaskedCase):
    """a graph, its queries, and per mask the oracle's full sorted list of the allowed rows"""

    def lists(self, mask, Q=None):
        return self.ref(mask, self.n, Q)

    def nth(self, mask, j, default=0.5):
        """per query the j-th smallest allowed distance (the last one where fewer rows are
        usable, default where none is)"""
        _, rd, rn = self.lists(mask)
        return np.array([rd[b, min(j, rn[b]) - 1] if rn[b] else default for b in range(len(rn))], np.float32)

    def usable(self, mask):
        """the rows of the mask the search works over: allowed and not deleted"""
        return int((np.asarray(mask, bool) & ~self.ex["dead"][: self.n].astype(bool)).sum())

    def want(self, mask, rad, Q=None):
        return _cut(self.lists(mask, Q), rad)

    def run(self, f, rad, **kw):
        return self.g.range_search_arrays(self.Q, rad, filters=f, **kw)

    def check(self, mask, rad, f=None, **kw):
        own = f is None
        f = self.filter(mask) if own else f
        try:
            got = self.run(f, rad, **kw)
        finally:
            if own:
                f.close()
        _same(got, self.want(mask, rad))
        return got


def _sized_mask(c, rng, m):
    """_mask's construction (the bitmap word boundary rows first, a deleted row among them),
    topped up with live rows so that exactly m rows are usable -- the sizes are the sizes of
    the row set the kernels see.  (N - 1 and N: every row but one, and every row.)"""
    mask = _mask(rng, c.n, m)
    if m < c.n - 1:
        live = ~c.ex["dead"][: c.n].astype(bool)
        short = m - int((mask & live).sum())
        mask[rng.choice(np.flatnonzero(~mask & live), short, replace=False)] = True
        assert c.usable(mask) == m
    return mask


def _radii(c, mask):
    r10, idx = c.nth(mask, 10), np.arange(len(c.Q))
    mixed = np.where(idx % 4 == 0, np.float32(-1), c.nth(mask, 1))
    mixed = np.where(idx % 4 == 2, r10, mixed)
    mixed = np.where(idx % 4 == 3, c.nth(mask, 300), mixed).astype(np.float32)
    return {
        "tenth": r10,
        "below_tenth": np.nextafter(r10, np.float32(-np.inf)),
        "below_nearest": np.nextafter(c.nth(mask, 1), np.float32(-np.inf)),
        "mixed": mixed,
    }


@pytest.fixture(scope="module")
def built(H, O):
    """BUILD_BATCH graphs of in-bound data per (metric, dimension), rows DEL deleted"""
    out = {}
    for metric in (0, 1):
        for d in (20, 100):
            X, Q = _data(metric, d)
            out[metric, d] = Case(H, O, _graph(H, metric, X), metric, Q)
    yield out
    for c in out.values():
        c.g.close()


# ---------------------------------------------------------------- exact mode: allow-set sizes
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_allow_set_sizes(built, metric, d):
    c = built[metric, d]
    for m in SIZES:
        mask = _sized_mask(c, np.random.default_rng(1000 * metric + d + m), m)
        u = c.usable(mask)
        f = c.filter(mask)
        try:
            for name, rad in _radii(c, mask).items():
                got = c.check(mask, rad, f=f)
                cand, fb = c.g.get_option("last_range_candidates"), c.g.get_option("last_range_fallback_queries")
                print(m, u, name, "hits", int(got[0][-1]), "candidates", cand, "fallback", fb)
                if u >= 256:  # the filter GEMM over the gathered plane answers
                    assert fb == 0 and cand >= int(got[0][-1]), (m, name)
                else:  # below one row tile the sweep over the id list is the whole path
                    assert cand == 0, (m, name)
                if name == "below_nearest" or m == 0:
                    assert int(got[0][-1]) == 0
                if name == "tenth" and u >= 11 and metric == 1:  # a row at the boundary is a hit
                    assert (np.diff(got[0]) >= 10).all()
        finally:
            f.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_forced_sweep(built, metric):
    """the sweep over the id list equals the fused path byte for byte; fused and swept queries
    in one chunk"""
    c = built[metric, 100]
    mask = _sized_mask(c, np.random.default_rng(600 + metric), 600)
    f = c.filter(mask)
    try:
        rads = _radii(c, mask)
        fused = {k: c.check(mask, r, f=f) for k, r in rads.items()}
        c.g.set_option("range_force_fallback", 1)
        try:
            for k, r in rads.items():
                got = c.run(f, r)
                assert c.g.get_option("last_range_fallback_queries") == B
                assert c.g.get_option("last_range_candidates") == 0
                for x, y in zip(got, fused[k]):
                    assert x.tobytes() == y.tobytes()
        finally:
            c.g.set_option("range_force_fallback", 0)
        big = np.arange(B) % 3 == 1
        rad = np.where(big, np.float32(3e38), rads["tenth"]).astype(np.float32)
        got = c.check(mask, rad, f=f)
        assert c.g.get_option("last_range_fallback_queries") >= int(big.sum())
        assert (np.diff(got[0])[big] == c.lists(mask)[2][big]).all()
    finally:
        f.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_deleted_rows(H, O, metric):
    """a deleted row inside the allowed set, and an allowed row deleted after the filter was
    made: neither is ever a hit"""
    X, Q = _data(metric, 20)
    g = _graph(H, metric, X)
    try:
        c = Case(H, O, g, metric, Q)
        mask = _mask(np.random.default_rng(5), N, 400)
        mask[list(DEL)] = True  # deleted before the filter was made
        mask[[5, 100, 64]] = True
        f = c.filter(mask)
        every = np.float32(3e38)
        got = c.check(mask, every, f=f)
        gone = {int(c.keys[i]) for i in DEL}
        assert not set(got[1].tolist()) & gone
        later = [5, 64] + np.flatnonzero(mask)[10:200:7].tolist()
        later = [i for i in later if i not in DEL]
        assert all(g.BatchDelete([int(c.keys[i]) for i in later]))
        c.refresh()
        for rad in (every, c.nth(mask, 10)):
            got = c.check(mask, rad, f=f)
            assert not set(got[1].tolist()) & (gone | {int(c.keys[i]) for i in later})
        f.close()
    finally:
        g.close()


def test_no_filter_is_the_plain_search(built):
    """filter -1 and an all-rows filter: the plain range search, byte for byte"""
    c = built[1, 100]
    mask = np.ones(N, bool)
    rad = _radii(c, mask)["mixed"]
    plain = c.g.range_search_arrays(c.Q, rad)
    f = c.filter(mask)
    try:
        for filters in ([None] * B, f):
            got = c.g.range_search_arrays(c.Q, rad, filters=filters)
            for x, y in zip(got, plain):
                assert x.tobytes() == y.tobytes()
    finally:
        f.close()
    _same(plain, c.want(mask, rad))


def test_mixed_host_batch(built):
    """three filters, None and an empty one interleaved: each query equals its own
    single-filter call, lims is the concatenation"""
    c = built[0, 100]
    masks = [_sized_mask(c, np.random.default_rng(s), m) for s, m in ((1, 40), (2, 300), (3, 1000))]
    masks += [np.zeros(N, bool), None]
    fs = [c.filter(m) for m in masks[:4]] + [None]
    order = np.random.default_rng(9).integers(0, 5, B)
    order[:6] = [2, 4, 0, 1, 3, 4]
    rad = np.where(np.arange(B) % 2 == 0, c.nth(masks[1], 10), c.nth(masks[2], 40)).astype(np.float32)
    try:
        got = c.g.range_search_arrays(c.Q, rad, filters=[fs[i] for i in order])
        single = [c.g.range_search_arrays(c.Q, rad, filters=f) for f in fs]
        refs = [c.want(m, rad) for m in masks]
        for i in range(5):
            _same(single[i], refs[i])
        keys, dist, lims = [], [], [0]
        for b in range(B):
            sl, sk, sd = single[int(order[b])]
            keys.append(sk[sl[b]:sl[b + 1]])
            dist.append(sd[sl[b]:sl[b + 1]])
            lims.append(lims[-1] + int(sl[b + 1] - sl[b]))
        _same(got, (np.asarray(lims, np.int64), np.concatenate(keys), np.concatenate(dist)))
        assert lims[-1] > 0 and int(single[3][0][-1]) == 0
    finally:
        for f in fs[:4]:
            f.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_second_query_tile(H, O, metric):
    """B = 300: a second, ragged query tile over a gathered set of 600 rows"""
    X, Q = _data(metric, 20, nq=300)
    g = _graph(H, metric, X)
    try:
        c = Case(H, O, g, metric, Q)
        mask = _sized_mask(c, np.random.default_rng(7), 600)
        f = c.filter(mask)
        for name, rad in _radii(c, mask).items():
            got = c.check(mask, rad, f=f)
            assert g.get_option("last_range_fallback_queries") == 0
            assert g.get_option("last_range_candidates") >= int(got[0][-1])
        c.check(mask, np.float32(3e38), f=f)
        assert g.get_option("last_range_fallback_queries") == 300
        f.close()
    finally:
        g.close()


@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_edge_data_flat_index(H, O, metric, d):
    """a flat index with a zero query and rows and a query outside the fp16 bound, 700 rows
    allowed (the edge rows among them): parity on whichever path answers"""
    X, Q = _data(metric, d, edge=True)
    g = _graph(H, metric, X, flat=True)
    try:
        c = Case(H, O, g, metric, Q)
        mask = _sized_mask(c, np.random.default_rng(d), 696)
        mask[[120, 121, 122, 123]] = True
        f = c.filter(mask)
        for name, rad in _radii(c, mask).items():
            c.check(mask, rad, f=f)
        if metric == 0:  # every distance of the zero query is NaN
            assert c.lists(mask)[2][2] == 0
        c.check(mask, np.float32(3e38), f=f)
        with pytest.raises(H.HnswError, match="flat index") as e:
            c.run(f, c.nth(mask, 10), mode=H.MODE_BEAM, ef=64)
        assert e.value.code == H._lib.EUNSUPPORTED
        f.close()
    finally:
        g.close()


def test_stage_times(built):
    """a filtered exact pass also marks its row set's compaction and gather"""
    c = built[0, 100]
    mask = _sized_mask(c, np.random.default_rng(1), 600)
    f = c.filter(mask)
    try:
        c.run(f, c.nth(mask, 10))
        total = c.g.last_kernel_ms() * 1e6
        parts = [c.g.get_option(f"last_range_{s}_ns") for s in ("filter", "refine", "sweep", "order")]
        parts += [c.g.get_option(f"last_fx_{s}_ns") for s in ("compact", "gather")]
        assert all(p > 0 for p in parts) and sum(parts) <= total * 1.001
        with pytest.raises(c.H.HnswError):
            c.g.get_option("last_fx_rerank_ns")
        c.g.range_search_arrays(c.Q, c.nth(mask, 10))  # the plain call has no row set
        with pytest.raises(c.H.HnswError):
            c.g.get_option("last_fx_compact_ns")
    finally:
        f.close()


# ---------------------------------------------------------------- device entry
def test_device_entry_cap_and_stream(built):
    import torch

    c = built[1, 100]
    H, g = c.H, c.g
    dev = torch.device("cuda:0")
    mask = _sized_mask(c, np.random.default_rng(11), 513)
    f = c.filter(mask)
    rad = _radii(c, mask)["mixed"]
    host = c.check(mask, rad, f=f)
    total = int(host[0][-1])
    q = torch.from_numpy(c.Q).to(dev)
    r = torch.from_numpy(rad).to(dev)
    GUARD = 64
    s = torch.cuda.Stream()

    def call(cap, filt, **kw):
        lims = torch.full((B + 1,), -5, dtype=torch.int64, device=dev)
        keys = torch.full((cap + GUARD,), -7, dtype=torch.int64, device=dev)
        dist = torch.full((cap + GUARD,), -9.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.range_search_filtered_device(q.data_ptr(), B, c.Q.shape[1], r.data_ptr(), filt, cap, lims.data_ptr(),
                                           keys.data_ptr(), dist.data_ptr(), stream=s.cuda_stream, **kw)
        s.synchronize()
        g.device_status()
        return lims.cpu().numpy(), keys.cpu().numpy(), dist.cpu().numpy()

    try:
        assert total > 100
        for cap in (total, total + 100, total - 1, total // 2, 7, 0):
            lims, keys, dist = call(cap, f)
            m = min(cap, total)
            assert lims.tolist() == host[0].tolist(), cap  # the true prefix whatever fits
            assert keys[:m].tolist() == host[1][:m].tolist(), cap
            assert dist[:m].view(np.uint32).tolist() == host[2][:m].view(np.uint32).tolist(), cap
            assert (keys[m:] == -7).all() and (dist[m:] == -9.0).all(), cap  # nothing past the hits or the buffer
        # None: the plain range search on the stream
        plain = g.range_search_arrays(c.Q, rad)
        n = int(plain[0][-1])
        lims, keys, dist = call(n, None)
        assert lims.tolist() == plain[0].tolist() and keys[:n].tolist() == plain[1].tolist()
        # beam mode: the one filter for the batch is filled on the stream
        want = g.range_search_arrays(c.Q, rad, filters=f, mode=H.MODE_BEAM, ef=32, route=256)
        n = int(want[0][-1])
        lims, keys, dist = call(B * 32, f, mode=H.MODE_BEAM, ef=32, route=256)
        assert lims.tolist() == want[0].tolist() and keys[:n].tolist() == want[1].tolist()
        assert dist[:n].view(np.uint32).tolist() == want[2].view(np.uint32).tolist()
    finally:
        f.close()


# ---------------------------------------------------------------- beam mode
@pytest.mark.parametrize("ef", [16, 128])
@pytest.mark.parametrize("metric", [0, 1])
def test_beam_mode(built, metric, ef):
    """the filtered walk at k = ef through a route list of 256, cut by the radius"""
    c = built[metric, 20]
    H = c.H
    rg, T = FR.Graph(c.ex), FR.distance_table(c.O, c.ex, metric, c.Q)
    rng = np.random.default_rng(30 + metric)
    for mask in (np.ones(N, bool), rng.random(N) < 0.3):
        f = c.filter(mask)
        try:
            rk, rd, rn, _ = FR.search_batch(rg, T, [mask] * B, c.keys, ef, ef, 256)
            for rad in (c.nth(mask, 10), _radii(c, mask)["mixed"], np.float32(3e38)):
                got = c.run(f, rad, mode=H.MODE_BEAM, ef=ef, route=256)
                _same(got, _cut((rk, rd, rn), rad))
                exact = c.want(mask, rad)
                for b in range(B):  # a subset of the exact hits
                    assert set(got[1][got[0][b]:got[0][b + 1]].tolist()) <= \
                        set(exact[1][exact[0][b]:exact[0][b + 1]].tolist())
            assert np.array_equal(np.diff(got[0]), rn)  # 3e38: the whole list
            # a mix of filters and None in one launch
            mix = [f if b % 2 else None for b in range(B)]
            mk, md, mn, _ = FR.search_batch(rg, T, [mask if b % 2 else None for b in range(B)], c.keys, ef, ef, 256)
            rad = c.nth(mask, 10)
            _same(c.g.range_search_arrays(c.Q, rad, filters=mix, mode=H.MODE_BEAM, ef=ef, route=256),
                  _cut((mk, md, mn), rad))
        finally:
            f.close()


def test_beam_mode_limits(built):
    c = built[0, 20]
    H = c.H
    f = c.filter(np.ones(N, bool))
    try:
        with pytest.raises(H.HnswError, match=r"filtered search supports max\(ef,k\) <= 128") as e:
            c.run(f, 0.5, mode=H.MODE_BEAM, ef=129)
        assert e.value.code == H._lib.EUNSUPPORTED
        with pytest.raises(H.HnswError, match="filtered search supports route <= 2048") as e:
            c.run(f, 0.5, mode=H.MODE_BEAM, ef=16, route=2049)
        assert e.value.code == H._lib.EUNSUPPORTED
    finally:
        f.close()


# ---------------------------------------------------------------- after a mutation
@pytest.mark.parametrize("metric", [0, 1])
def test_after_compact_and_update(H, O, metric):
    """Compact() remaps the filter, update_arrays re-embeds allowed rows in place: the filter
    still answers, and the results equal a fresh reference"""
    X, Q = _data(metric, 20)
    g = _graph(H, metric, X)
    try:
        c = Case(H, O, g, metric, Q)
        mask = _sized_mask(c, np.random.default_rng(21), 600)
        allowed = c.keys[mask]
        f = c.filter(mask)
        c.check(mask, c.nth(mask, 10), f=f)
        assert g.Compact() == len(DEL)
        c.refresh()
        mask = np.isin(c.keys, allowed)
        assert c.n == N - len(DEL) and c.usable(mask) == 600
        for rad in _radii(c, mask).values():
            c.check(mask, rad, f=f)
        rows = np.flatnonzero(mask)[::9]
        moved = (X[::-1][: len(rows)] * np.float32(0.5)).astype(np.float32)
        assert g.update_arrays(c.keys[rows], moved).all()
        c.refresh()
        for rad in _radii(c, mask).values():
            got = c.check(mask, rad, f=f)
        assert int(got[0][-1]) > 0
        f.close()
    finally:
        g.close()


# ---------------------------------------------------------------- errors
def test_errors(built):
    import ctypes as C

    c = built[0, 20]
    H, g = c.H, c.g
    f = c.filter(_mask(np.random.default_rng(2), N, 300))
    with pytest.raises(H.HnswError, match="range search supports beam and exact mode") as e:
        c.run(f, 0.5, mode=H.MODE_COMPAT)
    assert e.value.code == H._lib.EUNSUPPORTED
    with pytest.raises(H.HnswError, match="embedding dimension mismatch") as e:
        g.range_search_arrays(c.Q[:, :7], 0.5, filters=f)
    assert e.value.code == H._lib.EDIM
    other = built[1, 20]
    fo = other.filter(np.ones(N, bool))
    with pytest.raises(H.HnswError, match="filter of another graph"):
        c.run(fo, 0.5)
    fo.close()
    lib = H.load()
    rad = np.full(B, 0.5, np.float32)
    lims = np.full(B + 1, -3, np.int64)

    def call(fo, mode=H.MODE_EXACT):
        fo = np.ascontiguousarray(fo, np.int32)
        return lib.mhnsw_range_search_filtered(g._h, c.Q.ctypes.data_as(C.POINTER(C.c_float)), B, c.Q.shape[1],
                                               rad.ctypes.data_as(C.POINTER(C.c_float)), mode, 16, 0,
                                               fo.ctypes.data_as(C.POINTER(C.c_int32)),
                                               lims.ctypes.data_as(C.POINTER(C.c_int64)))

    fid = f.id
    for mode in (H.MODE_EXACT, H.MODE_BEAM):
        assert call(np.full(B, 999), mode) == H._lib.EINVAL
        assert lib.mhnsw_last_error(g._h).decode() == "unknown filter 999"
        mixed = np.full(B, fid)
        mixed[7], mixed[8] = -1, 1000
        assert call(mixed, mode) == H._lib.EINVAL
        assert lib.mhnsw_last_error(g._h).decode() == "unknown filter 1000"
        assert (lims == -3).all()  # refused before any pass wrote a result
    f.close()  # a destroyed filter
    assert call(np.full(B, fid)) == H._lib.EINVAL
    assert lib.mhnsw_last_error(g._h).decode() == f"unknown filter {fid}"
    with pytest.raises(H.HnswError, match="unknown filter"):
        c.run(f, 0.5)
    rc = lib.mhnsw_range_search_filtered_device(g._h, None, B, c.Q.shape[1], None, H.MODE_EXACT, 0, 0, fid, 10, None,
                                                None, None, None)
    assert rc == H._lib.EINVAL and lib.mhnsw_last_error(g._h).decode() == f"unknown filter {fid}"
    rc = lib.mhnsw_range_search_filtered_device(g._h, None, B, c.Q.shape[1], None, H.MODE_COMPAT, 0, 0, -1, 10, None,
                                                None, None, None)
    assert rc == H._lib.EUNSUPPORTED
