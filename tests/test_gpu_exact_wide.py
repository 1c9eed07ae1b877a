"""GPU: the wide exact search (wide.hip; option "exact_wide"): MODE_EXACT at 256 < k <= 4096
through the range pipeline, plain and filtered, host and device entries.

One contract: keys, distance bits and counts equal the oracle's MODE_EXACT search at the same
k on an export of the graph (for a filtered call: imported with dead[i] = 1 for every row that
is deleted or not allowed, as tests/test_gpu_filtered_exact.py does).  The oracle's list at k
is the first k entries of its list at k = rows (one order, by (distance, row id)), so each
data set is searched once at k = rows and cut.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import _bit_equal, _metric_fn

pytestmark = pytest.mark.gpu

N, D, B = 3000, 24, 300  # 11 full row tiles and a tail of 184 rows; a second, ragged query tile
KS = (257, 300, 1000, 2999, 3000, 3500, 4096)  # the last two are past the row count


def _graph(H, metric, X, keys=None, **opt):
    g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), build_mode=H.BUILD_FLAT, exact_wide=1, **opt)
    g.add_arrays(np.arange(len(X), dtype=np.int64) * 3 + 1 if keys is None else keys, X)
    return g


def _full(O, g, metric, Q, mask=None):
    """the oracle's whole (distance, row id) list per query: (keys, dist, n) at k = rows"""
    ex = g.export()
    n = len(ex["keys"])
    dead = ex["dead"].astype(bool)
    if mask is not None:
        dead = dead | ~np.asarray(mask, bool)
    if dead.all():
        return np.zeros((len(Q), 1), np.int64), np.zeros((len(Q), 1), np.float32), np.zeros(len(Q), np.int32)
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64)
    o.import_graph(ex["keys"], ex["vecs"], ex["deg"], ex["adj"], ex["entry"], dead.astype(np.uint8))
    return o.search(Q, n, mode=O.MODE_EXACT)


def _same(got, full, k, rows=None):
    gk, gd, gn = got
    rk, rd, rn = full
    rows = range(len(gn)) if rows is None else rows
    for i, b in enumerate(rows):
        n = min(k, int(rn[b]))
        assert gn[i] == n, (b, gn[i], n)
        assert gk[i, :n].tolist() == rk[b, :n].tolist(), b
        assert _bit_equal(gd[i, :n], rd[b, :n]), b


def _data(metric, d=D, n=N, nq=B, seed=0):
    rng = np.random.default_rng(1000 * metric + d + seed)
    X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    X[100:110] = X[5]  # duplicates: equal distances come out in row order
    Q = rng.uniform(-1, 1, (nq, d)).astype(np.float32)
    Q[0] = X[5]
    return X, Q


class Case:
    def __init__(self, H, O, metric, X, Q, **opt):
        self.H, self.O, self.metric, self.X, self.Q = H, O, metric, X, Q
        self.g = _graph(H, metric, X, **opt)
        self.full = _full(O, self.g, metric, Q)

    def check(self, k, nq=None, **kw):
        Q = self.Q[:nq]
        got = self.g.search_arrays(Q, k, mode=self.H.MODE_EXACT, **kw)
        assert self.g.get_option("last_wide_queries") == len(Q)
        _same(got, self.full, k)
        return got


@pytest.fixture(scope="module")
def cases(H, O):
    """per metric: 3000 x 24 rows, the 12 row tiles sampled at stride 4 (exact_sample 3)"""
    out = {m: Case(H, O, m, *_data(m), exact_sample=3) for m in (0, 1)}
    yield out
    for c in out.values():
        c.g.close()


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", [0, 1])
def test_shapes(cases, metric, k):
    c = cases[metric]
    c.check(k)  # B = 300: a second query tile, ragged
    hits, fb = c.g.get_option("last_wide_hits"), c.g.get_option("last_wide_fallback_queries")
    print("k", k, "J", c.g.get_option("last_wide_rank"), "room", c.g.get_option("last_wide_room"), "hits / (B k)",
          hits / (B * k), "fallback", fb)
    if k in (257, 300, 1000):  # the estimate is possible (J fits the 768 sampled rows): most queries take it
        assert fb < B // 2
        assert hits >= (B - fb) * k
    else:  # J exceeds the sample, or k the rows: every query is short
        assert fb == B
    c.check(k, nq=48)


@pytest.mark.parametrize("metric", [0, 1])
def test_default_sample(H, O, metric):
    """the default sample takes every full row tile (stride 1): J = k, the radius provably holds k rows"""
    X, Q = _data(metric, nq=48)
    c = Case(H, O, metric, X, Q)
    try:
        assert c.g.get_option("exact_sample") == 64
        for k in (300, 1000):
            c.check(k)
            assert c.g.get_option("last_wide_rank") == k
            assert c.g.get_option("last_wide_fallback_queries") == 0
    finally:
        c.g.close()


def test_dim_768(H, O):
    X, Q = _data(0, d=768, n=1531, nq=48)
    c = Case(H, O, 0, X, Q, exact_sample=3)
    try:
        for k in (300, 1531, 4096):
            c.check(k)
    finally:
        c.g.close()


# ---------------------------------------------------------------- the estimate fails
def _clustered(near_in_sample):
    """rows near the queries in the sampled tiles (0, 4, 8) and far ones elsewhere, or the reverse"""
    rng = np.random.default_rng(7)
    centre = rng.uniform(-1, 1, D).astype(np.float32)
    tile = np.arange(N) // 256
    sampled = (tile % 4 == 0) & (tile < 11)
    near = sampled if near_in_sample else ~sampled
    # (the near rows' spread is far above the score error the radius is widened by: about 0.07
    # on a squared L2 distance near 6)
    X = (centre + rng.normal(0, 1, (N, D)) * np.where(near, 0.5, 2.0)[:, None]).astype(np.float32)
    Q = (centre + rng.normal(0, 0.02, (48, D))).astype(np.float32)
    return X, Q


@pytest.mark.parametrize("near_in_sample", [True, False], ids=["low", "high"])
@pytest.mark.parametrize("metric", [0, 1])
def test_estimate_fails(H, O, metric, near_in_sample):
    """low: the radius holds fewer than k rows.  high: it admits nearly every row and the room
    is exceeded.  Either way the fallback answers, identically."""
    X, Q = _clustered(near_in_sample)
    c = Case(H, O, metric, X, Q, exact_sample=3)
    try:
        c.check(500)
        assert c.g.get_option("last_wide_rank") <= 768
        assert c.g.get_option("last_wide_fallback_queries") > 0
    finally:
        c.g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_forced_fallback(cases, metric):
    c = cases[metric]
    fused = c.check(300, nq=48)
    c.g.set_option("wide_force_fallback", 1)
    try:
        forced = c.check(300, nq=48)
        assert c.g.get_option("last_wide_fallback_queries") == 48
        assert c.g.get_option("last_wide_hits") == 0
    finally:
        c.g.set_option("wide_force_fallback", 0)
    for a, b in zip(fused, forced):
        assert a.tobytes() == b.tobytes()
    # groups of the fallback smaller than the short list
    c.g.set_option("wide_fallback_bytes", 4 * 3008 * 7)
    try:
        c.check(3000, nq=48)
    finally:
        c.g.set_option("wide_fallback_bytes", 1 << 30)


@pytest.mark.parametrize("metric", [0, 1])
def test_below_one_row_tile(H, O, metric):
    X, Q = _data(metric, n=200, nq=48)
    c = Case(H, O, metric, X, Q)
    try:
        for k in (257, 4096):
            c.check(k)
            assert c.g.get_option("last_wide_fallback_queries") == 48
    finally:
        c.g.close()


# ---------------------------------------------------------------- ties
def test_integer_ties(H, O):
    rng = np.random.default_rng(3)
    X = rng.integers(0, 3, (N, 4)).astype(np.float32)  # 81 distinct rows: massive exact ties at every rank
    Q = rng.integers(0, 3, (48, 4)).astype(np.float32)
    for opt in ({"exact_sample": 3}, {}):
        c = Case(H, O, 1, X, Q, **opt)
        try:
            for k in (300, 1000):
                c.check(k)
        finally:
            c.g.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_identical_rows(H, O, metric):
    X, Q = _data(metric, n=1000, nq=48)
    X[:600] = X[0]
    keys = np.arange(1000, dtype=np.int64)
    Q[:8] = X[0]
    g = _graph(H, metric, X, keys=keys)
    try:
        full = _full(O, g, metric, Q)
        for force in (0, 1):
            g.set_option("wide_force_fallback", force)
            got = g.search_arrays(Q, 300, mode=H.MODE_EXACT)
            _same(got, full, 300)
            for b in range(8):
                assert got[0][b].tolist() == list(range(300)), b
    finally:
        g.close()


def test_one_ulp_neighbours(H, O):
    v = np.float32(1.0)
    col = []
    for _ in range(N):
        col.append(v)
        v = np.nextafter(v, np.float32(2))
    X = np.zeros((N, 4), np.float32)
    X[:, 0] = np.random.default_rng(5).permutation(np.asarray(col, np.float32))
    Q = np.zeros((48, 4), np.float32)
    Q[:, 0] = np.linspace(-1, 1, 48, dtype=np.float32) * np.float32(1e-3)
    c = Case(H, O, 1, X, Q, exact_sample=3)
    try:
        for k in (300, 1000):
            c.check(k)
    finally:
        c.g.close()


# ---------------------------------------------------------------- row states
@pytest.mark.parametrize("metric", [0, 1])
def test_row_states(H, O, metric):
    X, Q = _data(metric, nq=48, seed=1)
    X[31] = 0  # NaN under cosine
    X[300] = 0
    X[120] *= np.float32(1e20)  # outside the fp16 bound, either side
    X[121] *= np.float32(1e-20)
    X[2900] *= np.float32(1e20)
    Q[2] = 0
    Q[5] *= np.float32(1e-20)
    Q[6] *= np.float32(1e20)
    g = _graph(H, metric, X, exact_sample=3)
    try:
        gone = [int(i) * 3 + 1 for i in (7, 300, 1200, 2999) + tuple(range(2000, 2100))]
        for step in ("fresh", "deleted", "compacted"):
            if step == "deleted":
                assert all(g.BatchDelete(gone))
            if step == "compacted":
                assert g.Compact() == len(gone)
            full = _full(O, g, metric, Q)
            for k in (300, 1000, 3000):
                got = g.search_arrays(Q, k, mode=H.MODE_EXACT)
                _same(got, full, k)
                if metric == 0:
                    assert got[2][2] == 0  # the zero query: every distance NaN
    finally:
        g.close()


# ---------------------------------------------------------------- old path against new, gates
@pytest.mark.parametrize("metric", [0, 1])
def test_old_against_new(cases, metric):
    c = cases[metric]
    g = c.g
    for k in (1, 10, 256):
        g.set_option("exact_wide_min_k", 257)
        old = g.search_arrays(c.Q, k, mode=c.H.MODE_EXACT)
        assert g.get_option("last_wide_queries") == 0  # k <= 256 takes today's path by default
        g.set_option("exact_wide_min_k", 1)
        try:
            new = g.search_arrays(c.Q, k, mode=c.H.MODE_EXACT)
            assert g.get_option("last_wide_queries") == B
        finally:
            g.set_option("exact_wide_min_k", 257)
        assert old[2].tolist() == new[2].tolist() == [k] * B
        assert old[0].tobytes() == new[0].tobytes()
        assert old[1].tobytes() == new[1].tobytes()


def test_gates(cases):
    c = cases[1]
    g, H = c.g, c.H
    assert g.get_option("exact_wide") == 1 and g.get_option("exact_wide_min_k") == 257
    with pytest.raises(H.HnswError, match=r"exact mode supports k <= 4096"):
        g.search_arrays(c.Q[:4], 4097, mode=H.MODE_EXACT)
    f = g.Filter([1, 4, 7])
    try:
        with pytest.raises(H.HnswError, match=r"exact mode supports k <= 4096"):
            g.search_filtered_arrays(c.Q[:4], 4097, f, mode=H.MODE_EXACT)
        with pytest.raises(H.HnswError, match=r"exact mode supports k <= 4096"):
            g.search_filtered_arrays(c.Q[:4], 4097, [f, None, f, None], mode=H.MODE_EXACT)
        g.set_option("exact_wide", 0)
        try:
            with pytest.raises(H.HnswError, match=r"exact mode supports k <= 256"):
                g.search_arrays(c.Q[:4], 257, mode=H.MODE_EXACT)
            with pytest.raises(H.HnswError, match=r"exact mode supports k <= 256"):
                g.search_filtered_arrays(c.Q[:4], 257, f, mode=H.MODE_EXACT)
            with pytest.raises(H.HnswError, match=r"exact mode supports k <= 256"):
                g.search_filtered_arrays(c.Q[:4], 257, [f, None, f, None], mode=H.MODE_EXACT)
        finally:
            g.set_option("exact_wide", 1)
    finally:
        f.close()
    for name, bad in (("exact_wide", 2), ("exact_wide_min_k", 0), ("wide_force_fallback", -1), ("wide_fallback_bytes", 0)):
        with pytest.raises(H.HnswError):
            g.set_option(name, bad)


# ---------------------------------------------------------------- filtered
def _mask(rng, n, m):
    mask = np.zeros(n, bool)
    mask[rng.choice(n, m, replace=False)] = True
    return mask


@pytest.mark.parametrize("metric", [0, 1])
def test_filtered_sizes(cases, metric):
    c = cases[metric]
    g, H = c.g, c.H
    keys = np.arange(N, dtype=np.int64) * 3 + 1
    rng = np.random.default_rng(11)
    Q = c.Q[:48]
    for m in (0, 1, 255, 256, 257, 513, N - 1, N):
        mask = _mask(rng, N, m)
        f = g.Filter(keys[mask].tolist())
        try:
            got = g.search_filtered_arrays(Q, 300, f, mode=H.MODE_EXACT)
        finally:
            f.close()
        _same(got, _full(c.O, g, metric, Q, mask), 300)
        assert got[2].tolist() == [min(300, m)] * 48, m
        # (of the last exact search, however it ended: nothing allowed returns before any kernel)
        assert g.get_option("last_wide_queries") == (48 if m else 0), m


def test_filtered_mixed_batch(cases):
    c = cases[1]
    g, H = c.g, c.H
    keys = np.arange(N, dtype=np.int64) * 3 + 1
    rng = np.random.default_rng(12)
    masks = [_mask(rng, N, 700), _mask(rng, N, 2000)]
    fs = [g.Filter(keys[m].tolist()) for m in masks]
    Q = c.Q[:48]
    try:
        which = [b % 3 for b in range(48)]  # 0, 1: a filter; 2: every live row
        got = g.search_filtered_arrays(Q, 400, [fs[w] if w < 2 else None for w in which], mode=H.MODE_EXACT)
    finally:
        for f in fs:
            f.close()
    for w in range(3):
        rows = [b for b in range(48) if which[b] == w]
        full = _full(c.O, g, 1, Q, masks[w] if w < 2 else None)
        _same(tuple(a[rows] for a in got), full, 400, rows)


# ---------------------------------------------------------------- device entry
def test_device_entry_streams(cases):
    """two streams back to back on one handle, guard words behind [B, k]; nothing but the
    caller's synchronize between the enqueue and the read"""
    import torch

    c = cases[1]
    g, H = c.g, c.H
    dev = torch.device("cuda:0")
    nq, GUARD = 48, 64
    Q = c.Q[:nq]
    q = torch.from_numpy(Q).to(dev)
    keys = np.arange(N, dtype=np.int64) * 3 + 1
    mask = _mask(np.random.default_rng(13), N, 1500)
    f = g.Filter(keys[mask].tolist())
    want_f = _full(c.O, g, 1, Q, mask)

    def alloc(k):
        ok = torch.full((nq * k + GUARD,), -7, dtype=torch.int64, device=dev)
        od = torch.full((nq * k + GUARD,), -9.0, dtype=torch.float32, device=dev)
        on = torch.full((nq + GUARD,), -5, dtype=torch.int32, device=dev)
        return k, ok, od, on

    def enqueue(res, stream, filt=None):
        k, ok, od, on = res
        with torch.cuda.stream(stream):
            if filt is None:
                g.search_device(q.data_ptr(), nq, D, k, ok.data_ptr(), od.data_ptr(), on.data_ptr(), mode=H.MODE_EXACT,
                                stream=stream.cuda_stream)
            else:
                g.search_filtered_exact_device(q.data_ptr(), nq, D, k, filt, ok.data_ptr(), od.data_ptr(), on.data_ptr(),
                                               stream=stream.cuda_stream)

    def verify(res, full):
        k, ok, od, on = res
        ok, od, on = ok.cpu().numpy(), od.cpu().numpy(), on.cpu().numpy()
        assert (ok[nq * k:] == -7).all() and (od[nq * k:] == -9.0).all() and (on[nq:] == -5).all()
        _same((ok[: nq * k].reshape(nq, k), od[: nq * k].reshape(nq, k), on[:nq]), full, k)

    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        for _ in range(2):
            a, b, d = alloc(300), alloc(1000), alloc(3500)
            torch.cuda.synchronize()  # the buffers are filled; from here to the next synchronize only enqueues
            enqueue(a, sa)
            enqueue(b, sb, f)  # the other stream: waits for the handle's scratch, not for the host
            enqueue(d, sa)
            torch.cuda.synchronize()
            verify(a, c.full)
            verify(b, want_f)
            verify(d, c.full)
        g.device_status()
    finally:
        f.close()


# ---------------------------------------------------------------- keys and the flat index
def test_string_keys(H, O):
    """string keys through the key map: the oracle's rows at the same k, each row's name"""
    X, Q = _data(0, n=700, nq=4)
    names = ["key%04d" % ((i * 37) % 700) for i in range(700)]  # row i holds names[i]: not in key order
    g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=H.CosineDistance, build_mode=H.BUILD_FLAT, exact_wide=1)
    try:
        g.BatchAdd([H.Node(k, v) for k, v in zip(names, X)])
        ex = g.export()
        row_of = {int(k): i for i, k in enumerate(ex["keys"])}
        assert g.decode_keys(ex["keys"]) == names
        rk, rd, rn = _full(O, g, 0, Q)
        for force in (0, 1):
            g.set_option("wide_force_fallback", force)
            for b in range(4):
                for k in (300, 700):
                    got = g.Search(Q[b], k, mode=H.MODE_EXACT)
                    n = min(k, int(rn[b]))
                    assert [node.Key for node in got] == [names[row_of[int(x)]] for x in rk[b, :n]], (force, b, k)
    finally:
        g.close()


def test_exact_index_wide(H, O):
    X, Q = _data(0, n=900, nq=4)
    ix = H.ExactIndex(H.CosineDistance, wide=True)
    plain = H.ExactIndex(H.CosineDistance)
    try:
        keys = list(range(900))
        ix.BatchAdd(keys, list(X))
        plain.BatchAdd(keys[:10], list(X[:10]))
        with pytest.raises(H.HnswError, match=r"exact mode supports k <= 256"):
            plain.Search(Q[0], 300)
        ix.BatchAdd([5, 6], [X[800], X[801]])  # replace in place
        assert all(ix.BatchDelete([17, 18, 19]))
        Xn = X.copy()
        Xn[5], Xn[6] = X[800], X[801]
        live = np.ones(900, bool)
        live[[17, 18, 19]] = False
        full = _full(O, ix._g, 0, Q)
        got = ix.search_batch(Q, 400)
        for b in range(4):
            assert got[2][b] == 400
            assert list(got[0][b]) == full[0][b, :400].tolist()
            assert _bit_equal(got[1][b, :400], full[1][b, :400])
        assert not {17, 18, 19} & set(got[0][0])
        res = ix.Search(Q[1], 897)
        assert [n.Key for n in res] == full[0][1, :897].tolist()
        f = ix.Filter(range(0, 900, 2))
        try:
            fl = ix.SearchFiltered(Q[2], 300, f)
            m = np.zeros(900, bool)
            m[::2] = True
            assert [n.Key for n in fl] == _full(O, ix._g, 0, Q, m)[0][2, :300].tolist()
        finally:
            f.close()
    finally:
        ix.Close()
        plain.Close()
