"""GPU: the LSH index (lsh.hip; mhnsw_lsh_* / mhnsw_search_lsh*; Graph.EnableLSH, SearchLSH,
adapters.LSHIndex).

Codes: bit i of table t = (canonical f32 dot of the row and projection t b + i) > 0, the sign of
oracle og_dev_sum.  Search: keys, distance bits, n and ncand equal the oracle's MODE_EXACT search
of the export with every row outside the query's candidate set in the dead flags (the
construction of tests/test_gpu_filtered_exact.py Case.ref, once per query).
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_filtered_exact import Case, _batch_graph, _same
from tests.test_gpu_parity import _metric_fn

pytestmark = pytest.mark.gpu

N, B = 1531, 16  # 1531 = 23 * 64 + 59: a tail row tile; the buckets' walks end in tails of 64 ids
_F = C.POINTER(C.c_float)


def _keys(n):
    return np.arange(n, dtype=np.int64) * 3 + 1


def _pack(S, T, b):
    """signs bool[n, T * b] -> codes uint32[n, T]"""
    return (S.reshape(len(S), T, b).astype(np.uint64) << np.arange(b, dtype=np.uint64)).sum(2).astype(np.uint32)


def _canon(O, X, P, T, b):
    """the reference codes: signs of the canonical sums"""
    L = O.lib()
    L.og_dev_sum.restype, L.og_dev_sum.argtypes = C.c_float, [_F, _F, C.c_int, C.c_int]
    X, P = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(P, np.float32)
    S = [[L.og_dev_sum(x.ctypes.data_as(_F), p.ctypes.data_as(_F), X.shape[1], 0) > 0 for p in P] for x in X]
    return _pack(np.array(S, bool), T, b)


def _flat(H, X, metric=0):
    g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), build_mode=H.BUILD_FLAT)
    g.add_arrays(_keys(len(X)), X)
    return g


# ---------------------------------------------------------------- codes
@pytest.mark.parametrize("T,b", [(1, 1), (4, 8), (3, 11), (8, 32)])
@pytest.mark.parametrize("d", [20, 100])
def test_codes_exact_data(H, d, T, b):
    """small integers: every f32 summation order gives the exact dot, zeros included"""
    rng = np.random.default_rng(d + T)
    X = rng.integers(-3, 4, (N, d)).astype(np.float32)
    P = rng.integers(-3, 4, (T * b, d)).astype(np.float32)
    X[3] = 0
    X[4, 2:] = 0
    P[0, :2] = 0  # row 4 . projection 0 == 0 exactly: the comparison is strict
    Q = rng.integers(-3, 4, (B, d)).astype(np.float32)
    dots = X.astype(np.int64) @ P.astype(np.int64).T
    assert (dots == 0).sum() >= 2
    g = _flat(H, X)
    try:
        g.EnableLSH(T, b, projections=P)
        assert np.array_equal(g.lsh_codes(), _pack(dots > 0, T, b))
        assert np.array_equal(g.lsh_hash(Q), _pack(Q.astype(np.int64) @ P.astype(np.int64).T > 0, T, b))
        assert np.array_equal(g.lsh_projections(), P)
    finally:
        g.close()


@pytest.mark.parametrize("cap", [None, 1])  # 1: the worklist overflows, the whole launch is redone canonically
@pytest.mark.parametrize("d", [20, 100])
def test_codes_rounding_noise(H, O, d, cap):
    T, b = 4, 8
    rng = np.random.default_rng(7 + d)
    X = rng.uniform(-1, 1, (N, d)).astype(np.float32)
    P = rng.normal(size=(T * b, d)).astype(np.float32)
    near = list(range(10, 30)) + [N - 1]  # projected off projection r % 32's hyperplane, in f32
    for r in near:
        p = P[r % 32]
        X[r] = X[r] - np.float32(np.dot(X[r], p) / np.dot(p, p)) * p
    # from the reference alone: such a pair lies inside the standard bound 2 gamma_d |x| |p|, which
    # the kernel's margin contains, so the canonical pass decides it
    u = 2.0 ** -24
    g2 = 2 * d * u / (1 - d * u)
    x64, p64 = X[near].astype(np.float64), P[[r % 32 for r in near]].astype(np.float64)
    mag = np.abs((x64 * p64).sum(1))
    assert (mag <= g2 * np.linalg.norm(x64, axis=1) * np.linalg.norm(p64, axis=1)).any()
    g = _flat(H, X)
    try:
        if cap is not None:
            g.set_option("lsh_worklist_cap", cap)
        g.EnableLSH(T, b, projections=P)
        assert np.array_equal(g.lsh_codes(), _canon(O, X, P, T, b))
        assert g.get_option("last_lsh_uncertain") > 0
    finally:
        g.close()


def test_codes_do_not_depend_on_batching(H):
    """one Add against three uneven ones; enabled before the first Add and after the last"""
    X = np.random.default_rng(3).uniform(-1, 1, (N, 100)).astype(np.float32)
    a = _flat(H, X)
    b = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=H.CosineDistance, build_mode=H.BUILD_FLAT)
    try:
        b.EnableLSH()
        for lo, hi in ((0, 1), (1, 778), (778, N)):
            b.add_arrays(_keys(N)[lo:hi], X[lo:hi])
        a.EnableLSH(0, 0)  # the defaults, 4 x 8
        assert a.get_option("lsh_tables") == 4 and a.get_option("lsh_bits") == 8
        assert np.array_equal(a.lsh_projections(), b.lsh_projections())
        assert np.array_equal(a.lsh_codes(), b.lsh_codes())
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- search against the oracle
def _data(metric, d, n=N):
    """rows and queries around a common offset (big buckets), duplicates, a zero row; query 2
    opposite to the offset (its buckets are nearly empty), queries 8.. without the offset"""
    rng = np.random.default_rng(100 * metric + d)
    X = (rng.uniform(-1, 1, (n, d)) + 0.6).astype(np.float32)
    X[100:110] = X[5]
    X[900 % n] = X[64]
    X[7] = 0
    Q = (rng.uniform(-1, 1, (B, d)) + 0.6).astype(np.float32)
    Q[0], Q[1], Q[2] = X[5], X[64] * 1.5, -0.6
    Q[8:] -= 0.6
    return rng, X, Q, rng.normal(size=(32, d)).astype(np.float32)


def _check(O, c, P, T, b, k):
    """codes, then per query the oracle's exact search over its candidate set"""
    X = c.ex["vecs"].reshape(c.n, -1)
    rc, qc = _canon(O, X, P, T, b), _canon(O, c.Q, P, T, b)
    assert np.array_equal(c.g.lsh_codes(), rc)
    masks = (rc[None] == qc[:, None]).any(2) & ~c.ex["dead"].astype(bool)[None]
    got = c.g.search_lsh_arrays(c.Q, k)
    assert np.array_equal(got[3], masks.sum(1)), (got[3], masks.sum(1))
    for q in range(len(c.Q)):
        _same(tuple(a[q:q + 1] for a in got[:3]), c.ref(masks[q], k, c.Q[q:q + 1]))
    return masks.sum(1)


@pytest.fixture(scope="module")
def built(H, O):
    out = {}
    for metric in (0, 1):
        for d in (20, 100):
            _, X, Q, P = _data(metric, d)
            out[metric, d] = Case(H, O, _batch_graph(H, metric, X), metric, Q), P
    yield out
    for c, _ in out.values():
        c.g.close()


@pytest.mark.parametrize("screen", [0, 1])
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_search_against_oracle(O, built, metric, d, screen):
    c, P = built[metric, d]
    c.g.set_option("screen", screen)
    c.g.EnableLSH(2, 2, projections=P[:4])  # 4 buckets a table: full lists, the screen acts
    for k in (1, 10, 256):
        nc = _check(O, c, P[:4], 2, 2, k)
    assert nc.max() > 256
    c.g.EnableLSH(4, 8, projections=P)
    qc, rc = _canon(O, c.Q, P, 4, 8), _canon(O, c.ex["vecs"].reshape(c.n, -1), P, 4, 8)
    nc = (rc[None] == qc[:, None]).any(2).sum(1)
    assert (nc == 0).any() and ((nc > 0) & (nc < 10)).any()  # from the reference masks alone
    _check(O, c, P, 4, 8, 10)
    assert c.g.get_option("last_lsh_candidates") == nc.sum() and c.g.get_option("last_lsh_rebuild_ns") > 0


def test_mutations(H, O):
    """each step against the reference of the new export"""
    n = 700
    _, X, Q, P = _data(0, 20, n + 100)
    g = _batch_graph(H, 0, X[:n])
    try:
        g.EnableLSH(4, 8, projections=P)  # on a handle that already holds rows
        c = Case(H, O, g, 0, Q)
        _check(O, c, P, 4, 8, 10)
        first = int(g.search_lsh_arrays(Q[:1], 1)[0][0, 0])
        assert g.Delete(first)
        c.refresh()
        _check(O, c, P, 4, 8, 10)
        g.add_arrays(_keys(n + 100)[n:], X[n:])
        c.refresh()
        _check(O, c, P, 4, 8, 10)
        before = g.lsh_codes()[[20, 21]]
        assert g.update_arrays(_keys(n)[[20, 21]], -X[[20, 21]]).all()  # -x: every nonzero sign flips
        assert (g.lsh_codes()[[20, 21]] != before).any()
        c.refresh()
        _check(O, c, P, 4, 8, 10)
        assert g.Compact() == 1
        c.refresh()
        assert c.n == n + 99
        _check(O, c, P, 4, 8, 10)
    finally:
        g.close()


# ---------------------------------------------------------------- hosts and errors
def test_lsh_index_adapter(H):
    _, X, Q, P = _data(1, 20, 300)
    ix = H.LSHIndex(4, 8, H.EuclideanDistance, projections=P)
    assert ix.Search(Q[0], 3) == ([], []) and ix.Len() == 0
    ix.BatchAdd([f"k{i:03d}" for i in range(300)], list(X))  # string keys
    keys, dist = ix.Search(X[17], 2)
    assert keys[0] == "k017" and dist[0] == 0.0
    ix.Add("k017", X[200])  # replace-on-add: the key moves to row 200's buckets
    keys, dist = ix.Search(X[200], 2)
    assert keys == ["k017", "k200"] and dist == [0.0, 0.0] and ix.Len() == 300
    assert ix.Delete("k200") and ix.BatchDelete(["k017", "nope"]) == [True, False]
    ks, od, on, nc = ix.search_batch(Q, 5)
    assert all("k017" not in k and "k200" not in k for k in ks) and (on <= np.minimum(nc, 5)).all()
    ix.Close()


def test_device_entry_on_a_second_stream(H, built):
    import torch

    c, P = built[0, 20]
    c.g.EnableLSH(4, 8, projections=P)
    k = 10
    want = c.g.search_lsh_arrays(c.Q, k)
    q = torch.from_numpy(c.Q).cuda()
    ok = torch.full((B * k + 2,), -7, dtype=torch.int64, device="cuda")
    od = torch.full((B * k + 2,), -7.0, dtype=torch.float32, device="cuda")
    on = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    nc = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    c.g.search_lsh_device(q.data_ptr(), B, 20, k, ok[1:].data_ptr(), od[1:].data_ptr(), on[1:].data_ptr(),
                          nc[1:].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    c.g.device_status()
    for t in (ok, od, on, nc):  # guard words
        assert t[0].item() == -7 and t[-1].item() == -7
    got = (ok[1:-1].cpu().numpy().reshape(B, k), od[1:-1].cpu().numpy().reshape(B, k), on[1:-1].cpu().numpy())
    _same(got, want[:3])
    assert np.array_equal(nc[1:-1].cpu().numpy(), want[3])


def test_refusals(H):
    X = np.random.default_rng(1).uniform(-1, 1, (40, 20)).astype(np.float32)
    g = _flat(H, X)
    try:
        with pytest.raises(H.HnswError, match="LSH search before mhnsw_lsh_enable"):
            g.search_lsh_arrays(X[:2], 3)
        for args in ((257, 1), (9, 32), (1, 33)):  # T b = 257 (T > 32), T b = 288, b = 33
            with pytest.raises(H.HnswError):
                g.EnableLSH(*args)
        with pytest.raises(H.HnswError):
            g.EnableLSH(4, 8, projections=np.zeros((31, 20), np.float32))
        with pytest.raises(H.HnswError, match="dimension"):
            g.EnableLSH(4, 8, projections=np.zeros((32, 21), np.float32))
        g.EnableLSH(4, 8)
        with pytest.raises(H.HnswError, match="k <= 256"):
            g.search_lsh_arrays(X[:2], 257)
    finally:
        g.close()
