"""GPU: the partitions (part.hip; mhnsw_part_* / mhnsw_search_part*; Graph.EnablePartitions,
SearchPartitions, adapters.Partitioner).

Probe order: the centroids by (oracle og_distance(metric, OG_ORDER_DEV, x, c), index), NaN last; a
row's partition is its first entry.  Search: keys, distance bits, n and ncand equal the oracle's
MODE_EXACT search of the export with every row outside the probed partitions in the dead flags
(tests/test_gpu_filtered_exact.py Case.ref, once per query).
"""
import numpy as np
import pytest

from tests.test_gpu_filtered_exact import Case, _batch_graph, _same
from tests.test_gpu_parity import _metric_fn

pytestmark = pytest.mark.gpu

N, B = 1531, 16  # 1531 = 23 * 64 + 59: a tail row tile; P 3 / 64 / 70: below one centroid tile, one, one and a tail


def _keys(n):
    return np.arange(n, dtype=np.int64) * 3 + 1


def _order(O, metric, X, Cn):
    """the reference probe orders int[n, P] and the distances they come from"""
    n, P = len(X), len(Cn)
    ia, ib = np.repeat(np.arange(n), P), np.tile(np.arange(P), n) + n
    D = O.distance_pairs(metric, O.ORDER_DEV, np.vstack([X, Cn]), ia, ib).reshape(n, P)
    return np.argsort(D, axis=1, kind="stable"), D  # (NaN sorts last, equal distances keep the index order)


def _flat(H, X, metric):
    g = H.Graph(M=8, Ml=0.25, EfSearch=20, Distance=_metric_fn(H, metric), build_mode=H.BUILD_FLAT)
    g.add_arrays(_keys(len(X)), X)
    return g


# ---------------------------------------------------------------- assignment
@pytest.mark.parametrize("force", [0, 1])
@pytest.mark.parametrize("P", [3, 64, 70])
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_assign_exact_data(H, O, metric, d, P, force):
    """small integers: every f32 summation order gives the exact dot, so the ties are exact"""
    rng = np.random.default_rng(d + P)
    X = rng.integers(-3, 4, (N, d)).astype(np.float32)
    Cn = rng.integers(-3, 4, (P, d)).astype(np.float32)
    Cn[0, :2] = (1, 3)
    Cn[1] = Cn[0]  # a duplicated centroid: the lower index wins
    Cn[2] = Cn[0]
    Cn[2, :2] = (3, 1)
    X[5] = Cn[0]
    X[5, :2] = 2  # equidistant from centroids 0 and 2, under both metrics
    X[3] = 0
    if metric == 0 and P > 3:
        Cn[P - 1] = 0  # a NaN distance: never chosen unless all are
    Q = np.vstack([X[3:6], rng.integers(-3, 4, (B - 3, d)).astype(np.float32)])
    want, D = _order(O, metric, X, Cn)
    assert D[5, 0] == D[5, 2] and (metric == 1 or np.isnan(D[3]).all())
    g = _flat(H, X, metric)
    try:
        g.set_option("part_force_canon", force)
        g.EnablePartitions(P, centroids=Cn)
        assert np.array_equal(g.partition_rows(), want[:, 0])
        wq = _order(O, metric, Q, Cn)[0]
        for m in (1, 3, P):
            assert np.array_equal(g.assign_partitions(Q, m), wq[:, :m]), m
        assert np.array_equal(g.partition_centroids(), Cn) and g.AssignPartition(Q[4]) == wq[4, 0]
        assert g.GetPartitionStats() == np.bincount(want[:, 0], minlength=P).tolist()
    finally:
        g.close()


@pytest.mark.parametrize("cap", [None, 1])  # 1: the worklist overflows, the whole launch is redone canonically
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_assign_rounding_noise(H, O, metric, d, cap):
    P = 70
    rng = np.random.default_rng(11 + d + metric)
    X = rng.uniform(-1, 1, (N, d)).astype(np.float32)
    Cn = rng.normal(size=(P, d)).astype(np.float32)
    near = list(range(10, 29)) + [N - 1]
    o0 = _order(O, metric, X[near], Cn)[0]
    for r, (a, b) in zip(near, o0[:, :2]):  # onto the bisector of the two nearest centroids, in f32
        if metric == 1:
            w, m = Cn[a] - Cn[b], (Cn[a] + Cn[b]) / np.float32(2)
        else:
            w, m = Cn[a] / np.linalg.norm(Cn[a]) - Cn[b] / np.linalg.norm(Cn[b]), np.float32(0)
        X[r] = X[r] - np.float32(np.dot(X[r] - m, w) / np.dot(w, w)) * w
    want, D = _order(O, metric, X, Cn)
    # from the reference alone: some canonical gap between the two nearest is a few ulps at most
    Ds = np.sort(D[near], axis=1)
    assert (Ds[:, 1] - Ds[:, 0] <= 4 * np.spacing(Ds[:, 0])).any()
    g = _flat(H, X, metric)
    try:
        if cap is not None:
            g.set_option("part_worklist_cap", cap)
        g.EnablePartitions(P, centroids=Cn)
        assert np.array_equal(g.partition_rows(), want[:, 0])
        assert g.get_option("last_part_uncertain") > 0
    finally:
        g.close()


# ---------------------------------------------------------------- UpdateCentroids, Rebalance, Train
def _mean(X, parts, Cn):
    out = Cn.copy()
    X64 = X.astype(np.float64)
    for p in np.unique(parts):
        ids = np.flatnonzero(parts == p)
        out[p] = np.float32(X64[ids].sum(0) / len(ids))
    return out


@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_update_rebalance_train(H, O, metric, d):
    """rows on a 2^-10 grid: their f64 sums are exact in any order, so the mean is bit for bit"""
    P = 70
    rng = np.random.default_rng(5 + d)
    X = (rng.integers(-4096, 4096, (N, d)) / 1024.0).astype(np.float32)
    Cn = rng.normal(size=(P, d)).astype(np.float32)
    Cn[P - 1] = Cn[0]  # never the first of a tie: an empty partition, its centroid stays
    g = _flat(H, X, metric)
    try:
        g.EnablePartitions(P, centroids=Cn)
        parts = _order(O, metric, X, Cn)[0][:, 0]
        assert (parts != P - 1).all()
        g.UpdateCentroids()
        Cn = _mean(X, parts, Cn)
        assert np.array_equal(g.partition_centroids().view(np.uint32), Cn.view(np.uint32))
        assert np.array_equal(g.partition_rows(), parts)  # (the rows stay where they were)
        new = _order(O, metric, X, Cn)[0][:, 0]
        assert g.Rebalance() == (new != parts).sum() > 0 and np.array_equal(g.partition_rows(), new)
        parts, moved, its = new, -1, 0
        while its < 5 and moved != 0:
            Cn = _mean(X, parts, Cn)
            new = _order(O, metric, X, Cn)[0][:, 0]
            moved, parts, its = int((new != parts).sum()), new, its + 1
        assert g.TrainPartitions(5) == moved
        assert np.array_equal(g.partition_centroids().view(np.uint32), Cn.view(np.uint32))
        assert np.array_equal(g.partition_rows(), parts) and g.get_option("last_part_train_ns") > 0
    finally:
        g.close()


def test_update_uniform_rows(H, O):
    """P 3 puts more than 256 rows in a partition (several chunks); the f64 accumulation's error
    is far below half an f32 ulp, so only a rounding boundary can cost one ulp"""
    rng = np.random.default_rng(9)
    X = rng.uniform(-1, 1, (N, 100)).astype(np.float32)
    Cn = X[:3].copy()
    g = _flat(H, X, 1)
    try:
        g.EnablePartitions(3, centroids=Cn)
        parts = _order(O, 1, X, Cn)[0][:, 0]
        assert np.bincount(parts).max() > 256
        g.UpdateCentroids()
        got = g.partition_centroids()
        for p in range(3):
            m = X[parts == p].astype(np.float64).mean(0)
            assert (np.abs(got[p] - m) <= np.spacing(np.abs(m).astype(np.float32))).all()
    finally:
        g.close()


# ---------------------------------------------------------------- search against the oracle
def _data(metric, d, n=N):
    """the LSH tests' shape: rows and queries around a common offset, duplicates, a zero row"""
    rng = np.random.default_rng(100 * metric + d)
    X = (rng.uniform(-1, 1, (n, d)) + 0.6).astype(np.float32)
    X[100:110] = X[5]
    X[900 % n] = X[64]
    X[7] = 0
    Q = (rng.uniform(-1, 1, (B, d)) + 0.6).astype(np.float32)
    Q[0], Q[1], Q[2] = X[5], X[64] * 1.5, -0.6
    Q[8:] -= 0.6
    return X, Q


def _check(O, c, Cn, parts, ks=(10,), nprobes=(1, 3)):
    """the stored partitions, then per query the oracle's exact search over the probed ones"""
    dead = c.ex["dead"].astype(bool)
    assert np.array_equal(c.g.partition_rows(), np.where(dead, -1, parts))
    probe = _order(O, c.metric, c.Q, Cn)[0]
    sizes = []
    for m in nprobes:
        masks = (parts[None, :, None] == probe[:, None, :m]).any(2) & ~dead[None]
        sizes += masks.sum(1).tolist()
        refs = [c.ref(masks[q], 256, c.Q[q:q + 1]) for q in range(len(c.Q))]
        for k in ks:  # (the best k of a sorted list are its first k)
            got = c.g.search_partitions_arrays(c.Q, k, m)
            assert np.array_equal(got[3], masks.sum(1)), (m, got[3], masks.sum(1))
            for q, (rk, rd, rn) in enumerate(refs):
                _same(tuple(a[q:q + 1] for a in got[:3]), (rk[:, :k], rd[:, :k], np.minimum(rn, k)))
    return np.array(sizes)


@pytest.fixture(scope="module")
def built(H, O):
    out = {}
    for metric in (0, 1):
        for d in (20, 100):
            X, Q = _data(metric, d)
            out[metric, d] = Case(H, O, _batch_graph(H, metric, X), metric, Q), X[::22][:70].copy()
    yield out
    for c, _ in out.values():
        c.g.close()


@pytest.mark.parametrize("screen", [0, 1])
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_search_against_oracle(H, O, built, metric, d, screen):
    c, Cn = built[metric, d]
    P = len(Cn)
    c.g.set_option("screen", screen)
    c.g.EnablePartitions(P, centroids=Cn)
    parts = _order(O, metric, c.ex["vecs"].reshape(c.n, -1), Cn)[0][:, 0]
    nc = _check(O, c, Cn, parts, ks=(1, 10, 256), nprobes=(1, 3, P))
    assert (nc < 10).any() and (nc > 256).any()  # from the reference masks alone
    _same(c.g.search_partitions_arrays(c.Q, 10, P)[:3], c.g.search_arrays(c.Q, 10, mode=H.MODE_EXACT))
    assert c.g.get_option("last_part_candidates") == B * (~c.ex["dead"].astype(bool)).sum()
    assert c.g.get_option("last_part_rebuild_ns") > 0


def test_mutations(H, O):
    """each step against the reference of the new export; the centroids stay until the last step"""
    n = 700
    X, Q = _data(0, 20, n + 200)
    Cn = X[:n:10].copy()
    g = _batch_graph(H, 0, X[:n])
    try:
        g.EnablePartitions(len(Cn), centroids=Cn)  # on a handle that already holds rows
        c = Case(H, O, g, 0, Q)

        def step():
            c.refresh()
            _check(O, c, Cn, _order(O, 0, c.ex["vecs"].reshape(c.n, -1), Cn)[0][:, 0])

        step()
        assert g.Delete(int(g.search_partitions_arrays(Q[:1], 1)[0][0, 0]))
        step()
        g.add_arrays(_keys(n + 100)[n:], X[n:n + 100])
        step()
        assert g.update_arrays(_keys(n)[[20, 21]], -X[[20, 21]]).all()
        step()
        assert g.Compact() == 1
        step()
        assert c.n == n + 99
        # rows added and still pending when the centroids change belong to the old centroids
        old = g.partition_rows()
        g.add_arrays(_keys(n + 200)[n + 100:], X[n + 100:])
        g.UpdateCentroids()
        c.refresh()
        mine = _order(O, 0, X[n + 100:], Cn)[0][:, 0]
        Cn = _mean(c.ex["vecs"].reshape(c.n, -1), np.concatenate([old, mine]), Cn)
        assert np.array_equal(g.partition_centroids().view(np.uint32), Cn.view(np.uint32))
        assert (mine != _order(O, 0, X[n + 100:], Cn)[0][:, 0]).any()  # (the new centroids would say otherwise)
        _check(O, c, Cn, np.concatenate([old, mine]))
    finally:
        g.close()


# ---------------------------------------------------------------- hosts and errors
def test_partitioner_adapter(H):
    X, Q = _data(1, 20, 300)
    ix = H.Partitioner(4, H.EuclideanDistance, centroids=X[[0, 1, 2, 200]])
    assert ix.Search(Q[0], 3) == ([], []) and ix.Len() == 0 and ix.GetPartition(3) == []
    ix.BatchAdd([f"k{i:03d}" for i in range(300)], list(X))  # string keys
    assert "k200" in ix.GetPartition(3) and "k017" not in ix.GetPartition(3)
    assert ix.AssignVectorToPartition("k017", X[200]) == 3  # replace-on-add: the key moves to row 200's partition
    assert "k017" in ix.GetPartition(3) and ix.Len() == 300 and sum(ix.GetPartitionStats()) == 300
    keys, dist = ix.Search(X[200], 2)
    assert keys == ["k017", "k200"] and dist == [0.0, 0.0]
    ix.RemoveFromPartitions("k200")
    assert "k200" not in ix.GetPartition(3) and sum(ix.GetPartitionStats()) == 299
    ix.UpdateCentroids()
    assert ix.Rebalance() >= 0 and ix.Search(X[200], 2, nprobe=4)[0][0] == "k017"
    ix.Close()


def test_device_entry_on_a_second_stream(H, built):
    import torch

    c, Cn = built[0, 20]
    c.g.EnablePartitions(len(Cn), centroids=Cn)
    k, m = 10, 3
    want = c.g.search_partitions_arrays(c.Q, k, m)
    q = torch.from_numpy(c.Q).cuda()
    ok = torch.full((B * k + 2,), -7, dtype=torch.int64, device="cuda")
    od = torch.full((B * k + 2,), -7.0, dtype=torch.float32, device="cuda")
    on = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    nc = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    c.g.search_partitions_device(q.data_ptr(), B, 20, k, m, ok[1:].data_ptr(), od[1:].data_ptr(), on[1:].data_ptr(),
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
    g = _flat(H, X, 0)
    try:
        with pytest.raises(H.HnswError, match="partition search before mhnsw_part_enable"):
            g.search_partitions_arrays(X[:2], 3)
        with pytest.raises(H.HnswError, match="at most 4096"):
            g.EnablePartitions(4097)
        with pytest.raises(H.HnswError, match="dimension"):
            g.EnablePartitions(4, centroids=np.zeros((4, 21), np.float32))
        g.EnablePartitions(0)  # the default, 10, drawn from the seed
        assert g.get_option("part_count") == 10 and sum(g.GetPartitionStats()) == 40
        with pytest.raises(H.HnswError, match="k <= 256"):
            g.search_partitions_arrays(X[:2], 257)
        for m in (0, 11):
            with pytest.raises(H.HnswError, match="nprobe"):
                g.search_partitions_arrays(X[:2], 3, m)
    finally:
        g.close()


def test_names_are_bound(H):
    lib = H.load()
    for name in ("enable", "assign", "rows", "centroids", "stats", "update_centroids", "rebalance", "train"):
        assert "mhnsw_part_" + name in H.SIGNATURES and hasattr(lib, "mhnsw_part_" + name)
    assert {"mhnsw_search_part", "mhnsw_search_part_device"} <= set(H.SIGNATURES)
