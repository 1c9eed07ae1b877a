"""GPU: the partition-major scan (part_scan.hip; option part_scan) -- mhnsw_search_part* answered by
k_part_scan instead of the one-wave walk.  Keys, distance bits, n and ncand equal the oracle's
MODE_EXACT search with every row outside the probed partitions in the dead flags
(tests/test_gpu_partitions.py _check's reference), and the same call with part_scan=0.

102 queries: at P = 3 a partition is probed by more than one 64-query tile; 1531 rows: row tiles
with a tail, and at P = 70 partitions smaller than a row tile and than k.
"""
import numpy as np
import pytest

from tests.test_gpu_partitions import B as B0, Case, _batch_graph, _data, _order, _same

pytestmark = pytest.mark.gpu

B = 32 + 70


def _queries(metric, d, n=1531):
    X, Q = _data(metric, d, n)
    rng = np.random.default_rng(7 + d)
    return X, np.vstack([Q, (rng.uniform(-1, 1, (B - B0, d)) + 0.6).astype(np.float32)])


@pytest.fixture(scope="module")
def built(H, O):
    out = {}
    for metric in (0, 1):
        for d in (20, 100):
            X, Q = _queries(metric, d)
            out[metric, d] = Case(H, O, _batch_graph(H, metric, X), metric, Q), X[::22][:70].copy()
    yield out
    for c, _ in out.values():
        c.g.close()


def _scan(c, k, m, **opt):
    """the search with part_scan=1 from one query on; the options back at their defaults after it"""
    for name, v in {"part_scan": 1, "part_scan_min_b": 1, **opt}.items():
        c.g.set_option(name, v)
    try:
        got = c.g.search_partitions_arrays(c.Q, k, m)
        stats = {s: c.g.get_option("last_part_scan_" + s) for s in ("queries", "pairs", "fallback_queries")}
    finally:
        for name, v in (("part_scan", 0), ("part_scan_min_b", 64), ("part_scan_room", 1024), ("part_scan_seed", 1)):
            c.g.set_option(name, v)
    return got, stats


def _masks(O, c, Cn, m, seed=1):
    """per query the live rows of its m nearest partitions, and how many its `seed` nearest hold"""
    dead = c.ex["dead"].astype(bool)
    parts = _order(O, c.metric, c.ex["vecs"].reshape(c.n, -1), Cn)[0][:, 0]
    probe = _order(O, c.metric, c.Q, Cn)[0]
    near = (parts[None, :, None] == probe[:, None, :seed]).any(2) & ~dead[None]
    return (parts[None, :, None] == probe[:, None, :m]).any(2) & ~dead[None], near.sum(1)


def _check(O, c, Cn, ks, nprobes, **opt):
    """scan == oracle == walk; returns the scan's counters per (nprobe, k)"""
    out = {}
    for m in nprobes:
        masks, near = _masks(O, c, Cn, m, min(opt.get("part_scan_seed", 1), m - 1))
        refs = [c.ref(masks[q], 256, c.Q[q:q + 1]) for q in range(len(c.Q))]
        for k in ks:
            got, st = _scan(c, k, m, **opt)
            walk = c.g.search_partitions_arrays(c.Q, k, m)
            assert c.g.get_option("last_part_scan_queries") == 0
            _same(got[:3], walk[:3])
            assert np.array_equal(got[3], masks.sum(1)) and np.array_equal(walk[3], got[3])
            for q, (rk, rd, rn) in enumerate(refs):
                _same(tuple(a[q:q + 1] for a in got[:3]), (rk[:, :k], rd[:, :k], np.minimum(rn, k)))
            # a silent fall-through to the walk fails here.  From the masks alone: a query whose
            # nearest partition holds fewer than k live rows has no full seed list and walks; one
            # with a full seed list whose other probed rows fit the survivor slots cannot overflow.
            sure = (near >= k) & (masks.sum(1) - near <= opt.get("part_scan_room", 1024))
            assert st["queries"] == B
            assert (near < k).sum() <= st["fallback_queries"] <= B - sure.sum()
            out[m, k] = st, near
    assert sum(st["pairs"] for st, _ in out.values()) > 0
    return out


@pytest.mark.parametrize("P", [3, 70])
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_parity_with_the_oracle(H, O, built, metric, d, P):
    c, Cn = built[metric, d]
    Cn = Cn[:P]
    c.g.EnablePartitions(P, centroids=Cn)
    res = _check(O, c, Cn, ks=(1, 10, 256), nprobes=(2, 3, P))
    if P == 70:  # short seed, from the reference masks alone: nearest partitions below 256 rows
        st, near = res[3, 256]
        assert st["fallback_queries"] >= (near < 256).sum() > 0
    # nprobe = P is the exact search
    _same(_scan(c, 10, P)[0][:3], c.g.search_arrays(c.Q, 10, mode=H.MODE_EXACT))


@pytest.mark.parametrize("screen", [0, 1])
def test_overflow_and_seed_width(H, O, built, screen):
    """one survivor slot: the queries with more walk instead, never from a partial list"""
    c, Cn = built[0, 100]
    c.g.set_option("screen", screen)
    c.g.EnablePartitions(len(Cn), centroids=Cn)
    res = _check(O, c, Cn, ks=(1, 10), nprobes=(8,), part_scan_room=1)
    for k in (1, 10):
        assert res[8, k][0]["fallback_queries"] > (res[8, k][1] < k).sum()
    _check(O, c, Cn, ks=(10,), nprobes=(8,), part_scan_seed=2)
    c.g.set_option("screen", 1)


def test_mutation(H, O):
    """a Delete in a probed partition (no list rebuild: the epilogue drops the row), then an Add"""
    n = 700
    X, Q = _queries(1, 20, n + 100)
    Cn = X[:n:100].copy()
    g = _batch_graph(H, 1, X[:n])
    try:
        g.EnablePartitions(len(Cn), centroids=Cn)
        c = Case(H, O, g, 1, Q)
        _check(O, c, Cn, ks=(10,), nprobes=(3,))
        hit = _scan(c, 5, 3)[0][0]
        for key in hit[0, :3].tolist():
            assert g.Delete(int(key))
        c.refresh()
        _check(O, c, Cn, ks=(10,), nprobes=(3,))
        g.add_arrays(np.arange(n, n + 100, dtype=np.int64) * 3 + 1, X[n:])
        c.refresh()
        _check(O, c, Cn, ks=(10,), nprobes=(3,))
    finally:
        g.close()


def test_device_entry_on_a_second_stream(H, built):
    import torch

    c, Cn = built[1, 20]
    c.g.EnablePartitions(len(Cn), centroids=Cn)
    k, m = 10, 3
    want, _ = _scan(c, k, m)
    q = torch.from_numpy(c.Q).cuda()
    ok = torch.full((B * k + 2,), -7, dtype=torch.int64, device="cuda")
    od = torch.full((B * k + 2,), -7.0, dtype=torch.float32, device="cuda")
    on = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    nc = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    c.g.set_option("part_scan", 1)
    c.g.set_option("part_scan_min_b", 1)
    try:
        c.g.search_partitions_device(q.data_ptr(), B, 20, k, m, ok[1:].data_ptr(), od[1:].data_ptr(), on[1:].data_ptr(),
                                     nc[1:].data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        c.g.device_status()
        assert c.g.get_option("last_part_scan_queries") == B
    finally:
        c.g.set_option("part_scan", 0)
        c.g.set_option("part_scan_min_b", 64)
    for t in (ok, od, on, nc):  # guard words
        assert t[0].item() == -7 and t[-1].item() == -7
    got = (ok[1:-1].cpu().numpy().reshape(B, k), od[1:-1].cpu().numpy().reshape(B, k), on[1:-1].cpu().numpy())
    _same(got, want[:3])
    assert np.array_equal(nc[1:-1].cpu().numpy(), want[3])


def test_refusals(H, built):
    c, Cn = built[0, 20]
    c.g.EnablePartitions(len(Cn), centroids=Cn)
    with pytest.raises(H.HnswError, match="part_scan must be 0 or 1"):
        c.g.set_option("part_scan", 2)
    with pytest.raises(H.HnswError, match="part_scan_room"):
        c.g.set_option("part_scan_room", 0)
    assert c.g.get_option("part_scan") == 0 and c.g.get_option("part_scan_min_b") == 64
    assert _scan(c, 10, 1)[1]["queries"] == 0  # one probe: the walk
    assert _scan(c, 10, 3, part_scan_min_b=B + 1)[1]["queries"] == 0  # a batch below the minimum
