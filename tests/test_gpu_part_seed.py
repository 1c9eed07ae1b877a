"""GPU: the partition scan at part_scan_seed=0 (part_scan.hip k_part_seed_scan, k_ps_pick): keys,
distance bits, n and ncand equal the oracle's masked MODE_EXACT search, the walk and the scan at its
default seed, one probe included; the fallback counter shows that the scan answered."""
import numpy as np
import pytest

from tests.test_gpu_part_scan import _masks, _queries, built  # noqa: F401  (the module's graphs, built again here)
from tests.test_gpu_partitions import Case, _batch_graph, _order, _same

pytestmark = pytest.mark.gpu

B = 102
DEFAULTS = {"part_scan": 0, "part_scan_min_b": 64, "part_scan_room": 1024, "part_scan_seed": 1, "part_scan_seed_room": 4096}


def _scan0(c, k, m, **opt):
    """the search with the scan from one query on at seed 0 (no survivor overflow: 2048 slots >= the rows)"""
    for name, v in {"part_scan": 1, "part_scan_min_b": 1, "part_scan_seed": 0, "part_scan_room": 2048, **opt}.items():
        c.g.set_option(name, v)
    try:
        got = c.g.search_partitions_arrays(c.Q, k, m)
        st = {s: c.g.get_option("last_part_scan_" + s) for s in ("queries", "pairs", "fallback_queries")}
    finally:
        for name, v in DEFAULTS.items():
            c.g.set_option(name, v)
    return got, st


def _check0(O, c, Cn, ks, nprobes, seed_room=4096):
    """seed 0 == oracle == walk == seed 1, and the fallback count within its bounds.  `near`: the live rows of
    the nearest partition; fewer than k: the query walks.  At least k and a list (`length`: live and deleted
    rows, no list is longer) within seed_room: it cannot walk, unless it is a zero query under cosine."""
    out = {}
    parts = _order(O, c.metric, c.ex["vecs"].reshape(c.n, -1), Cn)[0][:, 0]
    length = np.bincount(parts, minlength=len(Cn))[_order(O, c.metric, c.Q, Cn)[0][:, 0]]
    can = ~((c.Q == 0).all(1) & (c.metric == 0))
    for m in nprobes:
        masks, near = _masks(O, c, Cn, m, 1)
        refs = [c.ref(masks[q], 256, c.Q[q:q + 1]) for q in range(B)]
        for k in ks:
            got, st = _scan0(c, k, m, part_scan_seed_room=seed_room)
            walk = c.g.search_partitions_arrays(c.Q, k, m)
            seed1 = _scan0(c, k, m, part_scan_seed=1, part_scan_room=1024)[0]  # (the scan's defaults)
            for other in (walk, seed1):
                _same(got[:3], other[:3])
                assert np.array_equal(got[3], other[3])
            assert np.array_equal(got[3], masks.sum(1))
            for q, (rk, rd, rn) in enumerate(refs):
                _same(tuple(a[q:q + 1] for a in got[:3]), (rk[:, :k], rd[:, :k], np.minimum(rn, k)))
            fb = st["fallback_queries"]
            assert st["queries"] == B
            assert ((near < k) | (near > seed_room)).sum() <= fb <= B - ((near >= k) & can & (length <= seed_room)).sum()
            assert st["pairs"] >= k * (B - fb)  # (the picked rows come back as survivors)
            out[m, k] = fb
    return out


@pytest.mark.parametrize("P", [3, 70])
@pytest.mark.parametrize("d", [20, 100])
@pytest.mark.parametrize("metric", [0, 1])
def test_parity_with_the_oracle(H, O, built, metric, d, P):
    c, Cn = built[metric, d]
    c.g.EnablePartitions(P, centroids=Cn[:P])
    fb = _check0(O, c, Cn[:P], ks=(1, 10, 256), nprobes=(1, 2, 3, P))
    if P == 3:
        assert fb[1, 10] == 0  # one probe, every nearest partition holds k rows: the scan answered them all


@pytest.mark.parametrize("metric", [0, 1])
def test_ties_at_the_cut(H, O, metric):
    """65 equal rows under query 3: k = 10 cuts inside equal scores (not exactly k taken: no radius, a fallback)"""
    X, Q = _queries(metric, 20, 700)
    X[300:364] = X[11]
    Q[3] = X[11]
    Cn = X[[11, 400, 500]].copy()
    g = _batch_graph(H, metric, X)
    try:
        g.EnablePartitions(3, centroids=Cn)
        fb = _check0(O, Case(H, O, g, metric, Q), Cn, ks=(10, 70), nprobes=(1, 2))
        assert fb[1, 10] == 0 and fb[2, 10] == 0
    finally:
        g.close()


@pytest.mark.parametrize("seed_room,fallbacks", [(16, [B]), (600, range(1, B))])
def test_seed_room(H, O, built, seed_room, fallbacks):
    c, Cn = built[1, 100]
    c.g.EnablePartitions(3, centroids=Cn[:3])
    fb = _check0(O, c, Cn[:3], ks=(10,), nprobes=(1, 3), seed_room=seed_room)
    assert fb[1, 10] in fallbacks and fb[3, 10] in fallbacks


def test_delete_then_add(H, O):
    """Deletes that leave a nearest partition below k live rows (no list rebuild), then an Add"""
    n, k = 700, 10
    X, Q = _queries(1, 20, n + 100)
    Cn = X[:n:50].copy()
    g = _batch_graph(H, 1, X[:n])
    try:
        g.EnablePartitions(len(Cn), centroids=Cn)
        c = Case(H, O, g, 1, Q)
        before = _check0(O, c, Cn, ks=(k,), nprobes=(1, 3))
        parts = _order(O, 1, X[:n], Cn)[0][:, 0]
        p = _order(O, 1, Q, Cn)[0][0, 0]  # query 0's nearest partition: all but 5 of its rows go
        for row in np.flatnonzero(parts == p)[5:].tolist():
            assert g.Delete(row * 3 + 1)
        c.refresh()
        after = _check0(O, c, Cn, ks=(k,), nprobes=(1, 3))
        assert after[1, k] > before[1, k] and after[3, k] > before[3, k]
        g.add_arrays(np.arange(n, n + 100, dtype=np.int64) * 3 + 1, X[n:])
        c.refresh()
        _check0(O, c, Cn, ks=(k,), nprobes=(1, 3))
    finally:
        g.close()


def test_device_entry_on_a_second_stream(H, built):
    import torch

    c, Cn = built[0, 20]
    c.g.EnablePartitions(len(Cn), centroids=Cn)
    k, m = 10, 1
    want = c.g.search_partitions_arrays(c.Q, k, m)
    outs = [torch.full((B * k + 2,), -7, dtype=t, device="cuda") for t in (torch.int64, torch.float32)]
    outs += [torch.full((B + 2,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    q = torch.from_numpy(c.Q).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for name, v in (("part_scan", 1), ("part_scan_min_b", 1), ("part_scan_seed", 0)):
        c.g.set_option(name, v)
    try:
        c.g.search_partitions_device(q.data_ptr(), B, 20, k, m, *(t[1:].data_ptr() for t in outs), stream=s.cuda_stream)
        s.synchronize()
        c.g.device_status()
        assert c.g.get_option("last_part_scan_queries") == B
        assert c.g.get_option("last_part_scan_fallback_queries") < B
    finally:
        for name, v in DEFAULTS.items():
            c.g.set_option(name, v)
    for t in outs:  # guard words
        assert t[0].item() == -7 and t[-1].item() == -7
    ok, od, on, nc = (t[1:-1].cpu().numpy() for t in outs)
    _same((ok.reshape(B, k), od.reshape(B, k), on), want[:3])
    assert np.array_equal(nc, want[3])


def test_refusals_and_defaults(H, built):
    c, Cn = built[0, 20]
    c.g.EnablePartitions(len(Cn), centroids=Cn)
    with pytest.raises(H.HnswError, match="part_scan_seed_room"):
        c.g.set_option("part_scan_seed_room", 0)
    with pytest.raises(H.HnswError, match="part_scan_seed"):
        c.g.set_option("part_scan_seed", -1)
    assert _scan0(c, 10, 1)[1]["queries"] == B
    assert {name: c.g.get_option(name) for name in DEFAULTS} == DEFAULTS
