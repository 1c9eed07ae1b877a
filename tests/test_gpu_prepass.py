"""GPU: the ordered beam search's descent pre-pass (beam.hpp k_beam_descend) in
its own shape: its own rows in flight and waves per SIMD (beam_desc_group /
beam_desc_waves), its own small visited set up to upper_ef 4 (beam_desc_vis),
and its counters summed by k_beam_descend_stats instead of added per wave.

None of that may show in a result.  On 768-dimensional graphs (Cfg<64, 3>, the
headline's instantiation of the kernel) the ordered path must return the fused
launch's lists bit for bit, with the same five counters, and the oracle's
MODE_BEAM lists: over both metrics, the screen on and off, graphs with many
thin upper layers, before and after deletes that empty them, every upper_ef on
both sides of the small set's rule, and visited sets the user sized.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import _clustered, _metric_fn
from tests.test_gpu_query_order import _check, _search, _identical, _with

pytestmark = pytest.mark.gpu

D = 768
NQ = 600
B = 513


def _graph(H, O, metric, n, seed, levels=None):
    rng = np.random.default_rng(seed)
    X = _clustered(rng, n, D, intrinsic=24)
    Q = _clustered(rng, NQ, D, intrinsic=24)
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=5, build_mode=H.BUILD_BATCH,
                ef_construction=64, heuristic=2, m0=32)
    g.add_arrays(np.arange(n) * 3 + 1, X, levels=levels)
    g.set_option("search_order_min_b", 1)
    g.set_option("beam_mw_max_b", 0)
    return g, Q


def _mirror(O, g, metric):
    o = O.Graph(metric=metric, order=O.ORDER_DEV, M=16, M0=32, Ml=0.25, EfSearch=64)
    o.import_graph(**g.export())
    return o


@pytest.fixture(scope="module")
def built(H, O):
    """one batched 768-d graph per metric, mirrored into the oracle, and the oracle's lists at ef 10 and 64"""
    out = {}
    for metric in (0, 1):
        g, Q = _graph(H, O, metric, 3500, 211 + metric)
        o = _mirror(O, g, metric)
        ref = {ef: o.search(Q[:B], 10, mode=O.MODE_BEAM, ef=ef) for ef in (10, 64)}
        out[metric] = (g, Q, ref)
    yield out
    for g, _, _ in out.values():
        g.close()


def _tall_levels(n):
    """nine layers on n rows: 1, 2, 4, 8, 16 nodes in layers 8 .. 4, then 48, 190 and 750"""
    lv = np.zeros(n, np.int32)
    at = 0
    for level, count in ((8, 1), (7, 1), (6, 2), (5, 4), (4, 8), (3, 32), (2, 142), (1, 560)):
        lv[at : at + count] = level
        at += count
    return np.random.default_rng(9).permutation(lv)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("ef", [10, 64])
def test_ordered_matches_fused_and_oracle(H, O, built, metric, ef):
    """Case 1: B = 513, screen on and off; and the same with the whole descent
    above layer 1 in the pre-pass (a one-layer key from layer 1)"""
    import torch

    g, Q, ref = built[metric]
    try:
        for screen in (1, 0):
            _with(g, screen=screen)
            _check(torch, g, Q[:B], 10, ef, ref[ef])
            old = _with(g, search_order_top=1, search_order_fields=1)
            try:
                _check(torch, g, Q[:B], 10, ef, ref[ef])
            finally:
                _with(g, **old)
    finally:
        _with(g, screen=1)


@pytest.mark.parametrize("metric", [0, 1])
def test_many_thin_layers_and_restart(H, O, metric):
    """Case 2: nine layers on 3,000 rows, so the pre-pass walks many layers; then
    the top entry and every row of layers 5 and above deleted, among others, so
    the descent starts on a row that is in no layer and restarts at each layer's
    entry (deg == -2), or skips a layer that has none"""
    import torch

    n = 3000
    lv = _tall_levels(n)
    g, Q = _graph(H, O, metric, n, 223 + metric, levels=lv)
    ex = g.export()
    assert ex["deg"].shape[0] >= 8
    assert [int((ex["deg"][l] != -2).sum()) for l in (8, 7, 6, 5, 4)] == [1, 2, 4, 8, 16]
    o = _mirror(O, g, metric)
    for ef in (10, 64):
        ref = o.search(Q[:B], 10, mode=O.MODE_BEAM, ef=ef)
        for screen in (1, 0):
            _with(g, screen=screen)
            _check(torch, g, Q[:B], 10, ef, ref)
    gone = sorted({int(ex["entry"][-1])} | set(np.flatnonzero(lv >= 5).tolist()) | set(range(0, n, 17)))
    g.BatchDelete([3 * i + 1 for i in gone])
    o = _mirror(O, g, metric)
    keys_gone = {3 * i + 1 for i in gone}
    for ef in (10, 64):
        ref = o.search(Q[:B], 10, mode=O.MODE_BEAM, ef=ef)
        for screen in (1, 0):
            _with(g, screen=screen)
            r = _check(torch, g, Q[:B], 10, ef, ref)
            assert not (set(r[0][r[0] >= 0].tolist()) & keys_gone)
    g.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("upper_ef", [1, 4, 64])
def test_upper_ef_both_sides_of_the_rule(H, O, built, metric, upper_ef):
    """Case 3: upper_ef 1 and 4 walk with the pre-pass's small visited set, 64
    with the launch's own; ordered equals fused in lists and counters"""
    import torch

    g, Q, ref = built[metric]
    old = _with(g, upper_ef=upper_ef)
    try:
        for top, fields in ((0, 0), (1, 1)):
            _with(g, search_order_top=top, search_order_fields=fields)
            _check(torch, g, Q[:B], 10, 64, ref[64] if upper_ef == 1 else None)
    finally:
        _with(g, search_order_top=0, search_order_fields=0, **old)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("vis_entries", [64, 32768])
def test_user_sized_visited_set(H, O, built, metric, vis_entries):
    """Case 4: a set smaller than the pre-pass's own (kept as given: the fused
    and the ordered walks forget alike) and the largest one; the lists are the
    default's"""
    import torch

    g, Q, ref = built[metric]
    Qd = torch.tensor(Q[:B], device="cuda")
    order = g.get_option("search_order")
    try:
        want, _ = _search(torch, g, Qd, 10, 64, 1)
        g.set_option("vis_entries", vis_entries)
        got = _check(torch, g, Q[:B], 10, 64, ref[64])
    finally:
        g.set_option("vis_entries", 0)
        g.set_option("search_order", order)
    _identical(got, want)
