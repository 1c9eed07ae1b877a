"""CPU: the staircase graphs of tests/staircase.py are the case they claim to be.

The GPU tests (test_gpu_merge_steps.py) compare the engine with the oracle on
these graphs; that says something about bl_merge only if the search really
reaches a step that flushes twice with a later buffer that is wholly worse than
the list the first flush left.  Checked here, without a GPU, from a plain
restatement of the step batching (staircase.restate: bl_insert semantics, no
bl_merge) and the oracle's whole list.
"""
import numpy as np
import pytest

from tests import staircase as sc

CASES = [(ef, xw, metric, width, bad, origin)
         for ef in (256, 300, 512) for xw in (1, 2, 4) for metric in (0, 1) for width in (64, 63)
         for bad, origin in ((0, 0.0), (5, 0.0), (0, 16.0)) if not (metric == 0 and origin)]


@pytest.mark.parametrize("ef,xw,metric,width,bad,origin", CASES)
def test_staircase_is_the_case(O, ef, xw, metric, width, bad, origin):
    s = sc.staircase(ef, xw, metric, width=width, bad=bad, origin=origin)
    g, q, info = s["graph"], s["query"], s["info"]
    n = len(g["keys"])
    assert 300 <= n <= 1500
    dist = np.array([O.distance(metric, O.ORDER_DEV, q, g["vecs"][i]) for i in range(n)], np.float32)
    fin = np.array([i not in set(info["bad"]) for i in range(n)])
    # distinct, finite distances (bl_merge's fast path); the bad rows are not finite
    assert np.isfinite(dist[fin]).all()
    assert len(set(dist[fin].tolist())) == int(fin.sum())
    assert len(info["bad"]) == (bad * xw) and not np.isfinite(dist[~fin]).any()
    if bad:
        assert (np.isnan(dist[~fin]) if metric == 0 else np.isposinf(dist[~fin])).all()
    if metric == 1:
        assert all(dist[i] == info["pos"][i] for i in range(n) if fin[i])  # exactly p
    # the bait: better than every row, adjacent only to G2's best row
    assert dist[info["Z"]] == dist[fin].min()
    holders = [i for i in range(n) if info["Z"] in g["adj"][0, i, : g["deg"][0, i]].tolist()]
    assert holders == [info["g2_best"]]
    assert dist[info["g2_best"]] == dist[info["G2"]].min()

    lst, nx, steps = sc.restate(g, dist, ef, xw)
    (crit,) = [t for t in steps if info["P"][0] in t["cur"]]
    assert crit["full_before"] and np.isfinite(crit["worst_before"])
    # no bad row arrives once the list is full
    for t in steps:
        if t["full_before"]:
            assert not (set(info["bad"]) & {v for f in t["flushes"] for v in f["ids"]})
    if bad:
        assert any(set(info["bad"]) & {v for f in t["flushes"] for v in f["ids"]} for t in steps) == (metric == 1)
    if xw >= 2:
        assert crit["cur"][:2] == info["P"]
        assert len(crit["flushes"]) >= 2
        assert set(crit["flushes"][0]["ids"]) == set(info["G1"])
        later = [v for f in crit["flushes"][1:] for v in f["ids"]]
        assert set(later) == set(info["G2"])
        post = crit["flushes"][0]["worst_after"]
        assert post < crit["worst_before"]
        assert all(post < dist[v] < crit["worst_before"] for v in later)
    else:
        assert all(len(t["flushes"]) <= 1 for t in steps)  # the control: one batch per step
    # the right list: never a G2 row, never the bait
    ids = [e[1] for e in lst]
    assert len(ids) == ef and not (set(ids) & (set(info["G2"]) | {info["Z"]}))

    o = sc.oracle_graph(O, s)
    rk, rd, rn, ox = sc.oracle_list(O, o, s)
    assert rn[0] == ef and ox == nx
    assert rk[0].tolist() == g["keys"][ids].tolist()
    assert np.array_equal(rd[0].view(np.uint32), np.array([e[0] for e in lst], np.float32).view(np.uint32))
    assert int(g["keys"][info["Z"]]) not in rk[0].tolist()


def test_staircase_shape_of_the_first_instance():
    """ef 256, XW 4, Euclidean, width 64: E -> 64 A rows, A_0..A_3 -> 48 rows
    each, the first two of those -> G1 / G2"""
    info = sc.staircase(256, 4, 1)["info"]
    pos = info["pos"]
    assert [len(l) for l in info["levels"]] == [64, 192]
    assert sorted(pos[v] for v in info["levels"][1]) == list(range(500, 692))
    assert sorted(pos[v] for v in info["G1"]) == list(range(100, 164))
    assert sorted(pos[v] for v in info["G2"]) == list(range(800, 864))
    assert sorted(pos[v] for v in info["A"]) == list(range(900, 964))
    assert pos[info["E"]] == 1000 and pos[info["Z"]] == 1


def test_same_rows_do_not_fill_at_another_xw():
    """the fill steps depend on XW: the XW-4 rows searched at XW 2 reach P_0
    before the list is full, so every XW needs its own graph"""
    s = sc.staircase(256, 4, 1)
    g, info = s["graph"], s["info"]
    dist = np.array([info["pos"][i] for i in range(len(g["keys"]))], np.float32)
    _, _, steps = sc.restate(g, dist, 256, 2)
    (crit,) = [t for t in steps if info["P"][0] in t["cur"]]
    assert not crit["full_before"]
