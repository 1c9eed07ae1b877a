"""CPU: the restatement of the batched insert, link pass and update (oracle.c og_add_batch /
og_update) on its own.

1. Exhaustive regime, against ~40 lines of numpy that share nothing with the C: with
   n <= 60 rows, ef >= n and one-row batches, an insert's candidate list is every row reachable
   from its entry, so the expected graph after each insert follows from the written rules alone
   (ranking by (distance, id), the diversity rule with alpha, the keep-pruned fill, the
   commit's overflow rule).
2. Properties of every case of tests/batch_ref.py's table, which test_gpu_batch_oracle.py
   compares with the engine: structure, stored distances canonical both ways round, and the
   ascending and descending runs give the identical export.
3. Conditions the GPU comparison relies on (not measurements): no case would have dropped a
   proposal, and every counter a case claims to reach is above 0.
4. tests/golden/batch_build.npz, an engine-built graph recorded on an MI355X by
   test_gpu_batch_oracle.record_golden: the restatement reproduces it without a GPU.
"""
import os

import numpy as np
import pytest

from tests import batch_ref as BR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_build.npz")


# ---- 1: the exhaustive regime ------------------------------------------------------------------

def _rule(cand, D, mcap, alpha, rule, fill):
    """cand: [(d, id)] ranked; D: canonical distances between rows; alpha float32"""
    sel = []
    for d, c in cand:
        if len(sel) == mcap:
            break
        if rule and any(alpha * D[c, r] < d for _, r in sel):
            continue
        sel.append((d, c))
    for d, c in cand if fill else ():
        if len(sel) < mcap and (d, c) not in sel:
            sel.append((d, c))
    return sel


def _expected_insert(rows, entry, u, lv, D, caps, h, kp, alpha):
    """rows[l]: {id: [(d, id)]} of the members; entry[l]; the graph after row u (level lv) is
    inserted alone, by the contract: per layer from the top, a greedy step above lv, else every
    row reachable from the running entry ranked by (distance to u, id), u's selection, and the
    commit of u into each selected row."""
    top = max(l for l in range(len(rows)) if rows[l])
    cur = entry[top]
    for l in range(top, -1, -1):
        if l > lv:  # ef 1: the closest of the current row and its neighbours, until that is the row
            while True:
                best = min([(D[u, cur], cur)] + [(D[u, v], v) for _, v in rows[l][cur]])
                if best[1] == cur:
                    break
                cur = best[1]
            continue
        reach, todo = {cur}, [cur]
        while todo:
            for _, v in rows[l][todo.pop()]:
                if v not in reach:
                    reach.add(v)
                    todo.append(v)
        cand = sorted((D[u, v], v) for v in reach)
        cur = cand[0][1]
        sel = _rule(cand, D, caps[l], alpha, h > 0, kp)
        for d, v in sel:
            ents = sorted(rows[l][v] + [(d, u)])
            rows[l][v] = ents[:caps[l]] if len(ents) <= caps[l] or h < 2 else _rule(ents, D, caps[l], alpha, True, False)
        rows[l][u] = sel
    for l in range(top + 1, lv + 1):
        rows[l][u] = []
        entry[l] = u


@pytest.mark.parametrize("alpha_pct", [100, 130])
@pytest.mark.parametrize("kp", [0, 1])
@pytest.mark.parametrize("h", [0, 2])
@pytest.mark.parametrize("metric", [0, 1])
def test_exhaustive_regime(O, metric, h, kp, alpha_pct):
    n, d, M, m0 = 60, 8, 4, 6  # small caps: rows overflow, the rule and the fill both act
    rng = np.random.default_rng(7 + metric)
    X = BR.clustered(rng, n, d, nc=4, intrinsic=3)
    X[7] = X[3]  # a duplicate: equal distances, order by id
    keys = BR.keys_of(n)
    g = O.Graph(metric=metric, order=O.ORDER_DEV, M=M, M0=m0, Ml=0.25, EfSearch=64, seed=BR.RNG_SEED)
    levels = g.preview_levels(n)
    levels[20] = levels.max() + 1  # a row above the top, well after the first
    ia, ib = np.divmod(np.arange(n * n), n)
    D = O.distance_pairs(metric, O.ORDER_DEV, X, ia, ib).reshape(n, n)
    assert np.array_equal(D.view(np.uint32), D.T.view(np.uint32))  # canonical both ways round
    alpha = np.float32(alpha_pct) / np.float32(100)
    L = int(levels.max()) + 1
    caps = [m0] + [M] * (L - 1)
    rows, entry = [dict() for _ in range(L)], [-1] * L
    total = {}
    for u in range(n):
        cn = g.add_batch(keys[u:u + 1], X[u:u + 1], levels[u:u + 1], ef_construction=64, heuristic=h, keep_pruned=kp,
                         prune_alpha_pct=alpha_pct, batch_max=1)
        for k, v in cn.items():
            total[k] = total.get(k, 0) + v
        if u == 0:
            for l in range(levels[0] + 1):
                rows[l][0], entry[l] = [], 0
        else:
            _expected_insert(rows, entry, u, int(levels[u]), D, caps, h, kp, alpha)
        ex, ed = g.export(), g.export_edge_dist()
        assert ex["entry"].tolist() == entry[:len(ex["entry"])] and all(e == -1 for e in entry[len(ex["entry"]):])
        for l in range(ex["deg"].shape[0]):
            for v in range(u + 1):
                want = rows[l].get(v)
                got_deg = int(ex["deg"][l, v])
                assert (got_deg == -2) == (want is None), (u, l, v)
                if want is None:
                    continue
                got = list(zip(ed[l, v, :got_deg].tolist(), ex["adj"][l, v, :got_deg].tolist()))
                assert got == [(float(dd), int(c)) for dd, c in want], (u, l, v)
    assert total["dropped_proposals"] == 0
    assert total["overflow_commits" if h == 2 else "truncated_commits"] > 0
    if h:
        assert total["rule_drops"] > 0 and (total["fills"] > 0) == bool(kp)


# ---- 2 and 3: every case of the table ----------------------------------------------------------

def check_structure(O, metric, ex, ed, caps):
    """deg <= cap, no duplicate, no self-loop, members only, no live -> deleted edge; every stored
    distance is the canonical distance of the two rows, both ways round, bit for bit"""
    L, N = ex["deg"].shape
    dead = ex["dead"].astype(bool)
    for l in range(L):
        deg = np.maximum(ex["deg"][l], 0)
        assert (deg <= caps[l]).all(), l
        slot = np.arange(ex["adj"].shape[2])[None, :] < deg[:, None]
        assert (ex["adj"][l][~slot] == -1).all() and not ed[l][~slot].any(), l
        src, _ = np.nonzero(slot)
        dst = ex["adj"][l][slot]
        assert dst.min(initial=0) >= 0 and dst.max(initial=0) < N, l
        assert (src != dst).all(), l
        assert (ex["deg"][l][dst] >= 0).all(), l           # members of the layer only
        assert not (dead[dst] & ~dead[src]).any(), l      # no live -> deleted edge
        pair = src.astype(np.int64) * N + dst
        assert len(np.unique(pair)) == len(pair), l        # set-valued rows
        got = ed[l][slot]
        for a, b in ((src, dst), (dst, src)):
            want = O.distance_pairs(metric, O.ORDER_DEV, ex["vecs"], a, b)
            assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), l


@pytest.mark.parametrize("name,metric", BR.case_ids())
def test_case(O, name, metric):
    """3, the conditions the GPU comparison relies on: no proposal would have been dropped, and
    every counter the case claims to reach is above 0.  2: structure and stored distances after
    every step, and the ascending and the descending run give the identical export."""
    case, sh = BR.CASES[name], BR.CASES[name]["shape"]
    asc = BR.run_oracle(O, case, metric, keep=True)
    print(name, metric, asc.counters)
    assert asc.counters["dropped_proposals"] == 0
    for r in case["reach"]:
        assert asc.counters[r] > 0, r
    assert asc.g.topography()[0] >= 0.9 * sh["n"] and len(asc.g.topography()) >= 3
    desc = BR.run_oracle(O, case, metric, keep=True, descending=True)
    assert len(asc.snaps) == len(case["script"]) == len(desc.snaps)
    for (step, ex, ed), (_, ex2, ed2) in zip(asc.snaps, desc.snaps):
        check_structure(O, metric, ex, ed, [sh["m0"]] + [sh["M"]] * 31)
        BR.same_export(ex, ex2, ed, ed2, what=(name, metric, step))
    assert asc.counters == desc.counters


def test_update_found_and_chunks(O):
    """og_update's own bookkeeping: an absent and a deleted key are not found, the rows keep ids,
    levels and entries, and a repeated key is refused with the graph untouched"""
    case = BR.CASES["update-scenario"]
    drv = BR.run_oracle(O, case, 0, keep=True)
    (_, ex0, _), (_, ex1, _) = drv.snaps[-2:]
    assert (~drv.found).sum() == 2 and drv.counters["update_chunks"] >= 2
    for f in ("keys", "dead", "entry"):
        assert np.array_equal(ex0[f], ex1[f]), f
    assert np.array_equal(ex0["deg"] == -2, ex1["deg"] == -2)
    changed = np.flatnonzero((ex0["vecs"] != ex1["vecs"]).any(axis=1))
    assert len(changed) == int(drv.found.sum())
    # the detach reached its second rule: deleted rows held edges into the chunks and lost them,
    # in place and in order
    lost = 0
    for l in range(ex0["deg"].shape[0]):
        for r in np.flatnonzero((ex0["dead"] != 0) & (ex0["deg"][l] > 0)):
            old = ex0["adj"][l, r, : ex0["deg"][l, r]]
            keep = old[~np.isin(old, changed)]
            lost += len(old) - len(keep)
            assert ex1["adj"][l, r, : ex1["deg"][l, r]].tolist() == keep.tolist(), (l, r)
    assert lost > 0
    k = ex1["keys"][changed[:2]]
    with pytest.raises(O.OracleError, match="duplicate key"):
        drv.g.update(np.array([k[0], k[1], k[0]]), ex1["vecs"][:3], **drv.opts)
    BR.same_export(drv.g.export(), ex1, drv.g.export_edge_dist(), drv.snaps[-1][2])
    with pytest.raises(O.OracleError, match="duplicate key"):
        drv.g.add_batch(k[:1], ex1["vecs"][:1], [0], **drv.opts)


# ---- 4: the engine-built fixture ---------------------------------------------------------------

def test_golden_replay(O):
    """The engine's graph after each call of BR.GOLDEN (two Adds, a delete, a link batch and an
    update of n 300, d 16, cosine; recorded on an MI355X, see the module docstring): the
    restatement, given the recorded levels, gives every export and every edge distance bit for
    bit, and the fixture reaches what it is there for."""
    levels, snaps = BR.unpack_golden(np.load(GOLDEN))
    drv = BR.run_oracle(O, BR.GOLDEN, BR.GOLDEN_METRIC, levels=levels, keep=True)
    assert drv.counters["dropped_proposals"] == 0
    for r in BR.GOLDEN["reach"]:
        assert drv.counters[r] > 0, r
    assert len(drv.snaps) == len(snaps) == len(BR.GOLDEN["script"])
    for (step, ex, ed), (wx, wd) in zip(drv.snaps, snaps):
        BR.same_export(wx, ex, wd, ed, what=step)
