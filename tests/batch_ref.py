"""The batched insert's named cases, shared by test_batch_oracle.py (CPU: the restatement's own
conditions and properties) and test_gpu_batch_oracle.py (GPU: engine == restatement, bit for
bit).  Plain Python: generators, one table, and the walk that turns a case into calls on a
driver -- OracleDriver here, the engine's in the GPU test.

A case: shape (d, n, M, m0), build options under the engine's names, the data generator, the
call sequence (`script`), `variants` (engine-only options: they change how the engine runs, not
what it builds, so the restatement has no such knob), `metrics`, and `reach`: the counters of
the restatement (oracle.COUNTERS) that the case claims to exercise and that must be above 0.
"""
import numpy as np

NC, INTRINSIC = 64, 12
RNG_SEED = 5  # the level generator's seed on both sides


def clustered(rng, n, d, nc=NC, intrinsic=INTRINSIC, noise=0.05):
    """test_gpu_batch_link._clustered: rows of `nc` clusters on an `intrinsic`-dimensional sheet"""
    C = rng.normal(size=(nc, intrinsic)).astype(np.float32)
    A = rng.normal(size=(intrinsic, d)).astype(np.float32) / np.sqrt(intrinsic)
    z = C[rng.integers(0, nc, n)] + 0.35 * rng.normal(size=(n, intrinsic)).astype(np.float32)
    x = z @ A + noise * rng.normal(size=(n, d)).astype(np.float32)
    return x.astype(np.float32)


def adversarial(rng, n, d, metric):
    """test_gpu_screen._adversarial's rows: duplicates, a 1-ulp neighbour, huge and tiny rows,
    integer rows with many exact ties, a zero row under cosine"""
    X = clustered(rng, n, d)
    X[1] = X[2]
    X[3] = X[2]
    X[4] = np.nextafter(X[2], np.float32(np.inf))
    X[10] *= np.float32(1e20)
    X[11] *= np.float32(1e-20)
    X[12] *= np.float32(2.0 ** 49)
    X[13] *= np.float32(2.0 ** -49)
    X[20:40] = rng.integers(-1, 2, size=(20, d)).astype(np.float32)
    if metric == 0:
        X[14] = 0.0
    return X


def ties(rng, n, d, metric):
    """small-integer rows: most distances repeat, so order is decided by id everywhere"""
    return rng.integers(-2, 3, size=(n, d)).astype(np.float32) + np.float32(0.5)


class Gen:
    """test_gpu_update.Gen: the clustered generator with the labels kept, so that a row's new
    vector can be drawn from another cluster than its own"""

    def __init__(self, seed, d):
        self.rng = np.random.default_rng(seed)
        self.d = d
        self.C = self.rng.normal(size=(NC, INTRINSIC)).astype(np.float32)
        self.A = self.rng.normal(size=(INTRINSIC, d)).astype(np.float32) / np.sqrt(INTRINSIC)

    def draw(self, labels):
        n = len(labels)
        z = self.C[labels] + 0.35 * self.rng.normal(size=(n, INTRINSIC)).astype(np.float32)
        return (z @ self.A + 0.05 * self.rng.normal(size=(n, self.d)).astype(np.float32)).astype(np.float32)

    def rows(self, n):
        labels = self.rng.integers(0, NC, n)
        return self.draw(labels), labels

    def moved(self, labels):
        return self.draw((labels + self.rng.integers(1, NC, len(labels))) % NC)


def keys_of(n):
    return np.arange(n, dtype=np.int64) * 3 + 7


BASE = dict(d=48, n=3000, M=12, m0=24, ef_construction=64, heuristic=2, keep_pruned=1)
DENSE = dict(d=32, n=2000, M=32, m0=63, heuristic=2, keep_pruned=1)  # the `dense` fixture's parameters
TWO_ADDS = (("add", 2, 3), ("add", 1, 1))  # two thirds, then the rest: the second descends a multi-layer graph


def _case(base=BASE, script=TWO_ADDS, data="clustered", metrics=(0, 1), reach=(), variants=({},), seed=1, **over):
    c = dict(base)
    c.update(over)
    shape = {k: c.pop(k) for k in ("d", "n", "M", "m0")}
    return dict(shape=shape, opts=c, script=script, data=data, metrics=metrics, reach=tuple(reach),
                variants=tuple(variants), seed=seed)


CASES = {}
CASES["base"] = _case(reach=("rule_drops", "fills", "overflow_commits", "commit_drops"),
                      # engine-only: kernel variants, the screening copy, a visited set that forgets
                      variants=({}, dict(build_mw_max=0), dict(build_mw_max=1 << 30), dict(fuse_descent=0),
                                dict(vis_log2=6)))
for _h in (0, 1, 2):
    for _k in (0, 1):
        CASES[f"rule-h{_h}-kp{_k}"] = _case(
            n=1500, heuristic=_h, keep_pruned=_k,
            reach=(("truncated_commits",) if _h < 2 else ("overflow_commits", "commit_drops")) +
                  (("rule_drops",) if _h else ()) + (("fills",) if _h and _k else ()))
for _a in (115, 130):
    CASES[f"rule-alpha{_a}"] = _case(n=1500, prune_alpha_pct=_a, reach=("rule_drops", "overflow_commits", "commit_drops"))
for _x in (1, 2, 3):
    CASES[f"search-expand{_x}"] = _case(n=1500, build_expand=_x, reach=("rule_drops",))
CASES["search-upper-efc32"] = _case(n=1500, upper_efc=32, reach=("rule_drops",))
for _e in (100, 256, 300, 512):
    CASES[f"tier-efc{_e}"] = _case(DENSE, ef_construction=_e, reach=("overflow_commits", "commit_drops", "rule_drops"))
CASES["sched-ratio20"] = _case(n=1500, batch_ratio_pct=20, reach=("overflow_commits",))
CASES["sched-min64"] = _case(n=1500, batch_min=64, reach=("overflow_commits",))
CASES["sched-max7"] = _case(n=1500, batch_max=7, reach=("overflow_commits",))
CASES["sched-one-by-one"] = _case(n=1500, batch_ratio_pct=0, batch_min=1, reach=("overflow_commits",))
CASES["dim200"] = _case(d=200, n=1500, metrics=(1,), reach=("rule_drops",))
CASES["dim768"] = _case(d=768, n=1000, metrics=(0,), reach=("rule_drops",))
CASES["dim1536"] = _case(d=1536, n=600, metrics=(0,), reach=("rule_drops",))
CASES["adversarial"] = _case(n=1500, data="adversarial", reach=("id_ties", "rule_drops"),
                             variants=(dict(screen=1), dict(screen=0)))
CASES["ties"] = _case(d=16, n=800, data="ties", reach=("id_ties", "overflow_commits"))
# (dead_skipped is not claimed: BatchDelete's repair leaves no live row pointing at a deleted one,
# so an insert's search never meets a deleted row; what this case reaches is the id gaps, the
# entries fix_entries moved and the repaired rows' stored distances in later commits)
CASES["dead"] = _case(script=(("add", 2, 3), ("delete", 5), ("add", 1, 1)), reach=("overflow_commits", "commit_drops"))
for _e in (0, 32, 512):
    CASES[f"link-ef{_e}"] = _case(n=1800, script=(("add_n", 1500), ("link", 300, _e)),
                                  reach=("link_rows", "link_edges", "mutual"))
CASES["update-scenario"] = _case(script=(("add", 1, 1), ("delete_rows", (5, 17, 1000, 2993)), ("update_spread", 300)),
                                 reach=("update_chunks", "repaired"))
CASES["update-chunks"] = _case(n=2000, batch_max=40, script=(("add", 1, 1), ("update_spread", 130)),
                               reach=("update_chunks", "repaired"))
CASES["update-top"] = _case(n=2000, script=(("add", 1, 1), ("update_top",)), reach=("update_chunks", "repaired"))
CASES["update-all"] = _case(n=2000, script=(("add", 1, 1), ("update_all",)), reach=("update_chunks", "repaired"))
# The link pass (k_batch_link<L, V, XW>) and the update's relink at the dimension configurations
# the cases above leave out (engine.hpp pick_cfg; they run at d 48, and test_gpu_batch_link.py /
# test_gpu_update.py at 768): one row per configuration, (d, metric, n, link batch,
# build_expand).  build_expand 1 .. 4 is spread so that the link pass's units for widths 1 - 2
# and 3 - 4 are both reached inside every group of configurations that has two dimensions here.
for _d, _m, _n, _nb, _x in ((96, 1, 900, 150, 1), (200, 0, 900, 150, 3), (400, 1, 900, 150, 2), (1000, 0, 700, 120, 4),
                            (1536, 1, 700, 120, 1), (2048, 0, 700, 120, 2), (3072, 1, 600, 100, 3),
                            (4096, 0, 600, 100, 4)):
    CASES[f"link-update-dim{_d}"] = _case(d=_d, n=_n, metrics=(_m,), build_expand=_x,
                                          script=(("add_n", _n - _nb), ("link", _nb, 0), ("update_spread", 40)),
                                          reach=("link_rows", "link_edges", "mutual", "update_chunks", "repaired"))


# tests/golden/batch_build.npz: an engine-built graph after each of these calls
GOLDEN = _case(d=16, n=300, M=8, m0=16, seed=3,
               script=(("add", 1, 2), ("add_n", 240), ("delete", 5), ("link", 60, 0), ("update_spread", 40)),
               reach=("overflow_commits", "link_edges", "mutual", "update_chunks", "repaired"))


def case_ids():
    return [(name, m) for name, c in CASES.items() for m in c["metrics"]]


def data_of(case, metric):
    """(gen, X, labels): the case's rows; gen draws the update scenarios' new vectors"""
    sh = case["shape"]
    seed = 1000 * case["seed"] + 17 * metric + sh["d"]
    if case["data"] == "clustered":
        gen = Gen(seed, sh["d"])
        X, labels = gen.rows(sh["n"])
        return gen, X, labels
    rng = np.random.default_rng(seed)
    fn = adversarial if case["data"] == "adversarial" else ties
    return None, fn(rng, sh["n"], sh["d"], metric), None


def levels_of(ex):
    """each row's level: its highest layer"""
    member = ex["deg"] != -2
    return (member.shape[0] - 1 - np.argmax(member[::-1], axis=0)).astype(np.int32)


def walk(case, metric, drv):
    """The case's call sequence on a driver.  A driver has add(keys, vecs, cap_top) -> levels
    (cap_top: levels limited to the current top layer, so that the rows form one batch),
    delete(keys), update(keys, vecs), set(**opts), export(); after every call the walk tells it
    snapshot(step name).  Everything here is a function of the case and of exports, so two
    drivers that build the same graph are given the same calls."""
    n = case["shape"]["n"]
    gen, X, labels = data_of(case, metric)
    keys = keys_of(n)
    done = 0
    rng = np.random.default_rng(case["seed"] + 99)
    for si, step in enumerate(case["script"]):
        op = step[0]
        if op in ("add", "add_n"):
            hi = step[1] if op == "add_n" else n * step[1] // step[2]  # rows up to hi
            drv.add(keys[done:hi], X[done:hi], False)
            done = hi
        elif op == "link":  # the rest of the rows in exactly one batch with the link pass on
            nb, lef = step[1], step[2]
            assert done + nb == n
            drv.set(batch_link=1, batch_link_ef=lef, batch_ratio_pct=0, batch_max=nb, batch_min=nb)
            drv.add(keys[done:n], X[done:n], True)
            done = n
        elif op == "delete":  # step[1] per cent of the rows added so far
            rows = np.sort(rng.permutation(done)[: done * step[1] // 100])
            drv.delete(keys[rows])
        elif op == "delete_rows":
            drv.delete(keys[np.array(step[1])])
        else:
            ex = drv.export()
            L, N = ex["deg"].shape
            live = np.flatnonzero((ex["dead"] == 0) & (ex["deg"][0] >= 0))
            if op == "update_spread":  # test_gpu_update._update_rows: spread over the ids, a row of
                # every upper layer, the top layer's entry; plus a deleted key and a key never added
                rows = {int(live[0]), int(live[-1]), int(ex["entry"][L - 1])}
                for l in range(1, L):
                    rows.add(int(np.flatnonzero((ex["deg"][l] >= 0) & (ex["dead"] == 0))[-1]))
                for r in live[np.linspace(1, len(live) - 2, step[1]).astype(int)]:
                    if len(rows) >= step[1]:
                        break
                    rows.add(int(r))
                rows = np.array(sorted(rows))
                dead = np.flatnonzero(ex["dead"] != 0)
                ukeys = np.concatenate([keys[rows], keys[dead[:1]], [1]])  # (1 is no key: keys are 7 mod 3)
                lab = np.concatenate([labels[rows], labels[dead[:1]], labels[:1]])
                order = rng.permutation(len(ukeys))  # not in row order
                ukeys, lab = ukeys[order], lab[order]
            elif op == "update_top":  # the top layer's entry and every member of the layer below the top
                assert L >= 3
                rows = np.flatnonzero((ex["deg"][L - 2] >= 0) & (ex["dead"] == 0))
                assert int(ex["entry"][L - 1]) in rows
                ukeys, lab = keys[rows], labels[rows]
            else:  # update_all: every live row
                ukeys, lab = keys[live], labels[live]
            drv.update(ukeys, gen.moved(lab))
        drv.snapshot(f"{si}:{op}")


class OracleDriver:
    """walk()'s calls on the restatement.  levels: per add call, the levels to use (the engine's,
    in the GPU test); None: the restatement's own preview."""

    def __init__(self, O, case, metric, levels=None, descending=False, keep=False):
        sh = case["shape"]
        self.O, self.opts = O, dict(case["opts"])
        self.g = O.Graph(metric=metric, order=O.ORDER_DEV, M=sh["M"], M0=sh["m0"], Ml=0.25, EfSearch=64, seed=RNG_SEED)
        self.g.set_batch_descending(descending)
        self.levels_in = None if levels is None else list(levels)
        self.levels, self.counters, self.snaps, self.keep = [], {}, [], keep

    def _count(self, cn):
        for k, v in cn.items():
            self.counters[k] = self.counters.get(k, 0) + v

    def add(self, keys, vecs, cap_top):
        if self.levels_in is not None:
            lv = self.levels_in.pop(0)
        else:
            lv = self.g.preview_levels(len(keys))
            if cap_top:
                lv = np.minimum(lv, len(self.g.topography()) - 1).astype(np.int32)
        self.levels.append(lv)
        self._count(self.g.add_batch(keys, vecs, lv, **self.opts))

    def delete(self, keys):
        assert all(self.g.delete(keys, mode=1, heuristic=self.opts["heuristic"], keep_pruned=self.opts["keep_pruned"]))

    def update(self, keys, vecs):
        self.found, cn = self.g.update(keys, vecs, **self.opts)
        self._count(cn)

    def set(self, **opts):
        self.opts.update(opts)

    def export(self):
        return self.g.export()

    def snapshot(self, name):
        if self.keep:
            self.snaps.append((name, self.g.export(), self.g.export_edge_dist()))


def run_oracle(O, case, metric, **kw):
    drv = OracleDriver(O, case, metric, **kw)
    walk(case, metric, drv)
    return drv


GOLDEN_METRIC = 0


def pack_golden(levels, snaps):
    """A walk's add levels and snapshots as the arrays of tests/golden/batch_build.npz.  Keys are
    stored once (rows are only appended); a snapshot's vectors are stored only where the next
    snapshot's do not begin with them (an update), and for the last."""
    out = {"nadd": np.int32(len(levels)), "nsteps": np.int32(len(snaps)), "keys": snaps[-1][1]["keys"]}
    for i, lv in enumerate(levels):
        out[f"levels{i}"] = lv
    for i, (_, ex, ed) in enumerate(snaps):
        for f in ("deg", "adj", "entry", "dead"):
            out[f"s{i}_{f}"] = ex[f]
        out[f"s{i}_edge_dist"] = ed
        nxt = snaps[i + 1][1]["vecs"] if i + 1 < len(snaps) else None
        if nxt is None or not np.array_equal(nxt[: len(ex["vecs"])].view(np.uint32), ex["vecs"].view(np.uint32)):
            out[f"s{i}_vecs"] = ex["vecs"]
    return out


def unpack_golden(fx):
    """(levels, [(export, edge distances)]) of pack_golden's arrays"""
    levels = [fx[f"levels{i}"] for i in range(int(fx["nadd"]))]
    snaps = []
    for i in range(int(fx["nsteps"])):
        ex = {f: fx[f"s{i}_{f}"] for f in ("deg", "adj", "entry", "dead")}
        N = ex["deg"].shape[1]
        j = next(j for j in range(i, int(fx["nsteps"])) if f"s{j}_vecs" in fx)
        ex["vecs"], ex["keys"] = fx[f"s{j}_vecs"][:N], fx["keys"][:N]
        snaps.append((ex, fx[f"s{i}_edge_dist"]))
    return levels, snaps


def same_export(a, b, ad=None, bd=None, what=""):
    """two exports equal in every field, adj in stored order; edge distances by their bits"""
    for f in ("keys", "deg", "entry", "dead", "adj"):
        assert a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), (what, f, _first_diff(a[f], b[f]))
    assert np.array_equal(a["vecs"].view(np.uint32), b["vecs"].view(np.uint32)), (what, "vecs")
    if ad is not None:
        assert ad.shape == bd.shape, (what, "edge_dist shape")
        assert np.array_equal(ad.view(np.uint32), bd.view(np.uint32)), (what, "edge_dist", _first_diff(ad, bd))


def _first_diff(a, b):
    if a.shape != b.shape:
        return (a.shape, b.shape)
    w = np.argwhere(a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else np.argwhere(a != b)
    return (len(w), w[0].tolist(), a[tuple(w[0])].item(), b[tuple(w[0])].item()) if len(w) else None
