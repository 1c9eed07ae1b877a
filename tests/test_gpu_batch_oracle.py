"""GPU: the batched insert, its link pass and the in-place update against their plain-C
restatement (oracle.c og_add_batch / og_update), bit for bit: for every case of
tests/batch_ref.py's table the engine and the restatement are given the same calls and the same
levels, and after every call the whole exports are equal -- keys, deg, entry, dead, adj in
stored order -- and so are the bits of every stored edge distance.  There is no tolerance.

The two sides agree only where the engine drops no reverse proposal (which ones it drops
depends on arrival order): every case asserts dropped_proposals == 0 on the engine, and
tests/test_batch_oracle.py shows on the CPU that the restatement would not have dropped one
either and that each case reaches the rules it claims to test.

record_golden() is how tests/golden/batch_build.npz was produced: run once on an MI355X after
these tests passed; test_golden_current holds the engine to it, tests/test_batch_oracle.py the
restatement (without a GPU).
"""
import os

import numpy as np
import pytest

from tests import batch_ref as BR
from tests.test_gpu_parity import _metric_fn

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_build.npz")


class EngineDriver:
    """BR.walk()'s calls on the engine; the levels of every add are kept for the restatement"""

    def __init__(self, H, case, metric, variant=None):
        sh = case["shape"]
        opts = dict(case["opts"])
        opts.update(variant or {})
        self.g = H.Graph(M=sh["M"], Ml=0.25, EfSearch=64, Distance=_metric_fn(H, metric), Rng=BR.RNG_SEED,
                         build_mode=H.BUILD_BATCH, m0=sh["m0"], **opts)
        self.levels, self.snaps = [], []

    def add(self, keys, vecs, cap_top):
        lv = self.g.preview_levels(len(keys))
        if cap_top:
            lv = np.minimum(lv, self.g.export()["deg"].shape[0] - 1).astype(np.int32)
        self.levels.append(lv)
        self.g.add_arrays(keys, vecs, levels=lv)

    def delete(self, keys):
        assert all(self.g.BatchDelete(keys))

    def update(self, keys, vecs):
        self.found = self.g.update_arrays(keys, vecs)

    def set(self, **opts):
        for k, v in opts.items():
            self.g.set_option(k, v)

    def export(self):
        return self.g.export()

    def snapshot(self, name):
        assert self.g.stats()["dropped_proposals"] == 0, name
        self.snaps.append((name, self.g.export(), self.g.export_edge_dist()))


def oracle_equal(O, case, metric, eng):
    """the restatement, given the engine's levels, gives the engine's exports after every call"""
    ref = BR.run_oracle(O, case, metric, levels=eng.levels, keep=True)
    assert ref.counters["dropped_proposals"] == 0
    assert len(ref.snaps) == len(eng.snaps) == len(case["script"])
    for (step, ex, ed), (_, rx, rd) in zip(eng.snaps, ref.snaps):
        BR.same_export(ex, rx, ed, rd, what=step)
    if hasattr(eng, "found"):
        assert eng.found.tolist() == ref.found.tolist()
    return ref


def _ids():
    return [(name, m, vi) for name, m in BR.case_ids() for vi in range(len(BR.CASES[name]["variants"]))]


@pytest.mark.parametrize("name,metric,vi", _ids(),
                         ids=lambda v: v if isinstance(v, str) else str(v))
def test_engine_equals_restatement(H, O, name, metric, vi):
    case = BR.CASES[name]
    eng = EngineDriver(H, case, metric, case["variants"][vi])
    BR.walk(case, metric, eng)
    ref = oracle_equal(O, case, metric, eng)
    if "link_rows" in case["reach"]:  # the engine's own counters of the link pass
        assert eng.g.get_option("last_link_rows") == ref.counters["link_rows"]
        assert eng.g.get_option("last_link_edges") == ref.counters["link_edges"]
    if "update_chunks" in case["reach"]:
        assert eng.g.get_option("last_update_chunks") == ref.counters["update_chunks"]
        assert eng.g.get_option("last_update_repaired") == ref.counters["repaired"]
    eng.g.close()


def record_golden(H, path=GOLDEN):
    """BR.GOLDEN on the engine (cosine): the levels of every add and the export plus edge
    distances after every call, as one compressed archive (BR.pack_golden)"""
    eng = EngineDriver(H, BR.GOLDEN, BR.GOLDEN_METRIC)
    BR.walk(BR.GOLDEN, BR.GOLDEN_METRIC, eng)
    np.savez_compressed(path, **BR.pack_golden(eng.levels, eng.snaps))
    eng.g.close()


def test_golden_current(H):
    """the engine still builds the recorded graph"""
    levels, snaps = BR.unpack_golden(np.load(GOLDEN))
    eng = EngineDriver(H, BR.GOLDEN, BR.GOLDEN_METRIC)
    BR.walk(BR.GOLDEN, BR.GOLDEN_METRIC, eng)
    assert len(eng.snaps) == len(snaps) and len(eng.levels) == len(levels)
    for lv, want in zip(eng.levels, levels):
        assert np.array_equal(lv, want)
    for (step, ex, ed), (wx, wd) in zip(eng.snaps, snaps):
        BR.same_export(wx, ex, wd, ed, what=step)
    eng.g.close()
