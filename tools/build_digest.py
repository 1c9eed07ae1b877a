"""Digest of the graphs the insert and delete kernels build: one line per case
with the sha256 of the exported deg / adj / entry / dead arrays and the build
counters.  Run once per library (MHNSW_LIB=...) and compare the outputs: a
change that must leave the kernels alone gives byte-identical files
(profiles/build_refactor.txt).
Usage: python tools/build_digest.py > digest.txt"""
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_amd as H  # noqa: E402
from tests.test_gpu_parity import _clustered  # noqa: E402

COUNTERS = ("build_dist_evals", "build_expansions", "dropped_proposals", "build_screened", "build_f32_rows")


def line(name, g):
    ex, st = g.export(), g.stats()
    h = hashlib.sha256()
    for k in ("deg", "adj", "entry", "dead"):
        h.update(np.ascontiguousarray(ex[k]).tobytes())
    print(name, h.hexdigest(), " ".join(f"{k}={st[k]}" for k in COUNTERS), flush=True)


def main():
    n = int(os.environ.get("DIGEST_N", 20000))
    for d in (96, 768):
        X = _clustered(np.random.default_rng(d), n, d)
        for efc, xw, fuse, mw in itertools.product((64, 200, 400), (1, 2, 3, 4), (0, 1), (0, None)):
            opts = dict(build_expand=xw, fuse_descent=fuse)
            if mw is not None:
                opts["build_mw_max"] = mw
            g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance if d == 96 else H.EuclideanDistance,
                        Rng=9, build_mode=H.BUILD_BATCH, ef_construction=efc, heuristic=2, **opts)
            g.add_arrays(np.arange(n), X)
            line(f"batch d={d} efc={efc} expand={xw} fuse_descent={fuse} build_mw_max={'default' if mw is None else mw}", g)
            g.close()
    for d in (100, 768):
        rng = np.random.default_rng(d)
        X = rng.uniform(-1, 1, (1500, d)).astype(np.float32)
        g = H.Graph(M=16, Ml=0.25, EfSearch=20, Distance=H.CosineDistance if d == 100 else H.EuclideanDistance, Rng=5)
        g.add_arrays(np.arange(1500), X)
        line(f"compat d={d} add", g)
        g.BatchDelete([int(x) for x in rng.permutation(1500)[:300]])
        line(f"compat d={d} delete", g)
        g.close()


if __name__ == "__main__":
    main()
