"""The Analyzer on the bench index (1M x 768 cosine, built as bench.py builds it) with 10 % of
the rows deleted at random.

  reachability      wall ms, device ms (last_reach_ns), scratch bytes, the counts; the bytes it
                    must read -- per layer deg and the dead bytes of every row (seed and count
                    passes) plus the adjacency rows of the rows it visits -- over its device time,
                    beside the 6.3 TB/s streaming rate
  quality_metrics   wall ms (histogram, hop BFS of the 100 sample rows, their 100 x 100 distances)
  hops              100 keys at depth 10, wall ms
  relink            1,000 random live rows: wall ms, beside update_arrays of the same rows with their
                    own vectors (what Relink replaces), alternating on the same handle, best of 3
  export + host BFS the route the calls replace: Graph.export() and the numpy restatement's
                    reachability (tests/analyzer_ref.py) on it, wall s

Writes <out>/analyzer.txt and .json.
Usage: python tools/analyzer_probe.py [--out profiles] [--nbase N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hnsw_amd as H  # noqa: E402
from bench import gen_vectors  # noqa: E402
from tests import analyzer_ref as AR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--nbase", type=int, default=1_000_000)
args = ap.parse_args()

dev = torch.device("cuda")
n, d = args.nbase, 768
M, M0 = 16, 40
STREAM_TBS = 6.3
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
KEYS = np.arange(n, dtype=np.int64)
rng = np.random.default_rng(99)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


g = H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=M0,
            ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4,
            batch_ratio_pct=20, upper_efc=128, screen=1)
_, build_ms = wall(lambda: g.add_device(KEYS, X.data_ptr(), n, d))
gone = np.sort(rng.choice(n, n // 10, replace=False)).astype(np.int64)
out = np.zeros(len(gone), np.uint8)
assert H.load().mhnsw_delete(g._h, gone.ctypes.data_as(C.POINTER(C.c_int64)), len(gone),
                             out.ctypes.data_as(C.POINTER(C.c_uint8))) == 0 and out.all()
an = H.Analyzer(g)
rec = {"rows": n, "dim": d, "deleted": len(gone), "build_ms": build_ms}

an.Reachability()  # (the scratch buffers exist from here on)
r, ms = wall(an.Reachability)
dev_ms = g.get_option("last_reach_ns") / 1e6
caps = [M0 + 1] + [M + 1] * (len(r.members) - 1)
# deleted rows route and are read too: the live counts understate the rows visited by at most the deleted rows
read = sum(2 * n * 4 + n + r.reached[l] * 4 * (1 + caps[l]) for l in range(len(r.members)))
rec["reachability"] = dict(wall_ms=ms, device_ms=dev_ms, members=r.members, reached=r.reached, depth=r.depth,
                           unreachable=len(r.unreachable_keys), bytes_read=read, tb_per_s=read / (dev_ms * 1e-3) / 1e12,
                           scratch_bytes=g.get_option("last_analyzer_scratch_bytes"))
q, ms = wall(an.QualityMetrics)
rec["quality_metrics"] = dict(wall_ms=ms, metrics=q.__dict__, scratch_bytes=g.get_option("last_analyzer_scratch_bytes"))
live = np.setdiff1d(KEYS, gone)
hk = np.sort(rng.choice(live, 100, replace=False))
hp, ms = wall(lambda: an.Hops(hk, 10))
rec["hops"] = dict(wall_ms=ms, keys=100, depth=10, found=int((hp > 0).sum()), beyond=int((hp < 0).sum()),
                   scratch_bytes=g.get_option("last_analyzer_scratch_bytes"))

t0 = time.perf_counter()
ex = g.export()
t1 = time.perf_counter()
w = AR.reachability(ex)
t2 = time.perf_counter()
assert w["reached"] == r.reached and ex["keys"][w["unreachable"]].tolist() == r.unreachable_keys
rec["export_host_bfs"] = dict(export_s=t1 - t0, bfs_s=t2 - t1, export_bytes=int(sum(v.nbytes for v in ex.values())))
del ex

g.relink_arrays(np.sort(rng.choice(live, 1000, replace=False)))  # (the update path's scratch exists from here on)
rk = np.sort(rng.choice(live, 1000, replace=False))
own = X[torch.as_tensor(rk, device=dev)].cpu().numpy()
rms, ums = [], []
for _ in range(3):  # alternating, on the same handle: each call relinks the graph the last one left
    f, ms = wall(lambda: g.relink_arrays(rk))
    assert f.all()
    rms.append(ms)
    f, ms = wall(lambda: g.update_arrays(rk, own))
    assert f.all()
    ums.append(ms)
rec["relink"] = dict(rows=1000, relink_ms=rms, update_own_vectors_ms=ums, vector_bytes_not_sent=int(own.nbytes))
rms, ums = min(rms), min(ums)
b, a = an.Repair()
rec["repair"] = dict(unreachable_before=b, unreachable_after=a)
g.close()

R = rec["reachability"]
lines = ["Analyzer on the bench index: %d x %d cosine, M %d, m0 %d, efC 400, %d rows deleted at random" % (n, d, M, M0, len(gone)),
         "",
         "reachability     %8.2f ms wall, %8.2f ms device; members %s reached %s levels %s; %d unreachable" %
         (R["wall_ms"], R["device_ms"], R["members"], R["reached"], R["depth"], R["unreachable"]),
         "                 reads >= %.1f MB: %.3f TB/s of the %.1f TB/s streaming rate; scratch %.1f MB" %
         (R["bytes_read"] / 1e6, R["tb_per_s"], STREAM_TBS, R["scratch_bytes"] / 1e6),
         "quality_metrics  %8.2f ms wall; %s" % (rec["quality_metrics"]["wall_ms"], rec["quality_metrics"]["metrics"]),
         "hops             %8.2f ms wall (100 keys, depth 10: %d pairs found, %d beyond); scratch %.1f MB" %
         (rec["hops"]["wall_ms"], rec["hops"]["found"], rec["hops"]["beyond"], rec["hops"]["scratch_bytes"] / 1e6),
         "export + host BFS %7.2f s export (%.2f GB) + %.2f s numpy BFS: the route replaced" %
         (rec["export_host_bfs"]["export_s"], rec["export_host_bfs"]["export_bytes"] / 1e9, rec["export_host_bfs"]["bfs_s"]),
         "relink           %8.2f ms wall for 1,000 rows; update of the same rows with their own vectors %.2f ms" %
         (rms, ums),
         "                 (best of 3 each, alternating: relink %s, update %s)" %
         (["%.2f" % v for v in rec["relink"]["relink_ms"]], ["%.2f" % v for v in rec["relink"]["update_own_vectors_ms"]]),
         "repair           %d unreachable before, %d after" % (b, a), ""]
print("\n".join(lines))
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "analyzer.txt"), "w") as fh:
    fh.write("\n".join(lines))
with open(os.path.join(args.out, "analyzer.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
