"""The partitions on the bench index's rows (1M x 768 cosine, generated as bench.py generates them).

  assign    wall ms (enable on the filled handle: every row assigned, then a sync; best of 3) at
            P = 64, 1024, 4096 with rows of the index as centroids, as a rate over its N P d 2 flop,
            beside one streaming read of the rows and, where the exact path's GEMM timer is set
            (last_gemm_ns of an exact_precision 0 search), that GEMM's time; the share of rows the
            canonical pass assigned
  train     one TrainPartitions iteration at P = 1024: device ms (last_part_train_ns) and, of it,
            the list rebuild (last_part_rebuild_ns)
  search    16,384 queries, k = 10, P = 1024 after that iteration, nprobe = 1, 8, 32: kernel ms
            (best of 5 after 2 warm-ups, probe order included), candidates per query, recall@10
            against the exact search; the session's exact and LSH (8 x 16) times alongside.
            --graph builds the bench graph instead of a flat store and adds beam ef 64.

  --scan    the search cases again with part_scan 0 and 1 alternating on the same handle, at
            part_scan_seed 0, 1 and 2: kernel ms of both, survivors per query, fallback queries
            and the inversion + scan kernel's share (last_part_scan_ns; at seed 0 everything
            between the probe order and the finish: both inversions, the seed scan, the pick
            and the tiles) -> <out>/part_scan.txt

Writes <out>/partitions.txt and .json.
Usage: python tools/part_probe.py [--out profiles] [--nbase N] [--graph] [--scan]"""
import argparse
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

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--nbase", type=int, default=1_000_000)
ap.add_argument("--graph", action="store_true")
ap.add_argument("--scan", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda")
n, d, K, B = args.nbase, 768, 10, 16384
STREAM_TBS = 6.3
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
Q = gen_vectors(B, d, 4321, 12, 1000, dev, "cosine").cpu().numpy()
if args.graph:
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=40,
                ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4,
                batch_ratio_pct=20, upper_efc=128, screen=1)
else:
    g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, build_mode=H.BUILD_FLAT)
g.add_device(np.arange(n, dtype=np.int64), X.data_ptr(), n, d)
torch.cuda.synchronize()
Xh = X[:: max(n // 4096, 1)][:4096].cpu().numpy()  # centroids: rows of the index


def best(fn, reps=5, warm=2):
    ms = []
    for i in range(warm + reps):
        r = fn()
        if i >= warm:
            ms.append(g.last_kernel_ms())
    return min(ms), r


rec = {"rows": n, "dim": d, "stream_ms": n * d * 4 / (STREAM_TBS * 1e12) * 1e3, "assign": [], "search": [], "base": {}}
g.set_option("exact_precision", 0)
g.search_arrays(Q, K, mode=H.MODE_EXACT)
try:  # (the first query chunk's score GEMM; the option fails when that search was not timed)
    gemm_ms = g.get_option("last_gemm_ns") / 1e6
except H.HnswError:
    gemm_ms = None
g.set_option("exact_precision", 3)
ems, er = best(lambda: g.search_arrays(Q, K, mode=H.MODE_EXACT))
rec["base"]["exact_ms"] = ems
if args.graph:
    bms, br = best(lambda: g.search_arrays(Q, K, mode=H.MODE_BEAM, ef=64))
    rec["base"]["beam64_ms"] = bms
    rec["base"]["beam64_recall"] = float(np.mean([len(set(br[0][i]) & set(er[0][i])) / K for i in range(B)]))
g.EnableLSH(8, 16)
lms, lr = best(lambda: g.search_lsh_arrays(Q, K))
rec["base"]["lsh_ms"] = lms
rec["base"]["lsh_recall"] = float(np.mean([len(set(lr[0][i, : lr[2][i]]) & set(er[0][i])) / K for i in range(B)]))
rec["base"]["lsh_ncand"] = float(lr[3].mean())
rec["base"]["f32_mfma_gemm_ms"] = gemm_ms

for P in (64, 1024, 4096):
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.EnablePartitions(P, centroids=Xh[:P])
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    unc = g.get_option("last_part_uncertain")
    rec["assign"].append(dict(P=P, wall_ms=min(ts), gflop=2.0 * n * P * d / 1e9, uncertain=unc, fraction=unc / n))

g.EnablePartitions(1024, centroids=Xh[:1024])
moved = g.TrainPartitions(1)
rec["train"] = dict(P=1024, moved=moved, train_ms=g.get_option("last_part_train_ns") / 1e6,
                    rebuild_ms=g.get_option("last_part_rebuild_ns") / 1e6)
for m in (1, 8, 32):
    ms, r = best(lambda: g.search_partitions_arrays(Q, K, m))
    hit = np.mean([len(set(r[0][i, : r[2][i]]) & set(er[0][i])) / K for i in range(B)])
    rec["search"].append(dict(nprobe=m, kernel_ms=ms, ncand_mean=float(r[3].mean()), ncand_max=int(r[3].max()),
                              recall=float(hit)))
if args.scan:  # the same cases, the walk and the partition-major scan alternating on this handle
    rec["scan"] = []
    for seed in (0, 1, 2):
        for m in (1, 8, 32):
            row = dict(nprobe=m, seed=seed)
            for on in (0, 1):
                g.set_option("part_scan", on)
                g.set_option("part_scan_min_b", 1)
                g.set_option("part_scan_seed", seed)
                ms, r = best(lambda: g.search_partitions_arrays(Q, K, m))
                row["scan_ms" if on else "walk_ms"] = ms
                if on and g.get_option("last_part_scan_queries"):
                    row.update(pairs_per_query=g.get_option("last_part_scan_pairs") / B,
                               fallback=g.get_option("last_part_scan_fallback_queries"),
                               invert_tiles_ms=g.get_option("last_part_scan_ns") / 1e6)
            rec["scan"].append(row)
    g.set_option("part_scan", 0)
g.close()

lines = ["Partitions on the bench rows: %d x %d cosine, k = %d, B = %d" % (n, d, K, B), "",
         "streaming the rows once at %.1f TB/s: %.3f ms" % (STREAM_TBS, rec["stream_ms"])]
for a in rec["assign"]:
    lines.append("assign P = %4d: %9.2f ms wall (enable: assignment + sync), %.0f GFLOP -> %.1f TFLOP/s; "
                 "%d rows (%.4f %%) assigned canonically" %
                 (a["P"], a["wall_ms"], a["gflop"], a["gflop"] / a["wall_ms"], a["uncertain"], 100 * a["fraction"]))
t = rec["train"]
lines.append("train P = %d, one iteration: %.2f ms device (list rebuild %.2f ms of it), %d rows moved" %
             (t["P"], t["train_ms"], t["rebuild_ms"], t["moved"]))
b = rec["base"]
lines.append("exact path at exact_precision 0, first query chunk's f32-MFMA score GEMM (last_gemm_ns): " +
             ("%.2f ms" % b["f32_mfma_gemm_ms"] if b["f32_mfma_gemm_ms"] is not None else "not measured (no timer)"))
lines.append("exact top-10 %.2f ms; LSH 8 x 16 %.2f ms (ncand %.1f, recall %.4f)%s" %
             (b["exact_ms"], b["lsh_ms"], b["lsh_ncand"], b["lsh_recall"],
              "; beam ef 64 %.2f ms (recall %.4f)" % (b["beam64_ms"], b["beam64_recall"]) if args.graph else
              "; beam ef 64 not measured (flat store)"))
for s in rec["search"]:
    lines.append("P = 1024 nprobe = %2d: %8.2f ms, ncand mean %.1f max %d, recall@10 %.4f" %
                 (s["nprobe"], s["kernel_ms"], s["ncand_mean"], s["ncand_max"], s["recall"]))
print("\n".join(lines))
os.makedirs(args.out, exist_ok=True)
if args.scan:
    sl = ["Partition scan on the bench rows: %d x %d cosine, P = 1024, k = %d, B = %d; exact top-10 %.2f ms" %
          (n, d, K, B, b["exact_ms"])]
    for s in rec["scan"]:
        sl.append("seed %d nprobe %2d: walk %8.2f ms, scan %8.2f ms" % (s["seed"], s["nprobe"], s["walk_ms"], s["scan_ms"]) +
                  (" (%s %.2f ms), %.1f survivors per query, %d fallback queries" %
                   ("inversion + tiles" if s["seed"] else "seed scan + pick + inversions + tiles", s["invert_tiles_ms"], s["pairs_per_query"], s["fallback"]) if "fallback" in s else " (the walk ran)"))
    print("\n".join(sl))
    with open(os.path.join(args.out, "part_scan.txt"), "w") as fh:
        fh.write("\n".join(sl) + "\n")
with open(os.path.join(args.out, "partitions.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
with open(os.path.join(args.out, "partitions.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
