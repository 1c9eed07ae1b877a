"""The LSH index on the bench index (1M x 768 cosine, built as bench.py builds it).

  hashing   device ms for every row at P = 32 (4 x 8) and P = 256 (8 x 32), beside the time to
            stream the same rows once at 6.3 TB/s; the fraction of signs the canonical pass decided
  rebuild   the tables' device ms (last_lsh_rebuild_ns)
  search    (T, b) = (4, 8), (8, 16), (16, 16) (16 x 20 = 320 projections is past the limit of
            256; 16 x 16 is the widest shape with 16 tables) at batches of 1,024 and 16,384 queries, k = 10:
            kernel ms (best of 5 after 2 warm-ups, mhnsw_last_kernel_ms: query hashing included),
            mean and max ncand, recall@10 against the exact search; the session's exact top-10
            and beam ef 64 times alongside

Writes <out>/lsh_index.txt and .json.
Usage: python tools/lsh_probe.py [--out profiles] [--nbase N]"""
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
args = ap.parse_args()

dev = torch.device("cuda")
n, d, K = args.nbase, 768, 10
STREAM_TBS = 6.3
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
QS = {B: gen_vectors(B, d, 4321, 12, 1000, dev, "cosine").cpu().numpy() for B in (1024, 16384)}
g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=40,
            ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4,
            batch_ratio_pct=20, upper_efc=128, screen=1)
g.add_device(np.arange(n, dtype=np.int64), X.data_ptr(), n, d)
torch.cuda.synchronize()


def best(fn, reps=5, warm=2):
    """best kernel ms of `reps` runs after `warm` warm-ups, and the last result"""
    ms = []
    for i in range(warm + reps):
        r = fn()
        if i >= warm:
            ms.append(g.last_kernel_ms())
    return min(ms), r


rec = {"rows": n, "dim": d, "stream_ms": n * d * 4 / (STREAM_TBS * 1e12) * 1e3, "hash": [], "search": [], "base": {}}
exact = {}
for B, Q in QS.items():
    ms, r = best(lambda: g.search_arrays(Q, K, mode=H.MODE_EXACT))
    exact[B] = r[0]
    bms, br = best(lambda: g.search_arrays(Q, K, mode=H.MODE_BEAM, ef=64))
    hit = np.mean([len(set(br[0][i]) & set(r[0][i])) / K for i in range(B)])
    rec["base"][B] = dict(exact_ms=ms, beam64_ms=bms, beam64_recall=float(hit))

for T, b in ((4, 8), (8, 32)):  # hashing: enable on the filled handle hashes every row
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.EnableLSH(T, b)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    rec["hash"].append(dict(T=T, b=b, P=T * b, wall_ms=min(ts), uncertain=g.get_option("last_lsh_uncertain"),
                            fraction=g.get_option("last_lsh_uncertain") / (n * T * b)))

for T, b in ((4, 8), (8, 16), (16, 16)):
    g.EnableLSH(T, b)
    g.search_lsh_arrays(QS[1024][:1], K)  # builds the tables
    rebuild = g.get_option("last_lsh_rebuild_ns") / 1e6
    for B, Q in QS.items():
        ms, r = best(lambda: g.search_lsh_arrays(Q, K))
        hit = np.mean([len(set(r[0][i, : r[2][i]]) & set(exact[B][i])) / K for i in range(B)])
        rec["search"].append(dict(T=T, b=b, B=B, kernel_ms=ms, ncand_mean=float(r[3].mean()), ncand_max=int(r[3].max()),
                                  recall=float(hit), rebuild_ms=rebuild))
g.close()

lines = ["LSH index on the bench index: %d x %d cosine, k = %d" % (n, d, K), "",
         "streaming the rows once at %.1f TB/s: %.3f ms" % (STREAM_TBS, rec["stream_ms"])]
for h in rec["hash"]:
    lines.append("hash P = %3d (%d x %d): %8.2f ms wall (enable: hashing + sync); %d signs (%.4f %%) decided canonically" %
                 (h["P"], h["T"], h["b"], h["wall_ms"], h["uncertain"], 100 * h["fraction"]))
for B, v in rec["base"].items():
    lines.append("B = %5d: exact top-10 %.2f ms, beam ef 64 %.2f ms (recall %.4f)" % (B, v["exact_ms"], v["beam64_ms"], v["beam64_recall"]))
for s in rec["search"]:
    lines.append("(T, b) = (%2d, %2d) B = %5d: %8.2f ms, ncand mean %.1f max %d, recall@10 %.4f; table rebuild %.2f ms" %
                 (s["T"], s["b"], s["B"], s["kernel_ms"], s["ncand_mean"], s["ncand_max"], s["recall"], s["rebuild_ms"]))
print("\n".join(lines))
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "lsh_index.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
with open(os.path.join(args.out, "lsh_index.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
