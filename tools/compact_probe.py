"""Compaction on the bench index (1M x 768 cosine, built as bench.py builds it).

Legs, each on a fresh build: 10 %, 30 % and 50 % of the rows deleted uniformly at random, and
30 % deleted as one contiguous block.  Per leg: last_compact_ns, the bytes the call moves
(every array's row of the rows from the first deleted one on -- f32, fp16 + aux, norm, key,
level and each layer's deg, and adj / adjd for the layer's members -- read once and written once), the fraction of the
6.3 TB/s streaming rate DESIGN.md uses for copy-like kernels, and last_compact_scratch_bytes.

At 30 % uniform also: what the caller gains (kernel ms of the exact top-10 search and of an
exact range search at the 10th distance, 1,024 queries, and the wall ms of a BatchDelete of
1 % of the live rows, each before and after the compaction), the sweep of compact_stage_rows,
and the only route to the same state without mhnsw_compact: export() + host remap +
import_graph() wall time.

Writes <out>/compaction.txt and .json.
Usage: python tools/compact_probe.py [--out profiles] [--nbase N] [--no-route]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hnsw_amd as H  # noqa: E402
from bench import gen_vectors  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
ap.add_argument("--nbase", type=int, default=1_000_000)
ap.add_argument("--no-route", action="store_true", help="skip the export + remap + import comparison")
ap.add_argument("--stages", default="1024,4096,16384,65536,262144")
args = ap.parse_args()

dev = torch.device("cuda")
n, d, B, STREAM = args.nbase, 768, 1024, 6.3e12
M, M0 = 16, 40
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
Q = gen_vectors(B, d, 1234 + 7777, 12, 1000, dev, "cosine").cpu().numpy()
KEYS = np.arange(n, dtype=np.int64)
rng = np.random.default_rng(99)


def build(**options):
    g = H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=M0,
                ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4,
                batch_ratio_pct=20, upper_efc=128, screen=1, **options)
    g.reserve(n, d)
    g.add_device(KEYS, X.data_ptr(), n, d)
    return g


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def moved_bytes(g, dead):
    """bytes mhnsw_compact reads and writes: every per-row array, the live rows past the first deleted one"""
    first = int(np.argmax(dead))
    rows = int((~dead[first:]).sum())
    pitch, topo = g.get_option("pitch"), g.Topography()
    # an adjacency row moves only for the members of its layer: the layer's share of the live rows
    row = pitch * 4 + pitch * 2 + 8 + 4 + 8 + 4 + sum(4 + ((M0 if l == 0 else M) + 1) * 8 * c / max(topo[0], 1)
                                                      for l, c in enumerate(topo))
    return rows, int(2 * rows * row)


def searches(g, radius):
    out = {}
    for _ in range(2):  # (the first call after a mutation rebuilds the exact path's planes)
        g.search_arrays(Q, 10, mode=H.MODE_EXACT)
    out["exact_top10_ms"] = g.last_kernel_ms()
    for _ in range(2):
        g.range_search_arrays(Q, radius, mode=H.MODE_EXACT)
    out["exact_range_ms"] = g.last_kernel_ms()
    return out


def compact_leg(name, dead, extras=False, **options):
    g = build(**options)
    _, del_ms = wall(lambda: g.BatchDelete(KEYS[dead]))
    rec = {"leg": name, "dead_rows": int(dead.sum()), "delete_ms": del_ms}
    live = KEYS[~dead]
    if extras:
        _, xd, _ = g.search_arrays(Q, 10, mode=H.MODE_EXACT)
        radius = xd[:, 9].copy()
        rec["before"] = searches(g, radius)
        one = rng.permutation(live)[: len(live) // 100]
        _, rec["before"]["delete_1pct_ms"] = wall(lambda: g.BatchDelete(one))
        dead = dead.copy()
        dead[one] = True
        live = KEYS[~dead]
    rows, nbytes = moved_bytes(g, dead)
    removed, rec["compact_wall_ms"] = wall(g.Compact)
    assert removed == int(dead.sum()) and g.get_option("last_compact_dangling") == 0
    ns = g.get_option("last_compact_ns")
    rec.update(rows_moved=rows, bytes_moved=nbytes, compact_ms=ns / 1e6, stream_fraction=nbytes / (ns * 1e-9) / STREAM,
               scratch_bytes=g.get_option("last_compact_scratch_bytes"), stage_rows=g.get_option("compact_stage_rows"))
    if extras:
        rec["after"] = searches(g, radius)
        one = rng.permutation(live)[: len(live) // 100]
        _, rec["after"]["delete_1pct_ms"] = wall(lambda: g.BatchDelete(one))
    g.close()
    return rec


def route_leg(dead):
    """export + host remap + import: the same state without mhnsw_compact (filters are lost)"""
    g = build()
    g.BatchDelete(KEYS[dead])

    def route():
        ex = g.export()
        live = ~ex["dead"].astype(bool)
        new = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
        adj = ex["adj"][:, live]
        adj = np.where(adj >= 0, new[np.maximum(adj, 0)], -1).astype(np.int32)
        entry = np.where(ex["entry"] >= 0, new[np.maximum(ex["entry"], 0)], -1).astype(np.int32)
        g2 = H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=M0)
        g2.import_graph(ex["keys"][live], ex["vecs"][live], ex["deg"][:, live], adj, entry)
        return g2

    g2, ms = wall(route)
    assert g2.Len() == g.Len()
    g2.close()
    g.close()
    return ms


uniform = {f: rng.random(n) < f for f in (0.1, 0.3, 0.5)}
block = np.zeros(n, bool)
block[n // 3: n // 3 + (3 * n) // 10] = True
legs = [compact_leg("uniform 10 %", uniform[0.1]), compact_leg("uniform 30 %", uniform[0.3], extras=True),
        compact_leg("uniform 50 %", uniform[0.5]), compact_leg("block 30 %", block)]
sweep = [compact_leg("uniform 30 %%, stage %s" % s, uniform[0.3], compact_stage_rows=int(s))
         for s in args.stages.split(",") if s]
route_ms = None if args.no_route else route_leg(uniform[0.3])

lines = ["compaction on the bench index: %d x %d cosine, M %d, m0 %d, efC 400" % (n, d, M, M0), ""]
fmt = "%-28s dead %8d  moved %8d rows %7.2f GB  %8.2f ms  %.2f of 6.3 TB/s  scratch %7.1f MB  stage %d"
for r in legs + sweep:
    lines.append(fmt % (r["leg"], r["dead_rows"], r["rows_moved"], r["bytes_moved"] / 1e9, r["compact_ms"],
                        r["stream_fraction"], r["scratch_bytes"] / 1e6, r["stage_rows"]))
x = legs[1]
lines += ["", "what the caller gains at 30 % dead (1,024 queries; before -> after):"]
for key in ("exact_top10_ms", "exact_range_ms", "delete_1pct_ms"):
    lines.append("  %-16s %9.2f -> %9.2f" % (key, x["before"][key], x["after"][key]))
if route_ms is not None:
    lines += ["", "export + host remap + import_graph of the same index: %.0f ms wall (compaction: %.1f ms wall)"
              % (route_ms, x["compact_wall_ms"])]
print("\n".join(lines))
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "compaction.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
with open(os.path.join(args.out, "compaction.json"), "w") as f:
    json.dump({"legs": legs, "stage_sweep": sweep, "route_ms": route_ms}, f, indent=1)
