"""Wide exact search (option "exact_wide") on the bench rows (1M x 768 cosine, bench.py's vectors).

The exact path reads the rows only, never the graph, so the handle is a flat index
(BUILD_FLAT) over the same vectors: no graph build on the clock.

Batches of 1,024 and 16,384 queries.  Legs of one session, three repeats each after a warm-up,
alternating on one handle, kernel ms from last_kernel_ms:
  exact k = 10 and k = 256 on today's path; k = 256 on the wide path (exact_wide_min_k 1);
  k = 512, 1024, 4096 on the wide path; the plain range search at each query's true k-th
  distance for k = 256, 1024, 4096 (the yardstick: the wide search was not handed the radius);
  the filtered wide search at 1 % allowed rows and k = 1024.
Per wide leg: hits / (B k), fallback queries, J, room, and the stage marks
(last_wide_{sample,radius,range}_ns of the first chunk of queries, last_wide_{emit,fallback}_ns
of the call).

Writes <out>/exact_wide.txt and .json.
Usage: python tools/wide_probe.py [--out profiles] [--nbase N] [--batches 1024,16384]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hnsw_amd as H  # noqa: E402
from bench import Searcher, gen_vectors  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
ap.add_argument("--nbase", type=int, default=1_000_000)
ap.add_argument("--batches", default="1024,16384")
args = ap.parse_args()

dev = torch.device("cuda")
n, d, REPS = args.nbase, 768, 3
batches = [int(b) for b in args.batches.split(",")]
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
QALL = gen_vectors(max(batches), d, 1234 + 7777, 12, 1000, dev, "cosine")
g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, build_mode=H.BUILD_FLAT, exact_wide=1)
g.reserve(n, d)
g.add_device(np.arange(n, dtype=np.int64), X.data_ptr(), n, d)
stream = torch.cuda.current_stream().cuda_stream
allowed = np.sort(np.random.default_rng(5).choice(n, n // 100, replace=False))
flt = g.Filter(allowed.tolist())
STAGES = ("sample", "radius", "range", "emit", "fallback")


def timed(fn):
    fn()
    torch.cuda.synchronize()
    return g.last_kernel_ms()


def wide_stats(B, k):
    return {"hits_per_k": g.get_option("last_wide_hits") / (B * k), "fallback_queries": g.get_option("last_wide_fallback_queries"),
            "J": g.get_option("last_wide_rank"), "room": g.get_option("last_wide_room"),
            **{f"{s}_ms": g.get_option(f"last_wide_{s}_ns") / 1e6 for s in STAGES}}


rows, lines = [], []
for B in batches:
    Q = QALL[:B].contiguous()
    S = {k: Searcher(g, B, k, d, dev) for k in (10, 256, 512, 1024, 4096)}
    fk, fd = torch.empty(B * 1024, dtype=torch.int64, device=dev), torch.empty(B * 1024, dtype=torch.float32, device=dev)
    fn_ = torch.empty(B, dtype=torch.int32, device=dev)

    def old(k):
        g.set_option("exact_wide_min_k", 257)
        S[k].run(Q, H.MODE_EXACT, 0)

    def wide(k):
        g.set_option("exact_wide_min_k", 1)
        S[k].run(Q, H.MODE_EXACT, 0)
        g.set_option("exact_wide_min_k", 257)

    def filtered():
        g.search_filtered_exact_device(Q.data_ptr(), B, d, 1024, flt, fk.data_ptr(), fd.data_ptr(), fn_.data_ptr(), stream=stream)

    # the true k-th distances, from the wide search itself
    radii = {}
    for k in (256, 1024, 4096):
        wide(k)
        torch.cuda.synchronize()
        radii[k] = S[k].dist.view(B, k)[:, k - 1].contiguous()
    cap = int(B * 4096 * 1.02) + 4096
    lims = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    rkeys, rdist = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.float32, device=dev)

    def rng_search(r):
        g.range_search_device(Q.data_ptr(), B, d, r.data_ptr(), cap, lims.data_ptr(), rkeys.data_ptr(), rdist.data_ptr(),
                              mode=H.MODE_EXACT, stream=stream)

    legs = {"top10": lambda: old(10), "top256": lambda: old(256), "wide256": lambda: wide(256), "wide512": lambda: wide(512),
            "wide1024": lambda: wide(1024), "wide4096": lambda: wide(4096), "filtered1pct_k1024": filtered}
    for k, r in radii.items():
        legs[f"range_at_k{k}"] = (lambda r=r: rng_search(r))
    for fn in legs.values():
        timed(fn)
    ms = {name: [] for name in legs}
    extra = {}
    for _ in range(REPS):
        for name, fn in legs.items():
            ms[name].append(timed(fn))
            if name.startswith("wide"):
                extra[name] = wide_stats(B, int(name[4:]))
            elif name.startswith("filtered"):
                extra[name] = wide_stats(B, 1024)
            elif name.startswith("range"):
                extra[name] = {"hits_per_query": int(lims[B].item()) / B,
                               "fallback_queries": g.get_option("last_range_fallback_queries")}
    g.device_status()
    med = {name: float(np.median(v)) for name, v in ms.items()}
    rows.append({"batch": B, "kernel_ms": {k_: [round(x, 3) for x in v] for k_, v in ms.items()},
                 "kernel_ms_median": {k_: round(v, 3) for k_, v in med.items()}, "legs": extra})
    lines.append(f"batch {B:5d}: today's path: exact top-10 {med['top10']:9.3f} ms, exact k=256 {med['top256']:9.3f} ms")
    for name in legs:
        if name.startswith("wide") or name.startswith("filtered"):
            x = extra[name]
            lines.append(f"batch {B:5d}: {name:19s} {med[name]:9.3f} ms; J {x['J']}, room {x['room']}, hits / (B k) "
                         f"{x['hits_per_k']:.3f}, {x['fallback_queries']} fallback queries; first chunk: sample "
                         f"{x['sample_ms']:.3f}, radius {x['radius_ms']:.3f}, range stages {x['range_ms']:.3f}; call: sort + cut "
                         f"{x['emit_ms']:.3f}, fallback {x['fallback_ms']:.3f}")
        elif name.startswith("range"):
            x = extra[name]
            lines.append(f"batch {B:5d}: {name:19s} {med[name]:9.3f} ms (range search handed the true k-th distance; "
                         f"{x['hits_per_query']:.1f} hits per query, {x['fallback_queries']} swept queries)")
    for line in lines[-(len(legs)):]:
        print(line, flush=True)
    del S

os.makedirs(args.out, exist_ok=True)
head = (f"wide exact search, {n} x {d} cosine rows (bench.py's vectors, flat index: the exact path reads no graph); kernel ms "
        f"are last_kernel_ms medians of {REPS} repeats after one warm-up, the legs alternating on one handle in one session; "
        f"exact_sample at its default (64)")
with open(os.path.join(args.out, "exact_wide.txt"), "w") as fh:
    fh.write(head + "\n" + "\n".join(lines) + "\n")
with open(os.path.join(args.out, "exact_wide.json"), "w") as fh:
    json.dump({"what": head, "rows": rows}, fh, indent=1)
flt.close()
g.close()
