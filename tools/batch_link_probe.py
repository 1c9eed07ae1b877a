#!/usr/bin/env python3
"""Build rate and graph quality of the batched insert with and without the link
pass (option batch_link), on bench.py's index: its data generator and its build
recipe (1M x 768 cosine, efConstruction 400, M0 40, upper_efc 128, build_expand 4,
batches of 20 % of the index).  Not a test and not the benchmark.

Prints one JSON line per value of batch_link: inserts/s of every repeat (a
small build warms the kernels up first) and their median, and of the last
repeat the build kernel time (stats build_search_us, time_build), the link
kernels' device time (last_link_ns), recall@10 at ef 64 against the exact mode
on --queries fresh queries, the share of --queries stored rows that find their
own key at ef 64, and the dropped proposals.

    python tools/batch_link_probe.py [--links 0,1] [--repeats 3] [--nbase 1000000]

MHNSW_LIB=<another build of the library> measures that build (a library without
the option runs --links 0 only).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import hnsw_amd as H  # noqa: E402


def recipe():
    """bench.py's defaults (its parse() on an empty command line)"""
    argv, sys.argv = sys.argv, [sys.argv[0]]
    try:
        return bench.parse()
    finally:
        sys.argv = argv


def build(a, device, nrows, link):
    X = bench.gen_vectors(nrows, a.dim, a.seed, a.intrinsic, a.clusters, device, a.metric)
    g = H.Graph(M=a.M, Ml=0.25, EfSearch=a.ef, Distance=H.CosineDistance, Rng=1, build_mode=H.BUILD_BATCH,
                m0=a.M0, ef_construction=a.efc, heuristic=2, keep_pruned=a.keep_pruned, prune_alpha_pct=a.alpha,
                build_expand=a.build_expand, batch_ratio_pct=a.batch_ratio, upper_efc=a.upper_efc,
                screen=a.screen, time_build=1)
    if link:
        g.set_option("batch_link", 1)
    g.reserve(nrows, a.dim)
    keys = np.arange(nrows, dtype=np.int64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.add_device(keys, X.data_ptr(), nrows, a.dim)
    torch.cuda.synchronize()
    return g, X, time.perf_counter() - t0


def quality(a, g, X, device, nq):
    s = bench.Searcher(g, nq, a.k, a.dim, device)
    Q = bench.gen_vectors(nq, a.dim, a.seed + 7_777, a.intrinsic, a.clusters, device, a.metric)
    tk, _, tn = (x.clone() for x in s.run(Q, H.MODE_EXACT, 0))
    bk, _, bn = s.run(Q, H.MODE_BEAM, 64)
    torch.cuda.synchronize()
    recall = bench.recall_at_k(bk, bn, tk, tn, a.k)
    rows = torch.from_numpy(np.random.default_rng(3).choice(X.shape[0], nq, replace=False)).to(device)
    sk, _, sn = s.run(X[rows].contiguous(), H.MODE_BEAM, 64)
    torch.cuda.synchronize()
    own = float(((sn > 0) & (sk[:, 0] == rows)).float().mean())
    return recall, own


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--links", default="0,1")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--nbase", type=int, default=1_000_000)
    p.add_argument("--queries", type=int, default=4096)
    p.add_argument("--warm-rows", type=int, default=100_000)
    o = p.parse_args()
    a = recipe()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    for link in (int(x) for x in o.links.split(",")):
        g, X, _ = build(a, device, min(o.warm_rows, o.nbase), link)  # warm-up: code objects, allocator
        g.close()
        del X
        rates = []
        for rep in range(o.repeats):
            g, X, dt = build(a, device, o.nbase, link)
            rates.append(o.nbase / dt)
            if rep + 1 < o.repeats:
                g.close()
                del X
        st = g.stats()
        recall, own = quality(a, g, X, device, o.queries)
        try:
            link_ns, link_rows, link_edges = (g.get_option(f"last_link_{x}") for x in ("ns", "rows", "edges"))
        except H.HnswError:  # a library from before the option
            link_ns = link_rows = link_edges = None
        print(json.dumps({
            "batch_link": link, "lib": os.path.basename(os.path.dirname(H._lib.LIB_PATH)) + "/" +
            os.path.basename(H._lib.LIB_PATH), "n": o.nbase, "dim": a.dim, "efc": a.efc, "m0": a.M0,
            "upper_efc": a.upper_efc, "build_expand": a.build_expand, "batch_ratio_pct": a.batch_ratio,
            "inserts_per_s": [round(r) for r in rates], "inserts_per_s_median": round(float(np.median(rates))),
            "build_kernel_us": st["build_search_us"], "last_link_ns": link_ns, "last_link_rows": link_rows,
            "last_link_edges": link_edges, "recall_at_10_ef64": round(recall, 4), "self_recall_ef64": round(own, 4),
            "queries": o.queries, "dropped_proposals": st["dropped_proposals"]}), flush=True)
        g.close()
        del X


if __name__ == "__main__":
    main()
