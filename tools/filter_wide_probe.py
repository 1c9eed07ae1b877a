"""Filtered beam search past 128 results (option "filter_wide") on the bench index
(1M x 768 cosine, built as bench.py builds it): batches of 16,384 queries, route
2048, random filters of 100 / 50 / 10 / 1 % of the rows, k = ef in 128 / 256 / 512 /
1024 / 2048.  The k = ef = 128 leg is the narrow kernel (k_search_beam_filt),
the in-session yardstick; the others are k_search_beam_filt_wide.

Per filter and width: the walk's kernel ms per batch (last_kernel_ms; one
warm-up, then three repeats alternating with the comparison), expansions per
query, recall@k against a masked fp32 brute force in torch (the first 256
queries) and the queries that return fewer than k; next to it the filtered exact
search at the same k (exact_wide past k 256), its kernel ms and recall.  Once
per session: the other route a caller had, the unfiltered beam search at k = ef
= 2048 and the copy of its 16,384 x 2048 keys and distances to pinned host
memory (device events around the two copies).

Writes <out>/filtered_wide.txt.
Usage: python tools/filter_wide_probe.py [--out profiles] [--nbase N] [--batch B]"""
import argparse
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
ap.add_argument("--batch", type=int, default=16384)
args = ap.parse_args()

dev = torch.device("cuda")
n, d, B, W, NGT, REPS = args.nbase, 768, args.batch, 2048, 256, 3
KS = (128, 256, 512, 1024, 2048)
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
Q = gen_vectors(B, d, 1234 + 7777, 12, 1000, dev, "cosine")
g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=40,
            ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4, batch_ratio_pct=20,
            upper_efc=128, screen=1, filter_wide=1, exact_wide=1)
g.reserve(n, d)
g.add_device(np.arange(n, dtype=np.int64), X.data_ptr(), n, d)
stream = torch.cuda.current_stream().cuda_stream


def masked_truth(allowed, K):
    """exact top-K among the allowed rows for the first NGT queries: fp32 scores in row chunks"""
    best_s = torch.full((NGT, K), -float("inf"), device=dev)
    best_i = torch.full((NGT, K), -1, dtype=torch.int64, device=dev)
    for lo in range(0, n, 1 << 17):
        hi = min(n, lo + (1 << 17))
        s = Q[:NGT] @ X[lo:hi].T  # (rows are unit vectors: cosine distance orders as -score)
        s.masked_fill_(~allowed[lo:hi][None, :], -float("inf"))
        cs, ci = s.topk(min(K, hi - lo), dim=1)
        ms, mi = torch.cat([best_s, cs], 1).topk(K, dim=1)
        best_i = torch.gather(torch.cat([best_i, ci + lo], 1), 1, mi)
        best_s = ms
    best_i[torch.isinf(best_s)] = -1
    return best_i.cpu().numpy()


def recall(keys, cnt, truth, K):
    keys, cnt = keys[:NGT].cpu().numpy(), cnt[:NGT].cpu().numpy()
    tot = 0.0
    for b in range(NGT):
        t = set(truth[b, :K][truth[b, :K] >= 0].tolist())
        tot += len(set(keys[b, : cnt[b]].tolist()) & t) / max(1, len(t))
    return tot / NGT


def med(v):
    return round(float(np.median(v)), 3)


rows, lines = [], []
# the caller's other route, once: unfiltered k = ef = 2048 and its results over PCIe
plain = Searcher(g, B, W, d, dev)
hk = torch.empty(B, W, dtype=torch.int64).pin_memory()
hd = torch.empty(B, W, dtype=torch.float32).pin_memory()
u_ms, c_ms = [], []
for rep in range(REPS + 1):
    plain.run(Q, H.MODE_BEAM, W)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hk.copy_(plain.keys, non_blocking=True)
    hd.copy_(plain.dist, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    if rep:
        u_ms.append(g.last_kernel_ms())
        c_ms.append(e0.elapsed_time(e1))
unfiltered = {"unfiltered_k_ef_2048_kernel_ms": [round(x, 3) for x in u_ms], "unfiltered_kernel_ms_median": med(u_ms),
              "copy_to_pinned_host_ms": [round(x, 3) for x in c_ms], "copy_ms_median": med(c_ms)}
lines.append(f"unfiltered beam k = ef = {W}: {unfiltered['unfiltered_kernel_ms_median']:9.3f} ms/batch kernel + "
             f"{unfiltered['copy_ms_median']:8.3f} ms device-to-host copy of {B} x {W} keys and distances "
             f"(the host filter over them not included)")
print(lines[-1], flush=True)
del plain, hk, hd

rng = np.random.default_rng(99)
for pct in (100, 50, 10, 1):
    allowed_h = np.ones(n, bool) if pct == 100 else rng.random(n) < pct / 100.0
    allowed = torch.tensor(allowed_h, device=dev)
    f = g.Filter(np.flatnonzero(allowed_h))
    fo = torch.full((B,), f.id, dtype=torch.int32, device=dev)
    truth = masked_truth(allowed, max(KS))
    for K in KS:
        ok = torch.empty(B, K, dtype=torch.int64, device=dev)
        od = torch.empty(B, K, dtype=torch.float32, device=dev)
        on = torch.empty(B, dtype=torch.int32, device=dev)

        def walk():
            g.search_filtered_device(Q.data_ptr(), B, d, K, fo.data_ptr(), ok.data_ptr(), od.data_ptr(), on.data_ptr(),
                                     ef=K, route=W, stream=stream)
            torch.cuda.synchronize()
            return g.last_kernel_ms()

        def exact():
            g.search_filtered_exact_device(Q.data_ptr(), B, d, K, f, ok.data_ptr(), od.data_ptr(), on.data_ptr(),
                                           stream=stream)
            torch.cuda.synchronize()
            return g.last_kernel_ms()

        walk(), exact()
        w_ms, x_ms = [], []
        for _ in range(REPS):
            x_ms.append(exact())
            w_ms.append(walk())
        exact()
        g.device_status()
        x_recall, x_below = recall(ok, on, truth, K), int((on.cpu().numpy() < K).sum())
        g.reset_stats()
        walk()
        g.device_status()
        row = {"allowed_pct": pct, "k_ef": K, "route": W, "kernel": "k_search_beam_filt" + ("" if K <= 128 else "_wide"),
               "walk_kernel_ms": [round(x, 3) for x in w_ms], "walk_kernel_ms_median": med(w_ms),
               "expansions_per_query": round(g.stats()["search_expansions"] / B, 1),
               "walk_recall_at_k": round(recall(ok, on, truth, K), 4), "walk_queries_below_k": int((on.cpu().numpy() < K).sum()),
               "exact_kernel_ms": [round(x, 3) for x in x_ms], "exact_kernel_ms_median": med(x_ms),
               "exact_recall_at_k": round(x_recall, 4), "exact_queries_below_k": x_below}
        rows.append(row)
        lines.append(f"allowed {pct:3d} %  k = ef {K:4d} ({row['kernel']}): walk {row['walk_kernel_ms_median']:9.3f} ms/batch, "
                     f"{row['expansions_per_query']:7.1f} expansions per query, recall@k {row['walk_recall_at_k']:.4f}, "
                     f"{row['walk_queries_below_k']} queries below k | filtered exact {row['exact_kernel_ms_median']:9.3f} "
                     f"ms/batch, recall@k {row['exact_recall_at_k']:.4f}, {x_below} below k")
        print(lines[-1], flush=True)
    f.close()

os.makedirs(args.out, exist_ok=True)
head = (f"filtered beam search past 128 results, bench index {n} x {d} cosine, batches of {B}, route {W}, k = ef; kernel "
        f"ms are last_kernel_ms medians of {REPS} repeats after one warm-up, the walk and the filtered exact search "
        f"alternating; recall over the first {NGT} queries against a masked fp32 brute force")
with open(os.path.join(args.out, "filtered_wide.txt"), "w") as fh:
    fh.write(head + "\n" + "\n".join(lines) + "\n")
g.close()
