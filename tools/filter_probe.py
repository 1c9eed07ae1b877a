"""Filtered beam search on the bench index (1M x 768 cosine, built as bench.py
builds it): batches of 16,384 queries at ef 64, k 10, random filters of 100 / 50 /
10 / 1 % of the rows, route widths 256 / 1024 / 2048.

Per filter and route width: kernel ms per batch (last_kernel_ms; warmed, three
repeats alternating with the comparison), expansions and f32 / fp16 rows per
query, recall@10 against a masked fp32 brute force in torch (the first 2,048
queries), and the queries that return fewer than k.  Next to each, what a
caller had to do before: the unfiltered beam search at k = ef = W with the
lists filtered afterwards (here on the device; a caller would copy B x W results
to the host first), its kernel ms and its recall after filtering.

Writes <out>/filtered_search.txt and .json.
Usage: python tools/filter_probe.py [--out profiles]"""
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
ap.add_argument("--batch", type=int, default=16384)
args = ap.parse_args()

dev = torch.device("cuda")
n, d, B, EF, K, NGT, REPS = args.nbase, 768, args.batch, 64, 10, 2048, 3
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
Q = gen_vectors(B, d, 1234 + 7777, 12, 1000, dev, "cosine")
g = H.Graph(M=16, Ml=0.25, EfSearch=EF, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=40,
            ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4, batch_ratio_pct=20,
            upper_efc=128, screen=1)
g.reserve(n, d)
g.add_device(np.arange(n, dtype=np.int64), X.data_ptr(), n, d)


def masked_truth(allowed):
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
    return best_i


def recall(keys, truth):
    keys, truth = keys[:NGT].cpu().numpy(), truth.cpu().numpy()
    tot = 0.0
    for b in range(NGT):
        t = set(truth[b][truth[b] >= 0].tolist())
        tot += len(set(keys[b][keys[b] >= 0].tolist()) & t) / max(1, len(t))
    return tot / NGT


ok = torch.empty(B, K, dtype=torch.int64, device=dev)
od = torch.empty(B, K, dtype=torch.float32, device=dev)
on = torch.empty(B, dtype=torch.int32, device=dev)
stream = torch.cuda.current_stream().cuda_stream


def filtered(fo, W):
    g.search_filtered_device(Q.data_ptr(), B, d, K, fo.data_ptr(), ok.data_ptr(), od.data_ptr(), on.data_ptr(), ef=EF,
                             route=W, stream=stream)
    torch.cuda.synchronize()
    return g.last_kernel_ms()


rows, lines = [], []
rng = np.random.default_rng(99)
for pct in (100, 50, 10, 1):
    allowed_h = np.ones(n, bool) if pct == 100 else rng.random(n) < pct / 100.0
    allowed = torch.tensor(allowed_h, device=dev)
    f = g.Filter(np.flatnonzero(allowed_h))
    fo = torch.full((B,), f.id, dtype=torch.int32, device=dev)
    truth = masked_truth(allowed)
    for W in (256, 1024, 2048):
        wide = Searcher(g, B, W, d, dev)

        def today():
            wide.run(Q, H.MODE_BEAM, W)
            torch.cuda.synchronize()
            return g.last_kernel_ms()

        filtered(fo, W)
        today()
        f_ms, t_ms = [], []
        for _ in range(REPS):
            f_ms.append(filtered(fo, W))
            t_ms.append(today())
        g.reset_stats()
        filtered(fo, W)
        g.device_status()
        st = g.stats()
        nn = on.cpu().numpy()
        keys = torch.where(torch.arange(K, device=dev)[None, :] < on[:, None], ok, torch.full_like(ok, -1))
        # the caller's host filter, done here on the device: the first K allowed keys of each wide list
        wk = torch.where(torch.arange(W, device=dev)[None, :] < wide.n[:, None], wide.keys, torch.zeros_like(wide.keys))
        hit = allowed[wk] & (torch.arange(W, device=dev)[None, :] < wide.n[:, None])
        rank = torch.cumsum(hit.long(), 1)
        sel = hit & (rank <= K)
        tk = torch.full((B, K), -1, dtype=torch.int64, device=dev)
        bi, wi = sel.nonzero(as_tuple=True)
        tk[bi, rank[bi, wi] - 1] = wk[bi, wi]
        row = {"allowed_pct": pct, "route": W, "filtered_kernel_ms": [round(x, 3) for x in f_ms],
               "filtered_kernel_ms_median": round(float(np.median(f_ms)), 3),
               "expansions_per_query": round(st["search_expansions"] / B, 1),
               "f32_rows_per_query": round(st["search_f32_evals"] / B, 1),
               "fp16_rows_per_query": round(st["search_screened"] / B, 1) if "search_screened" in st else None,
               "recall_at_10": round(recall(keys, truth), 4), "queries_below_k": int((nn < K).sum()),
               "unfiltered_k_ef_W_kernel_ms": [round(x, 3) for x in t_ms],
               "unfiltered_k_ef_W_kernel_ms_median": round(float(np.median(t_ms)), 3),
               "unfiltered_then_host_filter_recall_at_10": round(recall(tk, truth), 4),
               "unfiltered_then_host_filter_below_k": int((sel.sum(1) < K).sum().item())}
        rows.append(row)
        lines.append(f"allowed {pct:3d} %  W {W:4d}: filtered {row['filtered_kernel_ms_median']:8.3f} ms/batch, "
                     f"{row['expansions_per_query']:7.1f} expansions, {row['f32_rows_per_query']:7.1f} f32 rows, "
                     f"{row['fp16_rows_per_query']} fp16 rows per query, recall@10 {row['recall_at_10']:.4f}, "
                     f"{row['queries_below_k']} queries below k | unfiltered k=ef=W "
                     f"{row['unfiltered_k_ef_W_kernel_ms_median']:8.3f} ms/batch, recall@10 after filtering "
                     f"{row['unfiltered_then_host_filter_recall_at_10']:.4f}, "
                     f"{row['unfiltered_then_host_filter_below_k']} below k")
        print(lines[-1], flush=True)
        del wide
    f.close()

os.makedirs(args.out, exist_ok=True)
head = (f"filtered beam search, bench index {n} x {d} cosine, batches of {B}, ef {EF}, k {K}; kernel ms are "
        f"last_kernel_ms medians of {REPS} alternating repeats after one warm-up; recall over the first {NGT} queries "
        f"against a masked fp32 brute force")
with open(os.path.join(args.out, "filtered_search.txt"), "w") as fh:
    fh.write(head + "\n" + "\n".join(lines) + "\n")
with open(os.path.join(args.out, "filtered_search.json"), "w") as fh:
    json.dump({"what": head, "rows": rows}, fh, indent=1)
g.close()
