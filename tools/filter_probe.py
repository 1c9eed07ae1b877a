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

--leg exact: the filtered exact search (mhnsw_search_filtered_exact_device) on the
same index, batches and k, random filters of 100 / 50 / 10 / 1 / 0.1 % of the rows.
Per selectivity, warmed and alternating in one session: the exact call's kernel ms
(compaction through re-rank) with its stage split (compaction, gather, and of the
first query chunk scores + selection, re-rank, fallback), its uncertified queries
and its recall@10 against the masked fp32 brute force; the filtered walk at the
route the walk's table uses for that selectivity (256 / 256 / 1024 / 2048 / 2048)
with its recall and its queries below k; and the unfiltered MODE_EXACT search, the
ceiling of the 100 % case.  --bench-lines FILE: lines copied into the write-up (the
parent's and this tree's bench.py result lines).  Writes <out>/filtered_exact.txt and
.json.
Usage: python tools/filter_probe.py [--leg walk|exact] [--out profiles]"""
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
ap.add_argument("--leg", choices=["walk", "exact"], default="walk")
ap.add_argument("--bench-lines", default=None)
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


def exact_leg():
    rows, lines = [], []
    rng = np.random.default_rng(99)
    plain = Searcher(g, B, K, d, dev)
    stages = ("compact", "gather", "select", "rerank", "fallback")

    def unfiltered():
        plain.run(Q, H.MODE_EXACT, 0)
        torch.cuda.synchronize()
        return g.last_kernel_ms()

    for pct, W in ((100, 256), (50, 256), (10, 1024), (1, 2048), (0.1, 2048)):
        allowed_h = np.ones(n, bool) if pct == 100 else rng.random(n) < pct / 100.0
        allowed = torch.tensor(allowed_h, device=dev)
        f = g.Filter(np.flatnonzero(allowed_h))
        fo = torch.full((B,), f.id, dtype=torch.int32, device=dev)
        truth = masked_truth(allowed)

        def exact():
            g.search_filtered_exact_device(Q.data_ptr(), B, d, K, f, ok.data_ptr(), od.data_ptr(), on.data_ptr(),
                                           stream=stream)
            torch.cuda.synchronize()
            return g.last_kernel_ms(), [g.get_option(f"last_fx_{s}_ns") / 1e6 for s in stages]

        exact(), filtered(fo, W), unfiltered()
        e_ms, e_st, w_ms, u_ms = [], [], [], []
        for _ in range(REPS):
            ms, st = exact()
            e_ms.append(ms)
            e_st.append(st)
            w_ms.append(filtered(fo, W))
            u_ms.append(unfiltered())
        g.device_status()
        w_keys = torch.where(torch.arange(K, device=dev)[None, :] < on[:, None], ok, torch.full_like(ok, -1))
        w_recall, w_below = recall(w_keys, truth), int((on.cpu().numpy() < K).sum())
        g.reset_stats()
        exact()
        g.device_status()
        uncert = g.stats()["exact_uncertified"]
        e_keys = torch.where(torch.arange(K, device=dev)[None, :] < on[:, None], ok, torch.full_like(ok, -1))
        st = np.median(np.asarray(e_st), axis=0)
        med = float(np.median(e_ms))
        row = {"allowed_pct": pct, "allowed_rows": int(allowed_h.sum()), "exact_kernel_ms": [round(x, 3) for x in e_ms],
               "exact_kernel_ms_median": round(med, 3),
               "compaction_ms": round(float(st[0]), 3), "gather_ms": round(float(st[1]), 3),
               "pipeline_ms": round(med - float(st[0]) - float(st[1]), 3),
               "first_chunk_scores_selection_ms": round(float(st[2]), 3), "first_chunk_rerank_ms": round(float(st[3]), 3),
               "first_chunk_fallback_ms": round(float(st[4]), 3), "uncertified_queries": int(uncert),
               "exact_recall_at_10": round(recall(e_keys, truth), 4), "exact_queries_below_k": int((on.cpu().numpy() < K).sum()),
               "walk_route": W, "walk_kernel_ms": [round(x, 3) for x in w_ms],
               "walk_kernel_ms_median": round(float(np.median(w_ms)), 3), "walk_recall_at_10": round(w_recall, 4),
               "walk_queries_below_k": w_below, "unfiltered_exact_kernel_ms": [round(x, 3) for x in u_ms],
               "unfiltered_exact_kernel_ms_median": round(float(np.median(u_ms)), 3)}
        rows.append(row)
        lines.append(f"allowed {pct:5} % ({row['allowed_rows']:7d} rows): exact {row['exact_kernel_ms_median']:8.3f} ms/batch "
                     f"= compaction {row['compaction_ms']:.3f} + gather {row['gather_ms']:.3f} + pipeline "
                     f"{row['pipeline_ms']:.3f} (first chunk: scores + selection {row['first_chunk_scores_selection_ms']:.3f}, "
                     f"re-rank {row['first_chunk_rerank_ms']:.3f}, fallback {row['first_chunk_fallback_ms']:.3f}), "
                     f"{uncert} uncertified, recall@10 {row['exact_recall_at_10']:.4f} | walk route {W}: "
                     f"{row['walk_kernel_ms_median']:8.3f} ms/batch, recall@10 {w_recall:.4f}, {w_below} below k | "
                     f"unfiltered exact {row['unfiltered_exact_kernel_ms_median']:8.3f} ms/batch")
        print(lines[-1], flush=True)
        f.close()
    os.makedirs(args.out, exist_ok=True)
    head = (f"filtered exact search, bench index {n} x {d} cosine, batches of {B}, k {K}; kernel ms are last_kernel_ms "
            f"medians of {REPS} repeats after one warm-up, the exact call, the filtered walk (ef {EF}) and the unfiltered "
            f"exact search alternating; stage times from HIP events (options last_fx_*_ns); recall over the first {NGT} "
            f"queries against a masked fp32 brute force")
    bench = open(args.bench_lines).read().splitlines() if args.bench_lines else []
    with open(os.path.join(args.out, "filtered_exact.txt"), "w") as fh:
        fh.write(head + "\n" + "\n".join(lines + bench) + "\n")
    with open(os.path.join(args.out, "filtered_exact.json"), "w") as fh:
        json.dump({"what": head, "rows": rows, "bench_lines": bench}, fh, indent=1)


if args.leg == "exact":
    exact_leg()
    g.close()
    sys.exit(0)

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
