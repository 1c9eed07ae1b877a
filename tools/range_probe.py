"""Range search on the bench index (1M x 768 cosine, built as bench.py builds it).

Batches of 1,024 and 16,384 queries; per-query radii at which 10, 100 and 1,000 rows are
expected: the 10th and 100th distances of the exact search at k = 256, and the 1,000th
distance of an fp32 brute force in torch (the exact search stops at k = 256).

Legs of one session, three repeats each after a warm-up, alternating on one handle, kernel
ms from last_kernel_ms: the exact top-10 search (with its fused GEMM, last_gemm_ns), the
exact search at k = 256 (what a caller had before), and the exact-mode range search at
each radius with its hits, last_range_candidates, last_range_fallback_queries and stage
marks (last_range_{filter,refine,sweep}_ns of the first chunk of queries, last_range_order_ns
of the call).  Yardstick: at 10 expected hits the range search may exceed the top-10 search
by that search's own non-GEMM share (top-10 ms - GEMM ms of its first chunk x chunks).

Beam leg: range search in beam mode at ef 64 and 256 and the 10-hit radius against the plain
beam search at k = ef, and the fraction of the exact hits it finds (first 2,048 queries).

Writes <out>/range_search.txt and .json.
Usage: python tools/range_probe.py [--out profiles] [--nbase N]"""
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
args = ap.parse_args()

dev = torch.device("cuda")
n, d, BMAX, REPS, NFRAC = args.nbase, 768, 16384, 3, 2048
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
QALL = gen_vectors(BMAX, d, 1234 + 7777, 12, 1000, dev, "cosine")
g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=40,
            ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4, batch_ratio_pct=20,
            upper_efc=128, screen=1)
g.reserve(n, d)
g.add_device(np.arange(n, dtype=np.int64), X.data_ptr(), n, d)
stream = torch.cuda.current_stream().cuda_stream


def kth_distance(Q, k):
    """per query the k-th smallest fp32 cosine distance (rows and queries are unit vectors)"""
    out = torch.empty(len(Q), device=dev)
    for q0 in range(0, len(Q), 2048):
        best = torch.full((min(2048, len(Q) - q0), k), -float("inf"), device=dev)
        for lo in range(0, n, 1 << 17):
            s = Q[q0:q0 + 2048] @ X[lo:lo + (1 << 17)].T
            best = torch.cat([best, s.topk(min(k, s.shape[1]), dim=1).values], 1).topk(k, dim=1).values
        out[q0:q0 + 2048] = 1.0 - best[:, -1]
    return out


def timed(fn):
    fn()
    torch.cuda.synchronize()
    return g.last_kernel_ms()


rows, lines = [], []
for B in (1024, BMAX):
    Q = QALL[:B].contiguous()
    top10, top256 = Searcher(g, B, 10, d, dev), Searcher(g, B, 256, d, dev)
    top256.run(Q, H.MODE_EXACT, 0)
    torch.cuda.synchronize()
    radii = {10: top256.dist[:, 9].contiguous(), 100: top256.dist[:, 99].contiguous(), 1000: kth_distance(Q, 1000)}
    lims = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    cap = int(B * 1000 * 1.2) + 4096
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    dist = torch.empty(cap, dtype=torch.float32, device=dev)

    def rng_search(r, mode=H.MODE_EXACT, ef=0):
        g.range_search_device(Q.data_ptr(), B, d, r.data_ptr(), cap, lims.data_ptr(), keys.data_ptr(), dist.data_ptr(),
                              mode=mode, ef=ef, stream=stream)

    legs = {"top10": lambda: top10.run(Q, H.MODE_EXACT, 0), "top256": lambda: top256.run(Q, H.MODE_EXACT, 0)}
    for e, r in radii.items():
        legs[f"range{e}"] = (lambda r=r: rng_search(r))
    for fn in legs.values():
        timed(fn)
    ms = {name: [] for name in legs}
    extra = {}
    for _ in range(REPS):
        for name, fn in legs.items():
            ms[name].append(timed(fn))
            if name == "top10":
                extra["top10_gemm_first_chunk_ms"] = g.get_option("last_gemm_ns") / 1e6
            if name.startswith("range"):
                extra[name] = {"hits": int(lims[B].item()), "candidates": g.get_option("last_range_candidates"),
                               "fallback_queries": g.get_option("last_range_fallback_queries"),
                               "gemm_first_chunk_ms": g.get_option("last_gemm_ns") / 1e6,
                               **{f"{s}_ms": g.get_option(f"last_range_{s}_ns") / 1e6
                                  for s in ("filter", "refine", "sweep", "order")}}
    g.device_status()
    # the exact path runs a batch in chunks of at most 4,096 queries within its 4 GiB score budget
    qc = min(B, 4096, (4 << 30) // (((n + 255) // 256 * 256) * 4))
    chunks = -(-B // qc)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    share = med["top10"] - extra["top10_gemm_first_chunk_ms"] * B / qc
    row = {"batch": B, "chunks": chunks, "kernel_ms": {k_: [round(x, 3) for x in v] for k_, v in ms.items()},
           "kernel_ms_median": {k_: round(v, 3) for k_, v in med.items()},
           "top10_gemm_first_chunk_ms": round(extra["top10_gemm_first_chunk_ms"], 3),
           "top10_non_gemm_share_ms": round(share, 3),
           "range10_minus_top10_ms": round(med["range10"] - med["top10"], 3),
           "range": {k_: v for k_, v in extra.items() if k_.startswith("range")}}
    lines.append(f"batch {B:5d}: exact top-10 {med['top10']:8.3f} ms (GEMM of its first chunk "
                 f"{row['top10_gemm_first_chunk_ms']:.3f} ms, non-GEMM share of the call {share:.3f} ms), exact k=256 "
                 f"{med['top256']:8.3f} ms")
    for e in radii:
        x = extra[f"range{e}"]
        lines.append(f"batch {B:5d}: range search, {e:4d} expected hits: {med[f'range{e}']:8.3f} ms, "
                     f"{x['hits'] / B:8.1f} hits and {x['candidates'] / B:8.1f} candidates per query, "
                     f"{x['fallback_queries']} fallback queries; first chunk: filter {x['filter_ms']:.3f} "
                     f"(GEMM {x['gemm_first_chunk_ms']:.3f}), refine {x['refine_ms']:.3f}, sweep + prefix + gather "
                     f"{x['sweep_ms']:.3f}; call: order {x['order_ms']:.3f}")
    lines.append(f"batch {B:5d}: range search at 10 hits - top-10 = {row['range10_minus_top10_ms']:.3f} ms against the "
                 f"allowed {share:.3f} ms: {'within' if row['range10_minus_top10_ms'] <= share else 'EXCEEDS'}")
    # beam leg at the 10-hit radius
    rng_search(radii[10])
    torch.cuda.synchronize()
    el = lims.cpu().numpy().copy()
    ek = keys[: el[-1]].cpu().numpy().copy()
    row["beam"] = {}
    for ef in (64, 256):
        plain = Searcher(g, B, ef, d, dev)
        pm, bm = [], []
        timed(lambda: plain.run(Q, H.MODE_BEAM, ef)), timed(lambda: rng_search(radii[10], H.MODE_BEAM, ef))
        for _ in range(REPS):
            pm.append(timed(lambda: plain.run(Q, H.MODE_BEAM, ef)))
            bm.append(timed(lambda: rng_search(radii[10], H.MODE_BEAM, ef)))
        bl = lims.cpu().numpy()
        bk = keys[: bl[-1]].cpu().numpy()
        nf = min(B, NFRAC)
        found = sum(len(set(bk[bl[b]:bl[b + 1]].tolist()) & set(ek[el[b]:el[b + 1]].tolist())) for b in range(nf))
        frac = found / max(1, int(el[nf]))
        full = int((np.diff(bl) == ef).sum())
        row["beam"][ef] = {"plain_beam_ms": [round(x, 3) for x in pm], "range_beam_ms": [round(x, 3) for x in bm],
                           "fraction_of_exact_hits": round(frac, 4), "queries_with_count_ef": full}
        lines.append(f"batch {B:5d}: beam mode ef {ef:3d} at the 10-hit radius: {np.median(bm):8.3f} ms against the plain "
                     f"beam search at k = ef {np.median(pm):8.3f} ms; {frac:.4f} of the exact hits found (first {nf} "
                     f"queries), {full} queries with a count of ef")
        del plain
    rows.append(row)
    for line in lines[-7:]:
        print(line, flush=True)

os.makedirs(args.out, exist_ok=True)
head = (f"range search, bench index {n} x {d} cosine; kernel ms are last_kernel_ms medians of {REPS} repeats after one "
        f"warm-up, the legs alternating on one handle in one session; range_expect at its default (64); radii: the "
        f"exact search's 10th / 100th distances, an fp32 brute force's 1,000th")
with open(os.path.join(args.out, "range_search.txt"), "w") as fh:
    fh.write(head + "\n" + "\n".join(lines) + "\n")
with open(os.path.join(args.out, "range_search.json"), "w") as fh:
    json.dump({"what": head, "rows": rows}, fh, indent=1)
g.close()
