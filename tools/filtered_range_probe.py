"""Filtered range search on the bench index (1M x 768 cosine, built as bench.py builds it):
the sibling of tools/range_probe.py, with its conventions.

Batches of 1,024 and 16,384 queries; random filters that allow 100 / 10 / 1 / 0.1 % of the
rows; per-query radii at the 10th and 100th allowed distance (the filtered exact search's at
k = 256).  Legs of one session, three repeats each after a warm-up, alternating on one handle,
kernel ms from last_kernel_ms: the filtered range search at each radius (hits, candidates per
hit, fallback queries, the stage marks of its first chunk of queries and the row set's
compaction and gather), and next to it what it replaces or resembles -- the plain range search
at the same radius (only where it expects at most 1,000 hits per query: below that the
unfiltered sweep of 16,384 queries is minutes), the filtered exact top-10 and the filtered
exact search at k = 256.

--control: only the plain legs (exact top-10, plain range search at 10 and 100 hits) of one
library, for runs that alternate the parent commit's tree and this one (--root).

Writes <out>/filtered_range.txt and .json (appends the control lines when --control).
Usage: python tools/filtered_range_probe.py [--out profiles] [--nbase N] [--control NAME --root DIR]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument("--out", default=os.path.join(here, "profiles"))
ap.add_argument("--nbase", type=int, default=1_000_000)
ap.add_argument("--control", default="")
ap.add_argument("--root", default=here)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hnsw_amd as H  # noqa: E402
from bench import Searcher, gen_vectors  # noqa: E402

dev = torch.device("cuda")
n, d, BMAX, REPS = args.nbase, 768, 16384, 3
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
QALL = gen_vectors(BMAX, d, 1234 + 7777, 12, 1000, dev, "cosine")
g = H.Graph(M=16, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=40,
            ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4, batch_ratio_pct=20,
            upper_efc=128, screen=1)
g.reserve(n, d)
g.add_device(np.arange(n, dtype=np.int64), X.data_ptr(), n, d)
stream = torch.cuda.current_stream().cuda_stream
os.makedirs(args.out, exist_ok=True)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    return g.last_kernel_ms()


def run_legs(legs, after=None):
    """one warm-up of every leg, then REPS alternating rounds -> {leg: [ms]}"""
    for fn in legs.values():
        timed(fn)
    ms = {name: [] for name in legs}
    for _ in range(REPS):
        for name, fn in legs.items():
            ms[name].append(round(timed(fn), 3))
            if after:
                after(name)
    return ms


class Ragged:
    def __init__(self, B, per_query):
        self.B, self.cap = B, int(B * per_query * 1.2) + 4096
        self.lims = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        self.keys = torch.empty(self.cap, dtype=torch.int64, device=dev)
        self.dist = torch.empty(self.cap, dtype=torch.float32, device=dev)

    def plain(self, Q, r):
        g.range_search_device(Q.data_ptr(), self.B, d, r.data_ptr(), self.cap, self.lims.data_ptr(), self.keys.data_ptr(),
                              self.dist.data_ptr(), stream=stream)

    def filtered(self, Q, r, f):
        g.range_search_filtered_device(Q.data_ptr(), self.B, d, r.data_ptr(), f, self.cap, self.lims.data_ptr(),
                                       self.keys.data_ptr(), self.dist.data_ptr(), stream=stream)


if args.control:
    lines = []
    for B in (1024, BMAX):
        Q = QALL[:B].contiguous()
        top10, top256 = Searcher(g, B, 10, d, dev), Searcher(g, B, 256, d, dev)
        top256.run(Q, H.MODE_EXACT, 0)
        torch.cuda.synchronize()
        r10, r100 = top256.dist[:, 9].contiguous(), top256.dist[:, 99].contiguous()
        del top256
        out = Ragged(B, 100)
        ms = run_legs({"top10": lambda: top10.run(Q, H.MODE_EXACT, 0), "range10": lambda: out.plain(Q, r10),
                       "range100": lambda: out.plain(Q, r100)})
        g.device_status()
        lines.append(f"{args.control:7s}: batch {B:5d} exact top-10 " + " ".join(f"{x:.3f}" for x in ms["top10"]) +
                     ", plain range search at 10 hits " + " ".join(f"{x:.3f}" for x in ms["range10"]) +
                     ", at 100 hits " + " ".join(f"{x:.3f}" for x in ms["range100"]))
        print(lines[-1], flush=True)
    with open(os.path.join(args.out, "filtered_range.txt"), "a") as fh:
        fh.write("\n".join(lines) + "\n")
    g.close()
    sys.exit(0)

rows, lines = [], []
keys_all = np.arange(n, dtype=np.int64)
rng = np.random.default_rng(4321)
for pct in (100.0, 10.0, 1.0, 0.1):
    mask = np.ones(n, bool) if pct == 100.0 else rng.random(n) < pct / 100.0
    m = int(mask.sum())
    f = g.Filter(keys_all[mask])
    for B in (1024, BMAX):
        Q = QALL[:B].contiguous()
        ok = torch.empty((B, 256), dtype=torch.int64, device=dev)
        od = torch.empty((B, 256), dtype=torch.float32, device=dev)
        on = torch.empty(B, dtype=torch.int32, device=dev)

        def ftop(k):
            g.search_filtered_exact_device(Q.data_ptr(), B, d, k, f, ok.data_ptr(), od.data_ptr(), on.data_ptr(),
                                           stream=stream)

        ftop(256)
        torch.cuda.synchronize()
        dist256 = od.view(B, 256)
        radii = {10: dist256[:, 9].contiguous(), 100: dist256[:, 99].contiguous()}
        out = Ragged(B, 1000)
        legs = {"ftop10": lambda: ftop(10), "ftop256": lambda: ftop(256)}
        for e, r in radii.items():
            legs[f"frange{e}"] = (lambda r=r: out.filtered(Q, r, f))
            if e * 100.0 / pct <= 1000:  # the plain search's expected hits per query at this radius
                legs[f"range{e}"] = (lambda r=r: out.plain(Q, r))
        extra = {}

        def after(name):
            if name.startswith("frange") or name.startswith("range"):
                x = {"hits": int(out.lims[B].item()), "candidates": g.get_option("last_range_candidates"),
                     "fallback_queries": g.get_option("last_range_fallback_queries"),
                     **{f"{s}_ms": round(g.get_option(f"last_range_{s}_ns") / 1e6, 3)
                        for s in ("filter", "refine", "sweep", "order")}}
                if name.startswith("frange"):
                    for s in ("compact", "gather"):
                        x[f"{s}_ms"] = round(g.get_option(f"last_fx_{s}_ns") / 1e6, 3)
                extra[name] = x

        ms = run_legs(legs, after)
        g.device_status()
        med = {k_: float(np.median(v)) for k_, v in ms.items()}
        rows.append({"allowed_pct": pct, "allowed_rows": m, "batch": B, "kernel_ms": ms,
                     "kernel_ms_median": {k_: round(v, 3) for k_, v in med.items()}, "range": extra})
        lines.append(f"{pct:5.1f} % allowed ({m:7d} rows), batch {B:5d}: filtered exact top-10 {med['ftop10']:9.3f} ms, "
                     f"filtered exact k=256 {med['ftop256']:9.3f} ms")
        for e in radii:
            x = extra[f"frange{e}"]
            plain = (f"{med[f'range{e}']:9.3f} ms ({extra[f'range{e}']['hits'] / B:.1f} hits per query, "
                     f"{extra[f'range{e}']['fallback_queries']} fallback queries)" if f"range{e}" in med else "not run")
            lines.append(f"{pct:5.1f} % allowed, batch {B:5d}, radius at the {e:3d}th allowed distance: filtered range search "
                         f"{med[f'frange{e}']:9.3f} ms, {x['hits'] / B:6.1f} hits per query, "
                         f"{x['candidates'] / max(x['hits'], 1):5.2f} candidates per hit, {x['fallback_queries']} fallback "
                         f"queries; row set: compact {x['compact_ms']:.3f}, gather {x['gather_ms']:.3f}; first chunk: filter "
                         f"{x['filter_ms']:.3f}, refine {x['refine_ms']:.3f}, sweep + prefix + gather {x['sweep_ms']:.3f}; "
                         f"call: order {x['order_ms']:.3f}; plain range search at the same radius: {plain}")
        for line in lines[-3:]:
            print(line, flush=True)
        del out
    f.close()

head = (f"filtered range search, bench index {n} x {d} cosine; kernel ms are last_kernel_ms medians of {REPS} repeats after "
        f"one warm-up, the legs alternating on one handle in one session; range_expect at its default (64); random "
        f"filters; radii: the filtered exact search's 10th / 100th distances")
with open(os.path.join(args.out, "filtered_range.txt"), "w") as fh:
    fh.write(head + "\n" + "\n".join(lines) + "\n")
with open(os.path.join(args.out, "filtered_range.json"), "w") as fh:
    json.dump({"what": head, "rows": rows}, fh, indent=1)
g.close()
