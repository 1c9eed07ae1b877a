"""The harder-data graph (bench.config_harder's build: latent 32, 1M x 768 cosine,
M 32, M0 63, efC 512, build_expand 4, upper_efc 256) searched past ef 512 on the
LDS-list tier (beam.hpp k_search_beam_lds): recall@10 against the exact path on
4,096 queries; queries/s on 16,384-query batches; expansions, rows scored in f32 and
visited resets per query; f32-scored rows per second.
Lines: ef 512 on the register list (default options: the yardstick), ef 512 on the
LDS list (beam_lds_min_ef 65: the same search, so the rows/s ratio is the list's
cost), then ef 768 / 1024 / 1536 / 2048, each at search_expand 1 and 4.
Usage: python tools/wide_ef_probe.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hnsw_amd as H  # noqa: E402
from bench import Searcher, gen_vectors, recall_at_k  # noqa: E402

dev = torch.device("cuda")
n, d, B, REPS = 1_000_000, 768, 16384, 3
X = gen_vectors(n, d, 4321, 32, 1000, dev, "cosine")
Q = gen_vectors(B, d, 4321 + 7777, 32, 1000, dev, "cosine")
g = H.Graph(M=32, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=5, build_mode=H.BUILD_BATCH, m0=63,
            ef_construction=512, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4, upper_efc=256,
            screen=1, batch_ratio_pct=20)
g.reserve(n, d)
g.add_device(np.arange(n), X.data_ptr(), n, d)
del X
tk, _, tn = (x.clone() for x in Searcher(g, 4096, 10, d, dev).run(Q[:4096], H.MODE_EXACT, 0))
S = Searcher(g, B, 10, d, dev)


def line(tier, ef, xw, lds_min_ef):
    g.set_option("search_expand", xw)
    g.set_option("beam_lds_min_ef", lds_min_ef)
    kk, _, nn = (x.clone() for x in S.run(Q, H.MODE_BEAM, ef))
    r = recall_at_k(kk[:4096], nn[:4096], tk, tn, 10)
    g.reset_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        S.run(Q, H.MODE_BEAM, ef)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / REPS
    st = g.stats()
    per = REPS * B
    print(f"{tier} ef={ef} search_expand={xw}: recall {r:.4f}, {B / dt:.0f} queries/s, "
          f"{st['search_expansions'] / per:.1f} expansions/query, {st['search_f32_evals'] / per:.1f} f32 rows/query, "
          f"{st['visited_resets'] / per:.2f} resets/query, {st['search_f32_evals'] / REPS / dt / 1e6:.2f} M f32 rows/s",
          flush=True)


for xw in (1, 4):
    line("register", 512, xw, 513)
    line("lds", 512, xw, 65)
for ef in (768, 1024, 1536, 2048):
    for xw in (1, 4):
        line("lds", ef, xw, 513)
g.close()
