"""In-place update on the bench index (1M x 768 cosine, built as bench.py builds it).

For 0.1 %, 1 % and 10 % of the rows, chosen uniformly at random and given fresh draws of the
generator, three routes to the same content, on twin handles built identically in this process:

  update          mhnsw_update_device (rows keep their ids and filter bits)
  delete+add      BatchDelete of the keys, then add_device of the new vectors (new row ids, the
                  old rows stay as deleted rows)
  +compact        the same handle, then Compact (the deleted rows leave the store)

Per route: wall ms and rows/s (device synchronised), for the update the device ms of its three
steps (time_build 1: detach, overwrite, re-insert), last_update_chunks and last_update_repaired;
recall@10 at ef 64 of 1,024 fresh queries against the handle's own exact mode before and after,
and the share of the updated rows whose new vector finds its own key first at ef 64.

Writes <out>/update.txt and .json.
Usage: python tools/update_probe.py [--out profiles] [--nbase N] [--shares 0.001,0.01,0.1]"""
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
ap.add_argument("--shares", default="0.001,0.01,0.1")
args = ap.parse_args()

dev = torch.device("cuda")
n, d, B = args.nbase, 768, 1024
M, M0 = 16, 40
X = gen_vectors(n, d, 1234, 12, 1000, dev, "cosine")
Q = gen_vectors(B, d, 1234 + 7777, 12, 1000, dev, "cosine").cpu().numpy()
KEYS = np.arange(n, dtype=np.int64)
rng = np.random.default_rng(99)


def build():
    g = H.Graph(M=M, Ml=0.25, EfSearch=64, Distance=H.CosineDistance, Rng=1234, build_mode=H.BUILD_BATCH, m0=M0,
                ef_construction=400, heuristic=2, keep_pruned=1, prune_alpha_pct=115, build_expand=4,
                batch_ratio_pct=20, upper_efc=128, screen=1, time_build=1)
    g.reserve(n + n // 8, d)  # (room for the rows delete+add appends)
    g.add_device(KEYS, X.data_ptr(), n, d)
    return g


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def delete_keys(g, keys):
    """mhnsw_delete itself (Graph.BatchDelete walks the keys in Python: not the route's cost)"""
    import ctypes as C

    out = np.zeros(len(keys), np.uint8)
    rc = H.load().mhnsw_delete(g._h, keys.ctypes.data_as(C.POINTER(C.c_int64)), len(keys),
                               out.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0 and out.all()


def recall(g):
    bk, _, bn = g.search_arrays(Q, 10, mode=H.MODE_BEAM, ef=64)
    xk, _, xn = g.search_arrays(Q, 10, mode=H.MODE_EXACT)
    hit = sum(len(set(bk[b, :bn[b]].tolist()) & set(xk[b, :xn[b]].tolist())) for b in range(B))
    return hit / float(xn.sum())


def self_found(g, keys, V):
    found = 0
    for lo in range(0, len(keys), 16384):
        bk, _, bn = g.search_arrays(V[lo:lo + 16384], 1, mode=H.MODE_BEAM, ef=64)
        found += int(((bn == 1) & (bk[:, 0] == keys[lo:lo + 16384])).sum())
    return found / len(keys)


def leg(share, seed):
    m = max(1, int(round(share * n)))
    keys = np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    # fresh draws of the rows' own generator: the same mixture, rows of the stream past the stored ones
    V = gen_vectors(m, d, 1234, 12, 1000, dev, "cosine", offset=n + seed * (n // 4))
    Vh = V.cpu().numpy()
    rec = {"share": share, "rows": m}
    # update
    g = build()
    r0 = recall(g)
    found, ms = wall(lambda: g.update_device(keys, V.data_ptr(), m, d))
    assert found.all() and g.Len() == n and g.get_option("dead_rows") == 0
    rec["update"] = dict(wall_ms=ms, rows_per_s=m / ms * 1e3, device_ms=g.get_option("last_update_ns") / 1e6,
                         detach_ms=g.get_option("last_update_detach_ns") / 1e6,
                         overwrite_ms=g.get_option("last_update_overwrite_ns") / 1e6,
                         insert_ms=g.get_option("last_update_insert_ns") / 1e6,
                         chunks=g.get_option("last_update_chunks"), repaired=g.get_option("last_update_repaired"),
                         dropped_proposals=g.stats()["dropped_proposals"], recall_before=r0, recall_after=recall(g),
                         self_found=self_found(g, keys, Vh), stored_rows=n)
    g.close()
    # delete + add, then + compact, on the twin
    g = build()
    r0 = recall(g)
    _, dms = wall(lambda: delete_keys(g, keys))
    _, ams = wall(lambda: g.add_device(keys, V.data_ptr(), m, d))
    rec["delete_add"] = dict(wall_ms=dms + ams, delete_ms=dms, add_ms=ams, rows_per_s=m / (dms + ams) * 1e3,
                             recall_before=r0, recall_after=recall(g), self_found=self_found(g, keys, Vh),
                             stored_rows=n + m)
    removed, cms = wall(g.Compact)
    assert removed == m
    rec["delete_add_compact"] = dict(wall_ms=dms + ams + cms, compact_ms=cms, rows_per_s=m / (dms + ams + cms) * 1e3,
                                     recall_before=r0, recall_after=recall(g), self_found=self_found(g, keys, Vh),
                                     stored_rows=n)
    g.close()
    return rec


legs = [leg(float(s), i) for i, s in enumerate(args.shares.split(",")) if s]
lines = ["in-place update on the bench index: %d x %d cosine, M %d, m0 %d, efC 400, batch_ratio_pct 20" % (n, d, M, M0),
         "(recall: recall@10 at ef 64 of %d fresh queries against the handle's exact mode, before -> after;" % B,
         " self: share of the updated rows whose new vector finds its own key first at ef 64)", ""]
for r in legs:
    u = r["update"]
    lines.append("%.1f %% of the rows (%d)" % (100 * r["share"], r["rows"]))
    lines.append("  update              %9.1f ms wall %9.0f rows/s  recall %.4f -> %.4f  self %.4f  stored rows %d"
                 % (u["wall_ms"], u["rows_per_s"], u["recall_before"], u["recall_after"], u["self_found"], u["stored_rows"]))
    lines.append("     device %.1f ms = detach %.1f + overwrite %.2f + re-insert %.1f; %d chunk(s), %d (layer, row) pairs "
                 "repaired, %d dropped proposals" % (u["device_ms"], u["detach_ms"], u["overwrite_ms"], u["insert_ms"],
                                                     u["chunks"], u["repaired"], u["dropped_proposals"]))
    for name, key in (("delete + add", "delete_add"), ("delete + add + compact", "delete_add_compact")):
        x = r[key]
        lines.append("  %-19s %9.1f ms wall %9.0f rows/s  recall %.4f -> %.4f  self %.4f  stored rows %d"
                     % (name, x["wall_ms"], x["rows_per_s"], x["recall_before"], x["recall_after"], x["self_found"],
                        x["stored_rows"]))
    x = r["delete_add"]
    lines.append("     delete %.1f ms + add %.1f ms; compact %.1f ms" % (x["delete_ms"], x["add_ms"],
                                                                        r["delete_add_compact"]["compact_ms"]))
    lines.append("")
print("\n".join(lines))
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "update.txt"), "w") as f:
    f.write("\n".join(lines))
with open(os.path.join(args.out, "update.json"), "w") as f:
    json.dump({"legs": legs}, f, indent=1)
