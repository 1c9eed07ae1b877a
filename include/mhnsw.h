/*
 * mhnsw.h -- C ABI of the MI355X-native HNSW engine (libmhnsw.so).
 *
 * This is the drop-in boundary for the hot path of TFMV/hnsw (Go): the
 * distance sweep -> layer-0 greedy/beam search -> M-neighbour selection on
 * insert.  Every entry point is plain C (pointers + sizes, no torch types) so
 * the Go package can bind it through cgo; see INTEGRATION.md for the binding
 * a maintainer would add.  Each declaration names the reference interface it
 * replaces (paths relative to the reference repository root).
 *
 * Conventions
 *  - Keys are int64 (the reference's Graph[int]); vectors are float32,
 *    row-major, `dim` contiguous floats per row.
 *  - Host-pointer entry points copy their inputs before returning (the cgo
 *    rule forbids C from retaining Go pointers).  *_device entry points take
 *    device pointers and enqueue asynchronously on the given HIP stream
 *    (NULL = the HIP null stream, as in the HIP/CUDA runtime convention).
 *  - Return value: MHNSW_OK (0) or a negative error class; the message, with
 *    the reference's wording where one exists, is mhnsw_last_error(h).
 *  - Concurrency mirrors graph.go:328 (sync.RWMutex): searches may run
 *    concurrently on one handle; add/import are exclusive.
 */
#ifndef MHNSW_H
#define MHNSW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mhnsw_index mhnsw_index;

/* DistanceFunc identities (distance.go:25-28 distanceFuncs registry) */
#define MHNSW_NO_DISTANCE (-1) /* Graph.Distance == nil */
#define MHNSW_COSINE 0         /* distance.go:15 CosineDistance */
#define MHNSW_EUCLIDEAN 1      /* distance.go:20 EuclideanDistance */

/* search modes */
#define MHNSW_MODE_COMPAT 0 /* graph.go:94-170 semantics, results in heap order */
#define MHNSW_MODE_BEAM 1   /* standard HNSW best-first (ef), sorted results   */
#define MHNSW_MODE_EXACT 2  /* brute force (MFMA scores + canonical re-rank)   */

/* build modes (option "build_mode") */
#define MHNSW_BUILD_COMPAT 0 /* graph.go:437-531 sequential Add semantics */
#define MHNSW_BUILD_BATCH 1  /* batched parallel insert (throughput)      */
#define MHNSW_BUILD_FLAT 2   /* vector store only, exact search (hnsw-extensions/hybrid/exact.go ExactIndex) */

/* error classes */
#define MHNSW_OK 0
#define MHNSW_EINVAL (-1)       /* Validate() failure / bad argument          */
#define MHNSW_EDIM (-2)         /* "embedding dimension mismatch: %d != %d"   */
#define MHNSW_EK (-3)           /* "k must be greater than 0, got %d"         */
#define MHNSW_ENOMEM (-4)
#define MHNSW_EDEVICE (-5)      /* HIP runtime / kernel launch failure         */
#define MHNSW_EUNSUPPORTED (-6) /* outside this build's supported envelope     */
#define MHNSW_EINTERNAL (-7)

/* ---- lifecycle: NewGraph / NewGraphWithConfig (graph.go:340-366) ----
 * Binds the handle to the current HIP device.  Fails with the Validate()
 * message (graph.go:916-937) when the configuration is invalid; the message is
 * then available from mhnsw_last_error(NULL). */
int mhnsw_create(int metric, int M, double ml, int ef_search, uint64_t seed, mhnsw_index **out);
void mhnsw_destroy(mhnsw_index *h);
const char *mhnsw_last_error(const mhnsw_index *h);

/* ---- public Graph fields (graph.go:305-326): Distance, M, Ml, EfSearch, Rng ---- */
int mhnsw_set_params(mhnsw_index *h, int metric, int M, double ml, int ef_search);
int mhnsw_get_params(const mhnsw_index *h, int *metric, int *M, double *ml, int *ef_search);
int mhnsw_seed(mhnsw_index *h, uint64_t seed); /* Rng = rand.New(rand.NewSource(seed)) analogue */
/* engine options: "build_mode", "m0" (layer-0 degree cap, batch mode),
 * "ef_construction" (<= 512), "heuristic" (0 closest-M, 1 HNSW heuristic on new rows,
 * 2 also when a reverse edge overflows a row), "keep_pruned", "prune_alpha_pct"
 * (heuristic slack x100: c is dropped when alpha*d(c,kept) < d(u,c); 100 = HNSW
 * Alg. 4), "batch_min", "batch_max", "batch_ratio_pct" (batched insert: each batch holds this
 * % of the rows already indexed, default 5 -- a batch is searched against the index as it
 * stood before it, so larger batches build faster but link a batch's rows to each other
 * only through reverse edges: adding 1,000 rows to a 5,100-row index in one 20 % batch
 * left 16 % of them unreachable by their own vector at ef 64; "batch_link" 1 is the remedy),
 * "batch_link" (batched insert, 0 (default) or 1: after a layer's commit every row of the
 * batch searches the layer again, now that its batch-mates are in it, and takes the
 * batch-mates it finds into its neighbour selection -- the build rate with and without it
 * is measured in profiles/batch_link.txt; batch mode only, the compat and flat builds
 * ignore it),
 * "batch_link_ef" (the width of that search: 0 (default) = the width of the layer's insert
 * search, else clamped to [the layer's degree cap, 512]); read-only, of the last Add:
 * "last_link_rows" (rows, one per layer, whose selection the link pass changed),
 * "last_link_edges" (the batch-mates those selections added, counted as selected: the
 * commit's overflow rule may prune one again, and the reverse edges the proposals add are
 * not counted), "last_link_ns" (its kernels' device time with
 * "time_build" 1, else 0), "vis_log2" (compat / build visited sets:
 * 2^n entries), "vis_entries" (beam search's visited set, 0 = 1.25 * 2^vis_log2),
 * "build_expand" (batched insert: entries expanded per step of its layer
 * searches, 1-4, default 4 -- they fetch their adjacency rows in one round
 * trip and evaluate their new neighbours as one batch), "upper_efc" (batched
 * insert: the candidate list of its searches in the layers above 0, 0 (default) =
 * efConstruction on every layer; those rows hold M neighbours and their
 * searches are narrow launches -- 128 builds the 1M bench index 22 % faster at
 * the same recall), "search_expand" (beam
 * mode: entries expanded per step of the layer-0 search, 1 (default, the
 * standard best-first search), 2 or 4 -- the best unexpanded entries are taken
 * together, their adjacency rows fetched in one round trip and their new
 * neighbours scored as one batch; a different search from 1 (results can
 * differ), bit-identical to the oracle's og_set_search_expand; always the
 * one-wave kernel), "search_order" (beam mode, 0 or 1: batches of at least
 * "search_order_min_b" queries run the greedy descent as a pre-pass, sort the
 * queries by their descent path and search layer 0 in that order, so that
 * queries walking the same neighbourhood run on one XCD at the same time and
 * share its L2; each query's search is independent of the others, so the
 * lists and the search counters are the same bit for bit; smaller batches and
 * the 4-wave small-batch kernel always run the single fused launch; the
 * pre-pass, the sort and the search all run on the caller's stream from
 * buffers the handle owns, and last_kernel_ms covers all of them),
 * "search_order_min_b" (>= 1: the smallest ordered batch; the default is the
 * smallest measured batch at which the extra launches do not cost more than
 * the order saves), "search_order_top" (the highest layer whose descent node
 * goes into the sort key, 0 (default) = the lowest layer with at most
 * batch / 128 nodes), "search_order_fields" (how many layers from there down
 * go into the key, 1-8, 0 (default) = 3; each takes 64 / fields bits, a hash
 * of the node id where the id does not fit; the pre-pass stops at the key's
 * lowest layer and the search launch walks the layers below it),
 * "search_order_map" (0 (default): workgroup i takes sorted position
 * (i % 8) * ceil(B / 8) + i / 8, one contiguous run of the sorted queries per
 * XCD; 1: workgroup i takes position i), "exact_kk",
 * "exact_thr_rank" (precision 3: the threshold is the sample's J-th best score,
 * J = max(k, this) capped at kk; 0 (default) = max(k, kk / 8)),
 * "exact_sample" (precision 3: at most this many row tiles form the threshold
 * sample, every ceil(tiles / this)-th, default 64),
 * "exact_precision" (exact-mode scoring: 0 f32-input MFMA, 1 bf16x3 split MFMA,
 * 2 fp16 2-product split MFMA, 3 (default) fp16 1-product MFMA with the top-kk
 * preselection fused into the GEMM epilogue; all preselect, re-rank canonically
 * and certify, so results are identical),
 * "exact_tile" (GEMM variant, 0 = the measured best per precision; precisions 1/2:
 * 1 128x256, 2 128x128, 3 256x256 ring tiles; precision 3: 34 (the default)
 * the persistent two-group ping-pong stream k_h1_pp16 on 16x16x32 MFMAs with
 * the fused filter storing per-lane records of a block row's accumulators,
 * 5 the ring kernel's fused filter (128x256), which also runs every shape
 * k_h1_pp16 does not admit), "compat_waves" (1 or 8 waves scoring the compat insert's
 * distance batches), "upper_ef" (beam mode: upper-layer descent width, 1 =
 * greedy), "beam_mw_max_b" (beam mode, ef and k <= 128: batches of at most this
 * many queries run one workgroup of 4 waves per query -- the single-query
 * latency path of ParallelSearch, graph.go:631-790; default 512, 0 = never;
 * results are identical either way; the standard search only: search_expand 2 / 4
 * run the one-wave kernel), "beam_lds_min_ef" (beam mode: the smallest max(ef, k)
 * whose layer-0 list lives in LDS instead of registers; default 513, i.e. past
 * the widest register list, valid [65, 513]; the results are identical on either
 * list, lower values let the LDS list be run against the register lists at
 * equal ef), "build_mw_max" (batched insert with the screening
 * copy, build_expand 2-4: a layer launch of at most this many inserts runs one
 * workgroup of 4 waves per insert, the candidate batches of its searches split
 * over the waves; default 256, 0 = never; the same graph either way), "vis_compact" (beam mode at max(ef, k) > 128 and batched insert at
 * efConstruction > 128, default 1: when node
 * ids are below 2^24 the visited set stores 16-bit entries -- 8,192 ids in 16 KiB
 * of LDS, where the beam search's 32-bit set holds 5,120 in 20 KiB and the
 * insert's (vis_log2 12) 4,096 in 16 KiB -- so a large-ef search resets it less;
 * exact, the same results and graph either way), "screen" (beam mode and batched insert, default 1: keep an fp16
 * copy of the rows; a candidate is skipped only when the copy proves the f32
 * distance rejects it, so results are unchanged);
 * "max_rows" (row capacity limit, 0 = none: an Add that would need more rows
 * fails with MHNSW_ENOMEM and leaves the index, its key maps and its Rng as
 * they were);
 * read-only: "pitch", "capacity", "strkeys", "strkey_relabels", "last_gemm_ns" (device
 *            time of the last timed exact search's fused fp16 score GEMM, first query chunk),
 *            "screen_err_ppb" (the fp16 screening copy's measured max relative
 *            rounding E, the margin its rejects use, in parts per 1e9) */
int mhnsw_set_option(mhnsw_index *h, const char *name, int64_t value);
int mhnsw_get_option(const mhnsw_index *h, const char *name, int64_t *value);
/* Graph.Validate (graph.go:916-937) */
int mhnsw_validate(mhnsw_index *h);
/* pre-size device storage for n vectors of `dim` floats */
int mhnsw_reserve(mhnsw_index *h, int64_t n, int dim);

/* ---- Graph.Add / Graph.BatchAdd (graph.go:437-531, 942-1042) ----
 * levels: NULL draws each level like randomLevel (graph.go:388-417) from the
 * handle's RNG; non-NULL injects them (a host drawing from its own Rng, or
 * parity testing).  COMPAT build mode follows BatchAdd's walk: the nodes are
 * inserted in order; a node whose key is already present (in the index or
 * earlier in the batch) replaces the key's nodes -- after its layer search,
 * every layer holding the key deletes and isolates it (graph.go:1015-1024) --
 * and when layer 0 held the key the walk stops with "node not added"
 * (MHNSW_EINTERNAL; graph.go:1035-1037: Len() did not grow); a key whose nodes
 * sat only in upper layers (left by a failed insert) leaves Len() one higher,
 * and the walk goes on.  A failing insert ("no nodes found in
 * neighborhood search", graph.go:1009) also ends the walk, leaving the graph as
 * the reference leaves it.  Add of a present key deadlocks in the reference
 * (graph.go:511-513 -> Delete re-locks, :844); here it is BatchAdd's walk.
 * BATCH / FLAT build modes reject a present key (MHNSW_EUNSUPPORTED). */
int mhnsw_add(mhnsw_index *h, const int64_t *keys, const float *vecs, int64_t n, int dim, const int32_t *levels);
/* same, vectors already in HBM (keys/levels stay host pointers) */
int mhnsw_add_device(mhnsw_index *h, const int64_t *keys, const float *d_vecs, int64_t n, int dim,
                     const int32_t *levels);
/* For hosts that draw levels from their own Rng (graph.go:962: one draw per
 * insert the walk reaches, from the layer-0 size at that moment): *nwalk = the
 * inserts up to and including the first key already present (or repeated) --
 * where a COMPAT walk may stop (it does when that key's node holds a layer at
 * or below the new level); *one_by_one = 1 when an insert may fail with "no
 * nodes found in neighborhood search" (the index holds deleted or replaced
 * rows).  A host draws nwalk levels, adds those nodes, and repeats with the
 * rest until done or an error ends the walk.  When one_by_one is set, a host
 * that can rewind its Rng still adds the nwalk nodes in one call: after an
 * error, mhnsw_add_reached says how many inserts the walk got to (the draws
 * the reference made, graph.go:962); the host rewinds and redraws that many.
 * A host that cannot rewind adds one node per call instead. */
int mhnsw_add_plan(mhnsw_index *h, const int64_t *keys, int64_t n, int64_t *nwalk, int *one_by_one);
/* The inserts the last mhnsw_add / mhnsw_add_device walk reached, counting a
 * replacing insert ("node not added") and a failing one ("no nodes found in
 * neighborhood search", graph.go:1009) -- i.e. the levels it consumed; 0 after
 * an error that left the index untouched (validation, dimension, capacity). */
int mhnsw_add_reached(const mhnsw_index *h, int64_t *reached);

/* ---- Graph.Search / Graph.BatchSearch (graph.go:534-625, 1047-1110) ----
 * B queries of `dim` floats; outputs hold B*k slots; out_n[b] results for
 * query b.  ef <= 0 uses EfSearch.  entry_key (nullable) replaces the
 * arbitrary layer.entry() (graph.go:250-258) of the top layer.
 * MHNSW_MODE_BEAM takes 1 <= max(ef, k) <= 2048 (up to 512 the list is held in
 * registers, from 513 in LDS: the same search, bit-identical to the oracle's);
 * past 2048 the call fails with MHNSW_EUNSUPPORTED, "beam mode supports
 * max(ef,k) <= 2048".
 * MHNSW_MODE_EXACT takes k <= 256 ("exact mode supports k <= 256"), and with
 * the option "exact_wide" = 1 (default 0) k <= 4096 ("exact mode supports
 * k <= 4096"): the wide exact search.  A search at k > 256, or at k >=
 * "exact_wide_min_k" (default 257, any value >= 1), then runs the range
 * search's pipeline at a per-query radius estimated from the sample pass (the
 * J-th smallest sample score, J from a Poisson tail bound on k x the sampled
 * fraction), cuts each query's sorted hits at k, and answers the queries whose
 * radius held fewer than k rows -- or that got no room in the hit buffer -- by
 * a select over the canonical distances of every row.  The results are the
 * exact mode's: the k rows of smallest canonical distance by (distance, row
 * id), the same skipped rows, NaN never returned, out_n[b] = min(k, rows
 * available); always scored at precision 3.  The filtered exact calls below
 * take the same path over a filter's allowed rows.  Options: "wide_fallback_bytes"
 * (default 2^30: the fallback's distance rows, queries per group = this /
 * (4 x rows)); test option "wide_force_fallback" (1: every query is answered by
 * the fallback select).  Read-only, of the last exact search:
 * last_wide_queries (the queries that took the wide path, 0: none),
 * last_wide_fallback_queries, last_wide_hits (hits that reached the sort: over
 * B x k it is the overshoot), last_wide_rank (J), last_wide_room (hit-buffer
 * entries per query), and of a timed search last_wide_sample_ns,
 * last_wide_radius_ns, last_wide_range_ns (first chunk of queries),
 * last_wide_emit_ns (sort and cut) and last_wide_fallback_ns; the
 * last_range_*_ns options then describe its range stages. */
int mhnsw_search(mhnsw_index *h, const float *queries, int64_t B, int dim, int k, int mode, int ef,
                 const int64_t *entry_key, int64_t *out_keys, float *out_dist, int32_t *out_n);
int mhnsw_search_device(mhnsw_index *h, const float *d_queries, int64_t B, int dim, int k, int mode, int ef,
                        int64_t *d_keys, float *d_dist, int32_t *d_n, void *stream);
/* Errors of *_device searches.  mhnsw_search_device returns once its kernels
 * are enqueued, so what they detect (a compat search whose visited set
 * overflows -- the reference's visited map is exact, graph.go:141-144 -- or an
 * out-of-range id in the adjacency) cannot be its return value: it accumulates
 * in a per-handle word.  This call waits for the last enqueued search, returns
 * MHNSW_OK or MHNSW_EINTERNAL with the message of the host-pointer path, and
 * clears the word. */
int mhnsw_device_status(mhnsw_index *h);

/* ---- Filtered search (the reference's hnsw-extensions/facets, search.go:15-88,
 * with the predicate applied inside the layer-0 walk; DESIGN.md "Filtered
 * search") ----
 * A filter is an allow-list of rows owned by the handle: a bitmap over its row
 * capacity.  mhnsw_filter_create allows the live layer-0 rows of `keys` (absent
 * keys are ignored) and returns the filter's id; mhnsw_filter_update allows
 * (allow != 0) or disallows the rows of `keys`.  Rows added later are not
 * allowed until an update names their keys.  mhnsw_filter_count: the allowed
 * rows that are live.  At most 1024 filters per handle.  Import / Load drop
 * every filter (the row ids change): its id then fails with MHNSW_EINVAL,
 * "unknown filter %d". */
int mhnsw_filter_create(mhnsw_index *h, const int64_t *keys, int64_t n, int *out_filter);
int mhnsw_filter_update(mhnsw_index *h, int filter, const int64_t *keys, int64_t n, int allow);
int mhnsw_filter_count(mhnsw_index *h, int filter, int64_t *rows);
int mhnsw_filter_destroy(mhnsw_index *h, int filter);
/* The beam search among the allowed rows: query b returns its nearest rows of
 * filter filter_of[b] (-1: every live row).  The search routes through every
 * row in a list of `route` entries and collects the allowed ones in a list of
 * max(ef, k) <= 128 entries; it stops when no unexpanded entry can improve
 * that list.  ef <= 0 uses EfSearch; route <= 0 uses the option filter_route
 * (default 1024); a route below max(ef, k) is raised to it; route <= 2048.
 * With every row allowed the result is mhnsw_search's in MHNSW_MODE_BEAM at the
 * same ef, whatever the route.  A route too narrow for the filter's
 * selectivity returns fewer than k rows (no error).  Errors: MHNSW_EUNSUPPORTED
 * "filtered search supports max(ef,k) <= 128" / "filtered search supports
 * route <= 2048"; MHNSW_EINVAL for a filter_of entry that names no filter (the
 * *_device call, whose filter_of is a device pointer, reports it through
 * mhnsw_device_status). */
int mhnsw_search_filtered(mhnsw_index *h, const float *queries, int64_t B, int dim, int k, int ef, int route,
                          const int32_t *filter_of, int64_t *out_keys, float *out_dist, int32_t *out_n);
int mhnsw_search_filtered_device(mhnsw_index *h, const float *d_queries, int64_t B, int dim, int k, int ef, int route,
                                 const int32_t *d_filter_of, int64_t *d_keys, float *d_dist, int32_t *d_n,
                                 void *stream);
/* The exact search among the allowed rows: a brute force over the filter's rows
 * only.  Query b considers the rows whose bit is set in its filter and which a
 * MHNSW_MODE_EXACT search could return (not deleted, not left partial by a
 * failed insert), and returns the k of them with the smallest canonical
 * distance by (distance, row id); a NaN distance is never returned; out_n[b] =
 * min(k, rows available), 0 and no error for an empty allow-set.  The result is
 * the exact mode's over an index that holds those rows only, bit for bit.  Per
 * distinct filter the call lists the allowed rows in ascending order from the
 * bitmap, gathers their fp16 rows into a dense plane and runs the exact mode's
 * stages on it (certificate and fallback included); nothing is kept between
 * calls.  With exact_precision 0 or 1, which keep no fp16 row plane, the call
 * scores at precision 3 (the results do not depend on the precision).  Works
 * in every build mode, MHNSW_BUILD_FLAT included.  k <= 256, or with the option
 * "exact_wide" k <= 4096 (the wide exact search, see mhnsw_search).
 * mhnsw_search_filtered_exact: filter_of[b] (host) is query b's filter, -1 for
 * every live row; the batch is grouped by filter, one pass per distinct one
 * (-1: mhnsw_search in MHNSW_MODE_EXACT), each query's results at its own
 * position.  mhnsw_search_filtered_exact_device: one filter (or -1) for the
 * whole batch, enqueued on `stream` with the handle's workspace like
 * mhnsw_search_device; a caller with a mixed batch groups it.  Errors:
 * MHNSW_EUNSUPPORTED "exact mode supports k <= 256" (with "exact_wide":
 * "exact mode supports k <= 4096"), MHNSW_EINVAL "unknown
 * filter %d".  mhnsw_last_kernel_ms covers the last pass, compaction through
 * re-rank; the read-only options last_fx_compact_ns, last_fx_gather_ns and (of
 * the first chunk of queries; the exact mode runs a large batch in chunks)
 * last_fx_select_ns, last_fx_rerank_ns, last_fx_fallback_ns split it.  There is no automatic switch between this call
 * and the walk.  Guidance (measured on 1M x 768 cosine rows, batches of 16,384,
 * k 10, profiles/filtered_exact.txt; DESIGN.md "Filtered exact search"): with
 * 10 % of the rows allowed or fewer this call is faster than the walk (7.6
 * against 81 ms at 10 %, 3.7 against 442 ms at 1 %) and below 1 % it is the only
 * one that answers; at 50 % and more the walk is faster (12.7 against 18.1 ms
 * at 50 %, at recall 0.997 against 1.0).  The crossover lies between. */
int mhnsw_search_filtered_exact(mhnsw_index *h, const float *queries, int64_t B, int dim, int k,
                                const int32_t *filter_of, int64_t *out_keys, float *out_dist, int32_t *out_n);
int mhnsw_search_filtered_exact_device(mhnsw_index *h, const float *d_queries, int64_t B, int dim, int k, int filter,
                                       int64_t *d_keys, float *d_dist, int32_t *d_n, void *stream);

/* ---- Range search: every row within a radius (faiss's range_search; DESIGN.md
 * "Range search") ----
 * For query b with radius radius[b], a row is a hit iff a MHNSW_MODE_EXACT search
 * could return it (not deleted, not left partial by a failed insert), its
 * canonical float32 distance d is finite, and d <= radius[b]: inclusive, on the
 * canonical distance itself (for MHNSW_EUCLIDEAN the square-rooted one).  NaN and
 * +inf distances are never hits; a NaN or negative radius gives zero hits and no
 * error (the comparison is d <= r as it stands: the one distance a negative radius
 * can admit is a cosine distance that rounded a few ulps below zero).  The result is ragged: lims[B + 1] is the exclusive prefix of the
 * per-query counts, query b's hits occupy [lims[b], lims[b + 1]) of keys / dist,
 * in ascending (distance, internal row id) order.
 * MHNSW_MODE_EXACT returns every hit: the radius becomes the threshold of the
 * exact mode's fp16 filter GEMM (the certificate's error bound added, so no hit
 * is filtered out), the candidates are checked canonically, and queries the
 * filter cannot cover (a bound that does not hold, an overflowed region or
 * sub-bucket, fewer than 256 rows) are answered by a canonical sweep of every
 * row.  The call always scores at exact_precision 3 (the results do not depend
 * on the precision).  Option "range_expect" (default 64): the expected hits per
 * query the filter's buffers are sized for; more hits only send queries to the
 * sweep.  Works in every build mode, MHNSW_BUILD_FLAT included.
 * MHNSW_MODE_BEAM returns the hits the beam search finds: it runs
 * mhnsw_search's beam mode at k = ef (max(ef, 1) <= 2048, ef <= 0 uses EfSearch)
 * and keeps the entries within the radius.  A per-query count equal to ef means
 * the list was exhausted: raise ef or use MHNSW_MODE_EXACT.
 * MHNSW_MODE_COMPAT fails with MHNSW_EUNSUPPORTED, "range search supports beam
 * and exact mode".  An empty index or B <= 0 gives all-zero lims.
 * mhnsw_range_search is synchronous: it writes out_lims and leaves the hits in a
 * buffer the handle owns until the next range search or mutation;
 * mhnsw_range_results copies them out (MHNSW_EINVAL when cap < lims[B]).  When
 * the hits do not fit the handle's buffer the search runs a second time with
 * room for exactly lims[B].
 * mhnsw_range_search_device is enqueued on `stream` with the handle's workspace
 * like mhnsw_search_device, without a host synchronisation: d_lims always holds
 * the true prefix; a hit whose position is >= cap is not written (the positions
 * below cap hold what a larger buffer would hold there); d_lims[B] > cap tells
 * the caller to come back with a larger buffer.  Exact mode needs
 * cap + rows < 2^31.  Read-only options: "last_range_candidates" ((query, row)
 * pairs the filter passed on to the canonical check) and
 * "last_range_fallback_queries" (queries the sweep answered); test option
 * "range_force_fallback" (1: every query takes the sweep).
 * mhnsw_last_kernel_ms covers the whole call (of a host call that ran twice,
 * the second run); the read-only options last_range_filter_ns, last_range_refine_ns
 * and last_range_sweep_ns (of the first chunk of queries) and last_range_order_ns
 * (the call's sort and emit) split an exact-mode call.  Measured on 1M x 768
 * cosine rows, batches of 16,384 (profiles/range_search.txt): 32.2 / 30.3 / 38.9 ms
 * at 10 / 100 / 1,000 hits per query, against 35.2 ms for the exact top-10 search. */
int mhnsw_range_search(mhnsw_index *h, const float *queries, int64_t B, int dim, const float *radius, int mode, int ef,
                       int64_t *out_lims);
int mhnsw_range_results(mhnsw_index *h, int64_t *out_keys, float *out_dist, int64_t cap);
int mhnsw_range_search_device(mhnsw_index *h, const float *d_queries, int64_t B, int dim, const float *d_radius, int mode,
                              int ef, int64_t cap, int64_t *d_lims, int64_t *d_keys, float *d_dist, void *stream);
/* The filtered range search: every allowed row within a radius (the reference's
 * facets/search.go searches a facet's rows by k; this extends that interface
 * by a radius; DESIGN.md "Filtered range search").  For query b with radius
 * radius[b] and filter f_b a row is a hit iff its bit is set in f_b, a
 * MHNSW_MODE_EXACT search could return it (not deleted, not left partial by a
 * failed insert), and its canonical float32 distance d is finite with
 * d <= radius[b] (the square-rooted distance for MHNSW_EUCLIDEAN).  The result
 * has mhnsw_range_search's ragged shape and order; a NaN or negative radius
 * gives what it gives there, an empty allow-set zero hits and no error, and
 * filter -1 is mhnsw_range_search itself (the same code path, the same bytes).
 * MHNSW_MODE_EXACT is the range search over the filter's rows as a gathered row
 * set (the filtered exact search's): the filter GEMM, the canonical check and
 * the sweep all run over the m allowed rows, so a call costs what m rows cost,
 * not what the index costs; with fewer than 256 allowed rows the sweep over the
 * id list is the whole path.  Every build mode works, MHNSW_BUILD_FLAT included.
 * MHNSW_MODE_BEAM returns the hits the filtered walk finds: mhnsw_search_filtered
 * at k = ef through a route list of `route` entries (0: option filter_route),
 * cut by the radius, with that call's limits and messages ("filtered search
 * supports max(ef,k) <= 128", "filtered search supports route <= 2048"); a
 * count equal to ef means the list was exhausted.  route is ignored in exact mode.
 * mhnsw_range_search_filtered: filter_of[b] (host) is query b's filter, -1 for
 * every live row.  Synchronous; the hits are left for mhnsw_range_results, with
 * the second run when they do not fit.  Exact mode groups the batch by filter
 * and runs one pass per distinct id; the passes' ragged results are moved on
 * the device to each query's own segment (only the passes' lims cross to the
 * host), and the last_* options then describe the last pass.  Beam mode is one
 * launch for any mix.
 * mhnsw_range_search_filtered_device: one filter (or -1) for the whole batch,
 * enqueued on `stream` without a host synchronisation, with the cap / true-lims
 * contract of mhnsw_range_search_device; exact mode needs cap + m < 2^31 (m:
 * the allowed rows).  A caller with a mixed batch groups it.
 * Errors: MHNSW_EINVAL "unknown filter %d"; MHNSW_EUNSUPPORTED "range search
 * supports beam and exact mode".  The last_range_* options apply as they are; a
 * filtered exact pass also fills last_fx_compact_ns and last_fx_gather_ns (its
 * row set's id list and plane).  Measurements: profiles/filtered_range.txt. */
int mhnsw_range_search_filtered(mhnsw_index *h, const float *queries, int64_t B, int dim, const float *radius,
                                int mode, int ef, int route, const int32_t *filter_of, int64_t *out_lims);
int mhnsw_range_search_filtered_device(mhnsw_index *h, const float *d_queries, int64_t B, int dim,
                                       const float *d_radius, int mode, int ef, int route, int filter, int64_t cap,
                                       int64_t *d_lims, int64_t *d_keys, float *d_dist, void *stream);

/* ---- SearchWithNegative(s) / BatchSearchWithNegatives (graph.go:1116-1537) ----
 * Query b's negatives are the next neg_count[b] rows of `negatives` (B*dim
 * queries, sum(neg_count)*dim negatives).  Candidates = Search(near,
 * max(3k,10)) in `mode`; scored in float32 as the reference (graph.go:1174-
 * 1210 / 1300-1345) and returned by descending score (ties in candidate
 * order, NaN last).  neg_count[b] == 0 runs a plain Search(near, k)
 * (out_score then holds distances).  flags bit 0 enables the reference's
 * key 7..9 boost (a test hack, graph.go:1338-1344).  k <= 85. */
int mhnsw_search_negatives(mhnsw_index *h, const float *queries, int64_t B, int dim, const float *negatives,
                           const int32_t *neg_count, int k, float neg_weight, int mode, int ef, int flags,
                           int64_t *out_keys, float *out_score, int32_t *out_n);

/* ---- Len / Dims / Lookup / Analyzer.Topography (graph.go:829, 421, 898; analyzer.go:41) ----
 * Lookup reads layer 0 (graph.go:906) and copies the key's vector. */
int64_t mhnsw_len(const mhnsw_index *h);
int mhnsw_dims(const mhnsw_index *h);
int mhnsw_lookup(mhnsw_index *h, int64_t key, float *out_vec); /* 1 found, 0 absent, <0 error */
/* out[i] = 1 when keys[i] has a live node (the `_, ok := layer.nodes[key]` test
 * of graph.go:1016 / hybrid/exact.go:30, without copying vectors) */
int mhnsw_contains(const mhnsw_index *h, const int64_t *keys, int64_t n, uint8_t *out);
int mhnsw_num_layers(const mhnsw_index *h);
int64_t mhnsw_layer_count(const mhnsw_index *h, int layer);
/* Analyzer.Connectivity (analyzer.go:20-38): mean neighbour count of each
 * non-empty layer; returns how many layers it has (writes min(that, max_layers)) */
int mhnsw_connectivity(mhnsw_index *h, double *out, int max_layers);

/* ---- Graph.Delete / Graph.BatchDelete (graph.go:843-895) ----
 * out[i] = 1 when keys[i] was present.  COMPAT build mode runs the reference's
 * isolate + replenish per key (graph.go:172-235: the deleted row keeps its
 * edges and stays reachable through one-directional links, as in Go); BATCH
 * build mode repairs every row that points at a deleted node in parallel.
 * Deleted rows are never returned by BEAM or EXACT searches. */
int mhnsw_delete(mhnsw_index *h, const int64_t *keys, int64_t n, uint8_t *out);

/* ---- ExactIndex replace-on-Add (hnsw-extensions/hybrid/exact.go:28-59: Add of
 * a present key is a map assignment) ----
 * FLAT build mode only (a vector store without links).  For every key present,
 * its row's vector is overwritten in place (norms, the fp16 screening copy and
 * the exact path's split planes follow); out[i] = 1 when keys[i] was present,
 * 0 otherwise (the caller adds those).  Keys must be distinct.  Nothing is
 * written unless every argument is valid. */
int mhnsw_replace(mhnsw_index *h, const int64_t *keys, const float *vecs, int64_t n, int dim, uint8_t *out);

/* ---- Compaction ----
 * Removes every deleted row from the handle's storage, on the device and in
 * place: live row i becomes row new(i) = the live rows below it, so the live
 * rows keep their order and every search returns the keys, distance bits and
 * counts it returned before.  Afterwards the stored rows are the live ones,
 * the capacity is unchanged (the freed tail is what later Adds fill), every
 * filter keeps its id and its rows, and the export is the old one without the
 * deleted rows, its ids renumbered.  *out_removed (nullable) = rows dropped;
 * with nothing deleted the call writes nothing.  BATCH and FLAT build modes
 * only: a COMPAT handle (whose deleted rows stay reachable), one with a
 * replaced or re-added key or with rows a failed insert left outside layer 0
 * fails with MHNSW_EUNSUPPORTED and is left as it was.  Device memory beyond
 * the index: 8 bytes per stored row and a staging buffer of at most
 * "compact_stage_rows" rows (option); MHNSW_ENOMEM leaves the index as it was.
 * Read-only options: "dead_rows", "last_compact_ns", "last_compact_dangling",
 * "last_compact_scratch_bytes". */
int mhnsw_compact(mhnsw_index *h, int64_t *out_removed);

/* ---- Update: new vectors for present keys, in place ----
 * Re-embeds stored rows on the device.  out_found[i] = 1 when keys[i] has a
 * live layer-0 row, else 0: an absent or deleted key is not added and nothing
 * is written for it (an update, not an upsert; the hosts build Upsert from
 * it).  A found row keeps its id, key, level, layer membership and filter
 * bits; its vector, norm, fp16 screening row and exact-path planes become the
 * new vector's (by row list: work proportional to the rows updated), and the
 * graph around it is relinked.  Len, the capacity, the deleted rows, every
 * layer's entry, every filter and the Rng are unchanged (no level is drawn).
 * Afterwards every layer holds deg <= cap - 1, no duplicate, no self-loop, no
 * edge to a deleted, absent or foreign row, and every stored edge distance is
 * the canonical distance between the current vectors of its two rows.
 *
 * A call works in chunks of at most min(batch_max, max(batch_min,
 * batch_ratio_pct % of the live rows)) rows (and at most half of the live
 * rows).  Per chunk: detach (the Delete path's repair rebuilds every row that
 * points into the chunk, the chunk's own rows are emptied), overwrite,
 * re-insert (the batched insert's descend, search and commit over the chunk's
 * rows at their ids and levels).  While a chunk is detached its descents start
 * from a member outside it: in the highest layer that has one, the layer's
 * entry, else its lowest-id live member; rows of layers whose every member is
 * in the chunk get no links there.  A chunk's rows do not see each other, as a
 * batch of Add's do not; the link pass (option "batch_link") is not applied to
 * update chunks.
 *
 * BATCH and FLAT build modes (FLAT: the vector refresh of mhnsw_replace, no
 * links).  Errors leave the index, its maps and its Rng as they were:
 * MHNSW_EINVAL (a key repeated within the call, null pointers), MHNSW_EDIM,
 * MHNSW_EUNSUPPORTED on a COMPAT handle ("update needs a batch or flat
 * (build_mode 1 or 2) handle": there Add of a present key already replaces it)
 * and on one with a replaced or re-added key or with rows outside layer 0.
 * Exclusive like Add and Delete; enqueued searches finish first.
 * Read-only options, of the last update: "last_update_rows",
 * "last_update_chunks", "last_update_repaired" ((layer, row) pairs whose
 * adjacency was rebuilt because it pointed at an updated row) and, with
 * "time_build" 1 (else 0), "last_update_ns" = "last_update_detach_ns" +
 * "last_update_overwrite_ns" + "last_update_insert_ns" (device time). */
int mhnsw_update(mhnsw_index *h, const int64_t *keys, const float *vecs, int64_t n, int dim, uint8_t *out_found);
int mhnsw_update_device(mhnsw_index *h, const int64_t *keys, const float *d_vecs, int64_t n, int dim,
                        uint8_t *out_found);
/* edge distances as stored: layout of mhnsw_export's adj ([L*N*cap]), 0 where adj is -1 */
int mhnsw_export_edge_dist(mhnsw_index *h, float *adjd, int cap);

/* ---- Relink: mhnsw_update with each found row's stored vector ----
 * The graph around the found rows is detached and rebuilt exactly as an update
 * with their own vectors would do it -- the same export, stored edge
 * distances, out_found and "last_update_*" options, bit for bit -- but no
 * vector is sent, written or converted: the overwrite step is skipped.  The
 * remedy for rows that mhnsw_reachability reports.  Chunking, refusals,
 * messages and exclusivity are mhnsw_update's; on a FLAT handle the call only
 * fills out_found. */
int mhnsw_relink(mhnsw_index *h, const int64_t *keys, int64_t n, uint8_t *out_found);

/* ---- Analyzer (analyzer.go): quality metrics, degree histogram, hops, reachability ----
 * Graph inspection on the device: the calls read `deg` and `adj` only (and the
 * vectors of at most 100 sample rows), never a copy of the store.  They are
 * read-only: they hold the handle's lock shared, first wait for the last
 * enqueued *_device search as a mutation does, and serialise among themselves.
 * A row is a live member of layer l when its deg there is not -2 and it is not
 * deleted.  Every walk follows every stored edge (positions below deg, ids
 * >= 0), through deleted rows too; an id outside the store is skipped and the
 * call fails with MHNSW_EINTERNAL, "out-of-range node id in adjacency (graph
 * corrupt)".  A handle with a replaced or re-added key fails every call with
 * MHNSW_EUNSUPPORTED (the reference's BFS marks visits by key, the engine by
 * row); a FLAT handle fails all but the histogram with MHNSW_EUNSUPPORTED,
 * "analyzer needs a compat or batch (build_mode 0 or 1) handle".  Rows of up
 * to 255 neighbours.  Read-only option: "last_analyzer_scratch_bytes" (device
 * memory the calls keep: about 14 bytes per row of capacity for reachability,
 * 52 for hops). */

/* analyzer.go:69-90 GraphQualityMetrics */
typedef struct mhnsw_quality {
    int64_t node_count;          /* live layer-0 rows */
    double avg_connectivity;     /* analyzer.go:93-109: sum of their deg (below 0: 0) / node_count, the sum exact */
    double connectivity_std_dev; /* analyzer.go:112-130, see below */
    double distortion_ratio;     /* analyzer.go:135-189, see below */
    double layer_balance;        /* analyzer.go:245-279, on the host with pow() of libm (Go's math.Pow may differ
                                    in the last bit) */
    int64_t graph_height;        /* len(layers): mhnsw_num_layers */
} mhnsw_quality;
/* Analyzer.QualityMetrics (analyzer.go:51-67); all zero without layers.
 * connectivity_std_dev = sqrt(sum_d hist[d] (d - avg)^2 / node_count) in
 * double, d ascending over the exact layer-0 degree histogram (Go sums per
 * node in map order, which is random: this order is the engine's policy).
 * distortion_ratio: 0 below 10 live layer-0 rows; else the sample is the first
 * min(100, node_count) live layer-0 rows in ascending row id (Go takes what its
 * map yields first), and over the pairs i < j in that nested order with
 * h = hops(sample[i] -> sample[j], depth 10) > 0 and a finite canonical
 * distance a (q = sample[i]'s vector, X = sample[j]'s: the bits of
 * mhnsw_distance) the mean of double(h) / double(a), summed in pair order (a
 * zero distance gives +Inf, as in Go); 0 without such a pair. */
int mhnsw_quality_metrics(mhnsw_index *h, mhnsw_quality *out);
/* out[d], d < 64: live members of `layer` with degree d (below 0 counts as 0): the histogram
 * behind analyzer.go:93-130.  MHNSW_EUNSUPPORTED when a member has more than 63 neighbours. */
int mhnsw_degree_histogram(mhnsw_index *h, int layer, int64_t *out);
/* estimateGraphDistance (analyzer.go:193-240) for every ordered pair of n keys:
 * out[i * n + j] = edges on the shortest directed layer-0 path keys[i] ->
 * keys[j], 0 for i == j, -1 when none of at most max_depth edges exists (the
 * reference's fixed limit is 10).  1 <= n <= 128 (more: MHNSW_EUNSUPPORTED,
 * "hops supports at most 128 keys"), 1 <= max_depth <= 64; a key without a
 * live layer-0 row or a repeated key is MHNSW_EINVAL.  Arguments are checked
 * before the handle is used. */
int mhnsw_hops(mhnsw_index *h, const int64_t *keys, int n, int max_depth, int32_t *out);
/* Which rows a search can ever visit.  T = the highest layer with a live
 * member; R_T = the rows reachable in layer T from its entry (the export's
 * entry[T], where every search starts); below, R_l = the rows reachable in
 * layer l from R_(l+1)'s members of layer l.  Per layer l < max_layers (each
 * pointer nullable): members[l] = live members, reached[l] = those in R_l,
 * depth[l] = BFS levels run until the frontier emptied (0 without seeds).
 * *out_unreachable (nullable) = members[0] - reached[0].  Returns the number
 * of layers (>= 0) or an error.  mhnsw_unreachable_keys then copies the first
 * min(cap, that count) keys of the last call's unreachable live layer-0 rows,
 * in ascending row id.  Read-only option: "last_reach_ns" (device time, HIP
 * events). */
int mhnsw_reachability(mhnsw_index *h, int64_t *members, int64_t *reached, int32_t *depth, int max_layers,
                       int64_t *out_unreachable);
int mhnsw_unreachable_keys(mhnsw_index *h, int64_t *out_keys, int64_t cap);

/* ---- DistanceFunc (distance.go:12-23): batched sweep of one query over n rows ---- */
int mhnsw_distance(int metric, const float *q, const float *X, int64_t n, int dim, float *out);
int mhnsw_distance_device(int metric, const float *d_q, const float *d_X, int64_t n, int dim, float *d_out,
                          void *stream);

/* ---- graph exchange (CSR view of encode.go's layer/neighbour structure) ----
 * keys[N], vecs[N*dim], deg[L*N] (-2 absent, -1 nil map, >=0 degree),
 * adj[L*N*cap] internal ids (row-major, -1 padded), entry[L] (-1: empty
 * layer), dead[N] (1 = deleted row; nullable). */
int mhnsw_export_sizes(mhnsw_index *h, int64_t *N, int *dim, int *L, int *cap);
int mhnsw_export(mhnsw_index *h, int64_t *keys, float *vecs, int32_t *deg, int32_t *adj, int cap, int32_t *entry,
                 uint8_t *dead);
int mhnsw_import(mhnsw_index *h, int64_t N, int dim, int L, int cap, const int64_t *keys, const float *vecs,
                 const int32_t *deg, const int32_t *adj, const int32_t *entry, const uint8_t *dead);

/* ---- the reference's binary format (encode.go:128-262) and SavedGraph (encode.go:264-327) ----
 * key_kind = the Go key type K: MHNSW_KEY_INT (Go `int`, varint-encoded),
 * MHNSW_KEY_INT64 / _INT32 / _UINT64 / _UINT32 (fixed-width little-endian).
 * Export: *size receives the byte count; buf == NULL only sizes.  Nodes are
 * written in insertion order and neighbour keys ascending (Go: map order).
 * Import replaces the graph (M, Ml, EfSearch and the distance come from the
 * file) and reports the reference's errors ("unknown distance function %q",
 * "incompatible encoding version: %d", ...).  Save writes a unique temp file
 * next to path, fsyncs it and renames it over path (renameio, encode.go:320);
 * Load of a missing or empty file leaves the graph empty. */
enum { MHNSW_KEY_INT = 0, MHNSW_KEY_INT64 = 1, MHNSW_KEY_INT32 = 2, MHNSW_KEY_UINT64 = 3, MHNSW_KEY_UINT32 = 4,
       MHNSW_KEY_STRING = 5 /* Go string keys: the labels of mhnsw_strkeys_encode */ };
int mhnsw_export_go(mhnsw_index *h, int key_kind, uint8_t *buf, int64_t cap, int64_t *size);
int mhnsw_import_go(mhnsw_index *h, const uint8_t *buf, int64_t size, int key_kind);
int mhnsw_save(mhnsw_index *h, const char *path, int key_kind);
int mhnsw_load(mhnsw_index *h, const char *path, int key_kind);

/* levels randomLevel() would draw for the next n Adds (does not consume the RNG) */
int mhnsw_preview_levels(mhnsw_index *h, int64_t n, int32_t *out);

/* counters: [0] search distance evals, [1] search expansions, [2] visited-set
 * resets, [3] build distance evals, [4] build expansions, [5] dropped reverse
 * proposals, [6] searches issued, [7] exact-mode queries whose preselection
 * could not be certified and were redone by a full canonical sweep, [8] beam
 * candidates screened on the fp16 copy, [9] beam candidates evaluated in f32,
 * [10] batched-insert candidates screened on the fp16 copy, [11] batched-insert
 * rows read in f32 (search evaluations + neighbour-selection rows), [12]
 * device time of the batched insert's kernels (descent, layer searches,
 * commits) in microseconds (option "time_build" = 1: HIP events around each
 * layer's launches) */
int mhnsw_stats(const mhnsw_index *h, int64_t *out, int n);
int mhnsw_reset_stats(mhnsw_index *h);
/* device time of the last search's main kernel (HIP events on its stream) */
int mhnsw_last_kernel_ms(mhnsw_index *h, float *ms);

/* ---- Go string keys (Graph[string], graph.go:305 K = string) ----
 * The engine compares keys only by order (graph.go:137 expansion order, map
 * order stand-ins), so a string key travels as an int64 order label: every
 * string ever added gets a label and labels follow lexicographic (Go string)
 * order.  encode: n strings (blob + offs[n+1]) -> labels; with `assign` new
 * strings get labels (a new string between two adjacent labels may re-space
 * all labels: the stored keys are rewritten, so earlier labels go stale --
 * hosts convert at every call, never cache), without it unknown strings give
 * INT64_MIN.  decode: labels -> strings (blob + offs[n+1]); `need` = bytes;
 * blob == NULL or cap < need only reports `need`.  Unknown labels decode to
 * "".  Options "strkeys" / "strkey_relabels" report the table size and the
 * number of re-spacings. */
int mhnsw_strkeys_encode(mhnsw_index *h, const char *blob, const int64_t *offs, int64_t n, int assign,
                         int64_t *out);
int mhnsw_strkeys_decode(mhnsw_index *h, const int64_t *labels, int64_t n, char *blob, int64_t cap,
                         int64_t *offs, int64_t *need);

/* ---- multi-GPU: merge per-shard top-k lists (device pointers) ----
 * inputs [shards][B][k] (+ n_in [shards][B]); output best k by (dist, key). */
int mhnsw_merge_topk_device(const int64_t *keys_in, const float *dist_in, const int32_t *n_in, int shards,
                            int64_t B, int k, int64_t *out_keys, float *out_dist, int32_t *out_n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
