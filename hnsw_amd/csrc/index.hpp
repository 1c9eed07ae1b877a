// index.hpp -- the engine's per-handle host state (struct mhnsw_index) and the
// host helpers shared by the C ABI's translation units: api.cpp (lifecycle,
// options, Add / Delete / build scheduling), search_host.cpp (search and
// exact-path orchestration), io_host.cpp (export / import, encode.go format,
// string keys).  Host only: no device code here.
#pragma once
#include <hip/hip_runtime.h>

#include <errno.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <functional>
#include <unordered_map>
#include <vector>

#include "../../include/mhnsw.h"
#include "codec.hpp"
#include "engine.hpp"

using namespace mh;

// defaults of "search_order" / "search_order_min_b" (measured: DESIGN.md "Query order")
#ifndef MH_SEARCH_ORDER_DEFAULT
#define MH_SEARCH_ORDER_DEFAULT 1
#endif
#ifndef MH_SEARCH_ORDER_MIN_B_DEFAULT
#define MH_SEARCH_ORDER_MIN_B_DEFAULT 16384
#endif

namespace mhh {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
};

struct Layer {
    int32_t* deg = nullptr;
    int32_t* adj = nullptr;
    float* adjd = nullptr;
    int cap = 0;
    int64_t count = 0;
    int32_t entry = -1;
};

}  // namespace mhh

using mhh::DevBuf;
using mhh::Layer;

struct mhnsw_index {
    // public fields (graph.go:305-326)
    int metric = COSINE;
    int M = 16;
    double ml = 0.25;
    int ef = 20;
    uint64_t rng = 0;
    // engine options
    int build_mode = MHNSW_BUILD_COMPAT;
    int m0 = 0;  // 0 => 2*M in batch mode, M in compat mode
    int efc = 0; // 0 => EfSearch
    int heuristic = 1;
    int keep_pruned = 0;
    int build_expand = 4;     // batched insert: entries expanded per step of its layer searches (1-4)
    int upper_efc = 0;        // batched insert: candidate list of the layers above 0 (0 = efConstruction)
    int search_expand = 1;    // beam search: entries expanded per layer-0 step (1, 2, 4; 1 = standard)
    int alpha_pct = 100;
    int batch_min = 1, batch_max = 65536, batch_ratio_pct = 5;
    int vis_log2 = 12;
    int vis_entries = 0;      // beam search's visited set; 0 = 1.25 * 2^vis_log2 (beam_vis_entries)
    int vis_compact = 1;      // beam search: the compact 16-bit visited set when ids < 2^24 and it fits
    int exact_kk = 0;
    int exact_sample = 64;   // fused preselection: row tiles in the threshold sample (at most; stride = ceil(tiles / this))
    int exact_thr_rank = 0;  // fused preselection: the sample's J-th best is the threshold (0 = max(k, kk / 8))
    int exact_precision = 3;  // scores: 0 f32-input MFMA, 1 bf16x3 split, 2 fp16 2-product split,
                              // 3 fp16 1-product with the fused preselection (all certified, same results)
    int exact_tile = 0;       // GEMM variant (exact.hip: launch_split_scores, launch_h1)
    int compat_waves = 8;     // compat insert: waves scoring each distance batch (1 = the walking wave alone)
    int upper_ef = 1;         // beam search: upper-layer descent width
    int64_t beam_mw_max_b = 512;  // beam search: batches up to this size run one workgroup of 4 waves per query
    int beam_lds_min_ef = 513;    // beam search: the smallest max(ef, k) whose layer-0 list lives in LDS ([65, 513])
    // beam search, ordered path: batches of at least search_order_min_b queries (the one-wave
    // kernels only) run the descent as a pre-pass, sort the queries by descent path and search
    // layer 0 in that order (DESIGN.md "Query order"); the same results either way
    int search_order = MH_SEARCH_ORDER_DEFAULT;
    int64_t search_order_min_b = MH_SEARCH_ORDER_MIN_B_DEFAULT;
    int search_order_top = 0;     // highest layer in the sort key (0 = by batch size, search_host.cpp order_key_top)
    int search_order_fields = 0;  // layers in the sort key (0 = search_host.cpp ORDER_KEY_FIELDS)
    int search_order_map = 0;    // 0: XCD-contiguous chunks of the sorted queries, 1: workgroup i takes position i
    int64_t build_mw_max = 256;  // batched insert: launches of at most this many inserts run 4 waves per insert
    int screen = 1;           // beam search / batched insert fp16 screening copy (results unchanged)
    int fuse_descent = 1;     // batched insert: all greedy descents of a batch in one launch (same graph)
    int time_build = 0;       // batched insert: time its search kernels with HIP events (stats [12])
    int batch_link = 0;       // batched insert: after a layer's commit the batch's rows search it again and link to each other
    int batch_link_ef = 0;    // ... the width of that search (0 = the layer's insert width; else clamped to [row cap, 512])
    int64_t max_rows = 0;     // row capacity limit (0 = none): an Add past it fails with MHNSW_ENOMEM, index unchanged
    std::vector<hipEvent_t> tev;  // event pairs around the timed launches of the current Add
    size_t tev_used = 0;
    std::vector<hipEvent_t> ltev;  // ... and around its link passes
    size_t ltev_used = 0;
    double build_search_us = 0;
    // link pass: staged rows of the current batch (run_build_batch sizes them like `touched`), the device
    // counters {rows staged, batch-mates written} and, of the last Add, their sums and the kernels' time
    int32_t* link_adj = nullptr;
    float* link_adjd = nullptr;
    int32_t* link_deg = nullptr;
    size_t link_cap = 0;  // rows staged at most
    int link_stride = 0;
    unsigned long long* link_cnt = nullptr;
    int64_t link_rows = 0, link_edges = 0;
    double link_us = 0;
    // shape
    int dim = 0, pitch = 0, lpr = 0, vpl = 0;
    bool layers_exist = false;
    int64_t n = 0, capn = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    // device state
    float* vecs = nullptr;
    float* norms = nullptr;
    uint16_t* h16 = nullptr;  // fp16 screening copy [capn * pitch] (screen = 1)
    float2* h16aux = nullptr;  // [capn] L2 screening {unscale, |x|}
    int h16_metric = -1;       // metric the copies were written for
    float* h16err = nullptr;   // [1] the copy's measured max relative rounding (screening margin)
    int64_t* keys = nullptr;
    int32_t* levels = nullptr;
    uint8_t* dead = nullptr;  // [capn] deleted rows (graph.go:843-864)
    bool any_dead = false;
    // key identity (compat; GraphDev::kid): allocated at the first replaced or re-added key
    int32_t* kid = nullptr;      // [capn] first row that held the row's key
    int32_t* kidlive = nullptr;  // [capn] by kid: the key's newest live row (-1 none)
    int32_t* kprev = nullptr;    // [capn] the next older live row of the same key (-1 none; GraphDev::kprev)
    bool aliased = false;
    uint32_t* cur_entry = nullptr;
    int32_t* inc_cnt = nullptr;
    uint32_t* inc_src = nullptr;
    float* inc_dist = nullptr;
    int inc_cap = 64;
    uint32_t* touched = nullptr;
    size_t touched_cap = 0;
    int32_t* touched_cnt = nullptr;
    int32_t* d_layer_entry = nullptr;
    LayerDev* d_layers = nullptr;
    LayerDev layers_host[MH_MAXL] = {};
    unsigned long long* d_stats = nullptr;
    // d_err[0]: error word of the current synchronous call (zeroed per call);
    // d_err[1]: sticky word of *_device searches, which return before their
    // kernels run -- read and cleared by mhnsw_device_status
    int* d_err = nullptr;
    std::vector<mhh::Layer> layers;
    // scratch
    DevBuf<float> qpad, qnorm, scores, tmp;
    DevBuf<uint32_t> cand;
    DevBuf<uint32_t> border;           // batched insert: batch nodes by level, descending
    uint32_t* ord_pin = nullptr;       // ... staged in pinned memory
    int64_t ord_cap = 0;
    hipEvent_t ord_ev = nullptr;       // the staging copy has been consumed
    bool ord_pending = false;
    DevBuf<int64_t> okeys;
    DevBuf<float> odist;
    DevBuf<int32_t> on;
    // ordered beam search: sort keys in / out [2 B], {query index, order, layer-0 entry} [3 B] and the pre-pass's
    // counters per query [4 B], sort scratch
    DevBuf<unsigned long long> ordkey;
    DevBuf<uint32_t> ordval;
    DevBuf<uint8_t> ordtmp;
    DevBuf<float> nq, nneg, ncd;  // negatives: queries, padded negative rows, candidate distances
    DevBuf<int64_t> nck, nok;
    DevBuf<int32_t> ncn, nci, noff, non;
    DevBuf<float> nos;
    // exact path: cached bf16 hi/lo planes of the first xsplit_rows rows (rows are
    // immutable once added; import resets), per-chunk query planes, certificate state
    DevBuf<uint16_t> xsplit, qsplit;
    int64_t xsplit_rows = 0, xsplit_plane = 0;  // rows converted; plane stride they were written with
    int xsplit_kind = 0;                        // 1: bf16 hi/lo planes, 2: fp16 hi plane + xinv (exact_precision)
    DevBuf<float> xinv, qinv;                   // exact_precision 2: per-row / per-query unscale
    DevBuf<float> xerr;                         // ... and the rows' max relative fp16 rounding
    // exact_precision 3 (fp16 1-product, fused preselection): sample thresholds,
    // filter constants, tile regions + counts, per-query buckets, the queries' rounding
    DevBuf<float> h1thr, h1c, h1s, qerr;
    DevBuf<float> h1xw;  // [4 capn] per-row filter constants of k_h1_pp16 (k_h1_rowconst)
    DevBuf<uint2> h1region, h1bucket;
    DevBuf<int32_t> h1rcnt, h1qcnt;
    DevBuf<uint8_t> h1ovf;
    DevBuf<float> xbound, xmaxn, xsegd;
    DevBuf<uint32_t> xsegi;
    DevBuf<uint8_t> xflag;
    DevBuf<uint8_t> xgone;     // exact path: rows to skip when some live row is not in layer 0
    int64_t add_reached = 0;   // inserts the last Add's walk reached (mhnsw_add_reached)
    int64_t partial_rows = 0;  // rows neither deleted nor in layer 0 (left by failed inserts, graph.go:1009)
    uint64_t mut_epoch = 0;            // bumped by every Add / Delete / Import: row membership may have changed
    uint64_t xgone_epoch = ~0ull;      // the epoch xgone was built at
    DevBuf<int32_t> xflagged, xnflag;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t gev0 = nullptr, gev1 = nullptr;  // the exact path's score GEMM (first query chunk)
    bool have_gemm_timing = false;
    // cross-stream ordering: a *_device search returns once enqueued on the
    // caller's stream; the next call on another stream (or a mutation) must
    // not reuse scratch / rewrite the graph under it
    hipEvent_t scr_ev = nullptr, meta_ev = nullptr;
    hipStream_t scr_stream = nullptr;
    bool scr_valid = false;
    bool have_timing = false;
    // host mirrors
    std::unordered_map<int64_t, int32_t> key2id;  // live keys only
    // Go string keys (Graph[string]): order-maintenance labels -- every string
    // ever added maps to an int64 label in lexicographic order, so the engine's
    // key comparisons (compat expansion order, tie-breaks) see the string order
    std::map<std::string, int64_t> s2l;
    std::unordered_map<int64_t, std::string> l2s;
    int64_t relabels = 0;
    std::vector<int32_t> hlevels;
    std::vector<uint32_t> hmask;  // bit l: row is in layer l (compat may promote into emptied layers)
    std::vector<uint8_t> hdead;
    std::vector<int32_t> hkid;                       // kid mirror (aliased only)
    std::vector<int32_t> hprev;                      // kprev mirror (aliased only)
    std::unordered_map<int64_t, int32_t> dead_kid;   // deleted keys -> kid, for a later re-add
    int64_t stats_host[8] = {0};
    // filtered search: per-query allow-lists (mhnsw_filter_*), slot = filter id.
    // A bitmap is row id -> bit over the row capacity; it grows zero-filled with
    // the rows (filters_fit), and Import / Load drop every filter (the ids change).
    struct Filter {
        bool used = false;
        std::vector<uint32_t> bits;  // host mirror, the words the device bitmap holds
        uint32_t* d = nullptr;
    };
    std::vector<Filter> filters;
    const uint32_t** d_filters = nullptr;  // [MHNSW_MAX_FILTERS] device table of the bitmaps (nullptr: none)
    bool filters_dirty = false;            // the table is to be uploaded
    int filter_route = 1024;               // route width of a filtered search that names none
    DevBuf<int32_t> fof;                   // a host-pointer filtered search's filter_of
    // filtered exact search (rowset.hip): the allowed rows of the call's filter as a row set --
    // bitmap words, per-block counts, row mask of the fallback, the ascending ids, their rows
    // of the fp16 plane and those rows' unscale / norm.  Grow-only, rebuilt by every call.
    DevBuf<uint32_t> fxwords, fxcnt, fxids;
    DevBuf<uint8_t> fxmask;
    DevBuf<uint16_t> fxplane;
    DevBuf<float> fxinv, fxnorm;
    // stage marks of the last filtered exact search: start, compaction done, gather done, and
    // around the first query chunk's re-rank and fallback (options "last_fx_*_ns")
    // ([6..8]: a filtered exact-mode range search's row set -- start, compaction done, gather done)
    hipEvent_t fxev[9] = {};
    bool have_fx_timing = false;
    bool have_rs_timing = false;
    // range search (range.hip): per-chunk thresholds, query states and counts, the call's hit
    // buffer (unsorted and sorted halves), sort segments and temporary storage, the counters of
    // the last call, and a host-pointer call's radii, prefix and results (mhnsw_range_results)
    int64_t range_expect = 64;     // expected hits per query: sizes the filter's regions and sub-buckets
    int range_force_fallback = 0;  // test option: every query takes the canonical sweep
    DevBuf<float> rthr, rrad, rdist;
    DevBuf<uint8_t> rstate, rsweep, rtmp;
    DevBuf<int32_t> rcnt, rcursor;
    DevBuf<uint32_t> rseg;
    DevBuf<unsigned long long> rhits, rstat;
    DevBuf<int64_t> rlims, rkeys;
    // a host filtered range search of several filters: the passes' hits, and each query's offset in them
    DevBuf<int64_t> rgkeys, rgoff;
    DevBuf<float> rgdist;
    int64_t range_total = -1;  // hits the last host-pointer range search left in rkeys / rdist (-1: none)
    bool have_range_stats = false;
    bool have_range_timing = false;  // fxev holds an exact-mode range search's stage marks (options "last_range_*_ns")
    // wide exact search (wide.hip; search_host.cpp wide_exact): exact mode past k 256 through the
    // range pipeline.  The call's radii, prefix, short-query list and counters {short queries,
    // hits that reached the sort}, the fallback's distance rows; stage marks of the last timed
    // call (created on first use): sample start, sample end, radius end, the first chunk's range
    // stages end, sort start, cut end, fallback end (options "last_wide_*_ns")
    int exact_wide = 0;            // 1: exact mode accepts k <= 4096
    int exact_wide_min_k = 257;    // the smallest k that takes the wide path (k > 256 always does)
    int wide_force_fallback = 0;   // test option: every query is answered by the fallback select
    int64_t wide_fallback_bytes = (int64_t)1 << 30;  // the fallback's distance rows: queries per group = this / (4 rows)
    DevBuf<float> wrad, wdist;
    DevBuf<int64_t> wlims;
    DevBuf<int32_t> wshort;
    DevBuf<unsigned long long> wstat;
    hipEvent_t wev[7] = {};
    bool have_wide_timing = false;
    int64_t wide_queries = 0;      // queries of the last exact search that took the wide path
    int64_t wide_room = 0, wide_rank = 0;  // ... its hit-buffer entries per query and its sample rank J
    // compaction (mhnsw_compact): rows per staged chunk (measured default: DESIGN.md §6 "Compaction"),
    // and of the last call its event pair, device allocations and dropped edges to deleted rows
    int64_t compact_stage_rows = 16384;
    hipEvent_t cev0 = nullptr, cev1 = nullptr;
    bool have_compact_timing = false;
    int64_t compact_scratch_bytes = 0, compact_dangling = 0;
    // in-place update (mhnsw_update): of the last call the rows updated, its chunks, the (layer, row)
    // pairs the detach rebuilt and, with time_build, the device time of its three steps (detach,
    // overwrite, re-insert); the id list and repair counter on the device, the steps' events
    int64_t update_rows = 0, update_chunks = 0, update_repaired = 0;
    double update_us[3] = {0, 0, 0};
    DevBuf<uint32_t> uids;
    unsigned long long* d_repaired = nullptr;
    std::vector<hipEvent_t> uev;
    // analyzer (analyze_host.cpp), grow-only: the reachability BFS's bitmaps (visited, unreachable),
    // its two queues, the compaction's workspace and id list, the counters; the hop BFS's masks,
    // source index and matrix; the sample rows and their distances.  The calls hold `mu` shared
    // and an_mu for this state; of the last reachability the events and the unreachable keys.
    DevBuf<uint32_t> an_bits, an_q, an_ids, an_blk, an_hm;
    DevBuf<uint8_t> an_mask;
    DevBuf<int32_t> an_sidx, an_hops;
    DevBuf<unsigned long long> an_cnt;
    DevBuf<int64_t> an_keys;
    DevBuf<float> an_rows, an_dist;
    hipEvent_t aev0 = nullptr, aev1 = nullptr;
    bool have_reach_timing = false;
    std::vector<int64_t> an_unreach;
    std::mutex an_mu;
    std::string err;
    mutable std::shared_mutex mu;
};

namespace mhh {

extern thread_local std::string g_create_err;

#define HIPCHK(h, x)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) return fail(h, MHNSW_EDEVICE, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

#define LCHK(h, x)                                                              \
    do {                                                                        \
        int r_ = (x);                                                           \
        if (r_ != 0) return fail(h, r_ == -4 ? MHNSW_EUNSUPPORTED : MHNSW_EDEVICE, "kernel launch failed (%d) at %s", r_, #x); \
    } while (0)

int fail(mhnsw_index* h, int code, const char* fmt, ...);
int validate(mhnsw_index* h);
int max_level(double ml, int64_t num);
double rng_next(uint64_t* s);
int random_level(double ml, bool layers_exist, int64_t count, uint64_t* rng);
int m0_of(const mhnsw_index* h);
int cap_of(const mhnsw_index* h, int l);
int ensure_layer(mhnsw_index* h, int l);
int ensure_caps(mhnsw_index* h);
int ensure_capacity(mhnsw_index* h, int64_t need);
int sync_layer_table(mhnsw_index* h);
GraphDev graph_view(const mhnsw_index* h);
int64_t live_count(const mhnsw_index* h);
int top_live_layer(const mhnsw_index* h);
bool in_layer(const mhnsw_index* h, int64_t id, int l);
void fix_entries(mhnsw_index* h);
int set_shape(mhnsw_index* h, int dim);
int set_deg(mhnsw_index* h, int l, int64_t id, int32_t v);
int sync_layer_entries(mhnsw_index* h);
int zero_err(mhnsw_index* h);
int run_batch_layers(mhnsw_index* h, int64_t a0, int64_t a1, int top, uint32_t entry, const uint32_t* rows = nullptr);
int ensure_batch_scratch(mhnsw_index* h);
int collect_build_times(mhnsw_index* h);
int run_build_batch(mhnsw_index* h, int64_t n0, int64_t n1, int top, uint32_t entry,
                    const std::function<void()>& while_gpu = nullptr);
int h16_rows(mhnsw_index* h, int64_t r0, int64_t r1);
int32_t kid_of_row(const mhnsw_index* h, int64_t r);
int set_kidlive(mhnsw_index* h, int32_t kid, int32_t row);
int start_alias(mhnsw_index* h);
void forget_key(mhnsw_index* h, int64_t key, int32_t row);
std::vector<int32_t> key_rows(const mhnsw_index* h, int64_t key);
int32_t key_row_in(const mhnsw_index* h, int64_t key, int l);
int add_step(mhnsw_index* h, const int64_t* keys, const float* vecs, bool vecs_on_device, int64_t n, int dim, const int32_t* levels, int64_t* reached, int64_t* cont_out);
int add_impl(mhnsw_index* h, const int64_t* keys, const float* vecs, bool vecs_on_device, int64_t n, int dim, const int32_t* levels);
int beam_vis_entries(const mhnsw_index* h);
int drain(mhnsw_index* h);
int search_impl(mhnsw_index* h, const float* queries, bool on_device, int64_t B, int dim, int k, int mode, int ef, const int64_t* entry_key, int64_t* okeys, float* odist, int32_t* on, hipStream_t s, bool timing, int32_t* out_ids = nullptr, bool sticky = false);
int device_error(mhnsw_index* h, int err);
int exact_k_check(mhnsw_index* h, int k);  // exact mode's limit on k (256, or 4096 with "exact_wide")
void reset_graph(mhnsw_index* h);
constexpr int MHNSW_MAX_FILTERS = 1024;
void drop_filters(mhnsw_index* h);
int filters_fit(mhnsw_index* h);
int search_filtered_impl(mhnsw_index* h, const float* queries, bool on_device, int64_t B, int dim, int k, int ef, int route, const int32_t* filter_of, int64_t* okeys, float* odist, int32_t* on, hipStream_t s, bool sticky);
int search_filtered_exact_impl(mhnsw_index* h, const float* queries, bool on_device, int64_t B, int dim, int k, int filter, int64_t* okeys, float* odist, int32_t* on, hipStream_t s, bool sticky);
int range_search_impl(mhnsw_index* h, const float* queries, int64_t B, int dim, const float* radius, int mode, int ef, int64_t* out_lims);
int range_search_device_impl(mhnsw_index* h, const float* d_queries, int64_t B, int dim, const float* d_radius, int mode, int ef, int64_t cap, int64_t* d_lims, int64_t* d_keys, float* d_dist, hipStream_t s);
int range_search_filtered_impl(mhnsw_index* h, const float* queries, int64_t B, int dim, const float* radius, int mode, int ef, int route, const int32_t* filter_of, int64_t* out_lims);
int range_search_filtered_device_impl(mhnsw_index* h, const float* d_queries, int64_t B, int dim, const float* d_radius, int mode, int ef, int route, int filter, int64_t cap, int64_t* d_lims, int64_t* d_keys, float* d_dist, hipStream_t s);
int import_csr(mhnsw_index* h, int64_t N, int dim, int L, int cap, const int64_t* keys, const float* vecs, const int32_t* deg, const int32_t* adj, const int32_t* entry, const uint8_t* dead);
const char* metric_name(int m);
int strkey_relabel(mhnsw_index* h);
int strkey_insert(mhnsw_index* h, const std::string& s);
void strkey_table(mhnsw_index* h, const std::vector<std::string>& strs, std::vector<int64_t>& lab);
bool key_fits(const mhnsw_index* h, int64_t k, int kind);
int export_go(mhnsw_index* h, int key_kind, std::vector<uint8_t>& out);
int import_go(mhnsw_index* h, const uint8_t* buf, int64_t size, int key_kind);


template <class T>
int ensure_buf(mhnsw_index* h, DevBuf<T>& b, size_t n) {
    if (b.n >= n) return 0;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.n = 0;
    size_t want = std::max(n, b.n * 2);
    if (hipMalloc(&b.p, want * sizeof(T)) != hipSuccess) return fail(h, MHNSW_ENOMEM, "device allocation of %zu bytes failed", want * sizeof(T));
    b.n = want;
    return 0;
}

template <class T>
int grow(mhnsw_index* h, T*& p, int64_t old_elems, int64_t new_elems, int fill_byte, bool fill32 = false,
         uint32_t fill_val = 0) {
    T* np = nullptr;
    if (hipMalloc(&np, (size_t)new_elems * sizeof(T)) != hipSuccess)
        return fail(h, MHNSW_ENOMEM, "device allocation of %lld bytes failed", (long long)(new_elems * sizeof(T)));
    if (fill32)
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)np, (int)fill_val, (size_t)new_elems * sizeof(T) / 4, h->stream));
    else if (fill_byte >= 0)
        HIPCHK(h, hipMemsetAsync(np, fill_byte, (size_t)new_elems * sizeof(T), h->stream));
    if (p && old_elems > 0) HIPCHK(h, hipMemcpyAsync(np, p, (size_t)old_elems * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    if (p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        (void)hipFree(p);
    }
    p = np;
    return 0;
}

}  // namespace mhh
