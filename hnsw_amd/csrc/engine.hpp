// engine.hpp -- host-side launch interface between the C ABI (api.cpp) and the
// HIP kernels (search.hip, build.hip, exact.hip and the *_units.hip).  No torch types anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"

namespace mh {

// supported dimension configurations (lanes per row, float4 per lane)
struct DimCfgId {
    int lpr, vpl;
};
inline bool pick_cfg(int dim, int& lpr, int& vpl) {
    if (dim <= 0) return false;
    if (dim <= 64) { lpr = 16; vpl = 1; return true; }
    if (dim <= 128) { lpr = 32; vpl = 1; return true; }
    if (dim <= 256) { lpr = 64; vpl = 1; return true; }
    if (dim <= 512) { lpr = 64; vpl = 2; return true; }
    if (dim <= 768) { lpr = 64; vpl = 3; return true; }
    if (dim <= 1024) { lpr = 64; vpl = 4; return true; }
    if (dim <= 1536) { lpr = 64; vpl = 6; return true; }
    if (dim <= 2048) { lpr = 64; vpl = 8; return true; }
    if (dim <= 3072) { lpr = 64; vpl = 12; return true; }
    if (dim <= 4096) { lpr = 64; vpl = 16; return true; }
    return false;
}
inline int pitch_of(int lpr, int vpl) { return lpr * 4 * vpl; }

// The same configurations as X(lpr, vpl, G), for the code that instantiates or
// selects a kernel per configuration.  G: the group width, rows in flight per
// wave step.  In four groups: the units of beam_units.hip, walks_units.hip and
// build_units.hip each instantiate one or two of them, so that they compile in
// parallel.
#define MH_CFGS_A(X) X(16, 1, 2) X(32, 1, 4) X(64, 1, 8)
#define MH_CFGS_B(X) X(64, 2, 8) X(64, 3, 8)
#define MH_CFGS_C(X) X(64, 4, 4) X(64, 6, 4)
#define MH_CFGS_D(X) X(64, 8, 2) X(64, 12, 1) X(64, 16, 1)
#define MH_FOR_EACH_CFG(X) MH_CFGS_A(X) MH_CFGS_B(X) MH_CFGS_C(X) MH_CFGS_D(X)

// f(DimCfg<L, V, G>()) for the configuration (lpr, vpl) of the table; -3: not in it
template <int L_, int V_, int G_>
struct DimCfg {
    static constexpr int L = L_, V = V_, G = G_;
};
template <class F>
int with_cfg(int lpr, int vpl, F&& f) {
#define X_(L, V, G) \
    if (lpr == L && vpl == V) return f(DimCfg<L, V, G>());
    MH_FOR_EACH_CFG(X_)
#undef X_
    return -3;
}
// group width G of configuration (L, V), from the table (0: not in it)
template <int L, int V>
constexpr int cfg_group() {
#define X_(L_, V_, G_) \
    if (L == L_ && V == V_) return G_;
    MH_FOR_EACH_CFG(X_)
#undef X_
    return 0;
}

// one launch of a kernel that takes the argument struct `a`: grid workgroups, lds_words 32-bit words of dynamic LDS
template <class K, class A>
int launch_grid(K kernel, int64_t grid, int block, int lds_words, const A& a, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), (size_t)4 * (size_t)lds_words, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

struct SearchArgs {
    GraphDev g;
    const float* q;  // padded queries [B * pitch]
    int64_t B;
    int k, ef, top;
    uint32_t entry;               // top-layer entry (internal id)
    const int32_t* layer_entry;   // [nlayers] policy entry per layer (compat)
    int64_t* out_keys;            // [B*k]
    float* out_dist;              // [B*k]
    int32_t* out_n;               // [B]
    int32_t* out_ids;             // [B*k] internal ids (nullable)
    unsigned long long* stats;    // [0]=dist evals [1]=expansions [2]=visited resets
                                  // [8]=rows screened in fp16 [9]=rows evaluated in f32 (beam)
    int* err;                     // set to nonzero on visited overflow (compat)
    int vis_log2;                 // compat: 2^vis_log2-entry visited set
    int vis_n;                    // beam: visited-set entries (the LDS it takes: 4 * vis_n bytes per wave)
    int vis16 = 0;                // beam: the compact 16-bit set in that LDS instead (ids < 2^24)
    int upper_ef;                 // beam: width of the upper-layer descent (1 = greedy, the reference's k = 1)
    int64_t mw_max_b;             // beam: batches up to this size run a workgroup per query (0 = never)
    int expand = 1;               // beam: entries expanded per layer-0 step (1, 2 or 4; beam_layer XW)
    int lds_min_ef = 513;         // beam: the smallest max(ef, k) whose layer-0 list lives in LDS (k_search_beam_lds)
    // beam, ordered path (option "search_order"): the descent through the layers
    // of the sort key and above runs as a pre-pass (k_beam_descend) that writes
    // ep0 / okey / oidx; the keys are sorted into `order`, and the layer-0
    // kernels take their query from it and finish its descent (nullptr: the
    // fused path, workgroup b runs query b with its whole descent)
    const uint32_t* order = nullptr;     // [B] sorted position -> query
    uint32_t* ep0 = nullptr;             // [B] the node each query's pre-pass stopped on (beam.hpp beam_order_lo)
    unsigned long long* okey = nullptr;  // [B] sort key: the descent's nodes of layers key_top .. key_top - key_n + 1
    uint32_t* oidx = nullptr;            // [B] 0 .. B - 1 (the sort's values)
    uint32_t* pstat = nullptr;           // [4 * B], 16-byte aligned: each query's pre-pass counters (E, X, S, F),
                                         // summed into stats after the pre-pass (search.hip k_beam_descend_stats)
    int key_top = 0, key_n = 0;          // the layers in the key (key_n = 0: every key is 0)
    int key_id_bits = 1;                 // bits per field of the key (in [1, 31])
    int key_hash = 0;                    // the fields are narrower than a node id: they hold a hash of it
    int64_t order_chunk = 0;             // > 0: workgroup i takes position (i % 8) * chunk + i / 8; 0: position i
};

// Filtered beam search (beam.hpp k_search_beam_filt): the second kernel
// argument.  With it SearchArgs::ef is the route width W (the layer-0 list the
// search routes through, in LDS) and `ef` here the result width max(ef, k).
struct FilterArgs {
    const uint32_t* const* filters;  // [nslots] a filter's bitmap, row id -> bit (nullptr: no such filter)
    int nslots;
    int ef;                          // max(ef, k) <= 128
    const int32_t* filter_of;        // [B] query b's filter (-1: every live row)
};

// the launch that runs one workgroup of 4 waves per query (beam.hpp
// k_search_beam_mw): small batches of the standard search on the narrow lists
inline bool beam_small_batch(const SearchArgs& a) {
    const int efl = a.ef > a.k ? a.ef : a.k;
    return a.expand != 2 && a.expand != 4 && efl <= 128 && efl < a.lds_min_ef && a.B <= a.mw_max_b;
}
// workgroups of an ordered layer-0 launch
inline int64_t beam_order_grid(const SearchArgs& a) { return a.order_chunk > 0 ? 8 * a.order_chunk : a.B; }

// negative-example re-ranking epilogue (graph.go:1116-1537)
struct NegArgs {
    GraphDev g;
    const float* neg;          // padded negative rows [total * pitch]
    const int32_t* neg_off;    // [B + 1] row offsets of each query's negatives
    const int32_t* cand_ids;   // [B * kx] Search(near, kx) internal ids
    const float* cand_d;       // [B * kx] their distances to the query
    const int32_t* cand_n;     // [B]
    int64_t B;
    int kx, k;
    float w;
    int flags;                 // bit 0: the reference's key 7..9 boost (test hack)
    int64_t* out_keys;         // [B * k]
    float* out_score;          // [B * k]
    int32_t* out_n;            // [B]
};
constexpr int NEG_MAX_CAND = 256;
int launch_negatives(const NegArgs& a, int lpr, int vpl, hipStream_t s);

int launch_pad_rows(const float* src, int64_t n, int dim, float* dst, int pitch, hipStream_t s);
int launch_scatter_rows(const float* src, const int32_t* ids, int64_t n, int pitch, float* dst, hipStream_t s);
// err: running max of the rows' measured relative rounding (GraphDev::h16err)
int launch_h16_rows(const float* X, const float* norms, int64_t n0, int64_t n1, int pitch, int metric, uint16_t* H,
                    float2* aux, float* err, hipStream_t s);
int launch_norms(const float* X, int64_t n0, int64_t n1, int pitch, int lpr, int vpl, float* out, hipStream_t s);
// the same kernels over a list of rows, ids[0 .. m) (the in-place update: work proportional to m)
int launch_norms_ids(const float* X, const uint32_t* ids, int64_t m, int pitch, int lpr, int vpl, float* out,
                     hipStream_t s);
int launch_h16_rows_ids(const float* X, const float* norms, const uint32_t* ids, int64_t m, int pitch, int metric,
                        uint16_t* H, float2* aux, float* err, hipStream_t s);
int launch_sweep(const float* q, const float* X, int64_t n, int pitch, int lpr, int vpl, int metric, float* out,
                 hipStream_t s);
int launch_sweep_raw(const float* q, const float* X, int64_t n, int dim, int metric, float* out, hipStream_t s);
int launch_search_beam(const SearchArgs& a, int lpr, int vpl, hipStream_t s);
int launch_search_beam_filtered(const SearchArgs& a, const FilterArgs& f, int lpr, int vpl, hipStream_t s);
// ordered path: the descent pre-pass (writes a.ep0 / a.okey / a.oidx, adds its
// counters to a.stats), then the sort of the keys into the permutation (order.hip)
int launch_beam_descend(const SearchArgs& a, int lpr, int vpl, hipStream_t s);
int order_sort_temp_bytes(int64_t n, size_t* bytes);
int launch_order_sort(const unsigned long long* keys, unsigned long long* keys_sorted, const uint32_t* idx,
                      uint32_t* order, int64_t n, int key_bits, void* temp, size_t temp_bytes, hipStream_t s);
int launch_search_compat(const SearchArgs& a, int lpr, int vpl, hipStream_t s);

// ---- build ----
struct CompatBuildArgs {
    GraphDev g;
    int64_t n0, n1;               // insert internal ids [n0, n1) in order
    const int32_t* levels;        // [cap_nodes] level of each node
    const int32_t* layer_entry;   // [MH_MAXL] first node id of each layer (-1 none)
    int top0;                     // len(g.layers) - 1 before this batch (-1: no layers)
    int M, ef;
    unsigned long long* stats;    // [0]=dist evals [1]=expansions
    int* err;                     // [0] error bits; on "no nodes found" (bit 2): [2] layer, [3] row
    int vis_log2;
    // BatchAdd of a present key (graph.go:1015-1024), after the fresh inserts:
    int rep_level;                // its level (-1: none)
    int rep_i0;                   // the layer whose search precedes the sweep
    uint32_t rep_a, rep_b;        // its rows above i0 (EMPTY_ID: none needed) / from i0 down
    const int32_t* rep_entry;     // [MH_MAXL] entry() of each layer at its turn (the row itself: empty then)
    const int32_t* rep_sweep;     // [MH_MAXL] row the sweep deletes + isolates in layer l (-1 none)
    int spec;                     // set by the launch: the eviction-staging area fits in LDS
};
int launch_build_compat(const CompatBuildArgs& a, int lpr, int vpl, int waves, hipStream_t s);  // waves: 1 or 8

// ---- delete (graph.go:843-895) ----
struct DeleteArgs {
    GraphDev g;
    const uint32_t* ids;          // compat: internal ids in BatchDelete order ...
    const uint32_t* lay;          // ... each isolated in layer lay[i] only (graph.go:852-861 walks a key's
                                  //     layers; a key's nodes can be several rows in disjoint layers)
    int64_t nids;
    int64_t n;                    // repair: rows [0, n)
    int layer;                    // repair: layer being repaired
    int M;                        // compat: the reference's cap (M on every layer)
    int mcap;                     // repair: row cap of this layer
    int heuristic, keep_pruned;   // repair: selection rule (as the batched insert)
    unsigned long long* stats;    // [0]=dist evals
    int* err;
    int vis_log2;
    unsigned long long* repaired;  // repair (nullable): += rows rebuilt (the in-place update's detach counts them)
};
constexpr int REPAIR_POOL = 256;  // candidate pool per repaired row (oracle: OG_REPAIR_POOL)
int launch_delete_compat(const DeleteArgs& a, int lpr, int vpl, hipStream_t s);
int launch_delete_repair(const DeleteArgs& a, int lpr, int vpl, hipStream_t s);

struct BatchBuildArgs {
    GraphDev g;
    int layer;
    int64_t n0, n1;               // batch of new internal ids
    const int32_t* levels;
    uint32_t* cur_entry;          // [cap_nodes] per-node descent entry (in/out)
    int ef;                       // efConstruction
    int mcap;                     // neighbors to select on this layer
    int heuristic;                // 0 closest-M, 1 HNSW heuristic on the new row, 2 also on overflowing rows
    int keep_pruned;              // fill the new row with pruned candidates up to mcap
    int expand;                   // entries expanded per step of the layer search (1-4; beam_layer XW)
    float alpha;                  // diversity slack: drop c when alpha * d(c, kept) < d(u, c) (1 = HNSW Alg. 4)
    int32_t* inc_cnt;             // [cap_nodes] incoming request counters (zero between batches)
    uint32_t* inc_src;            // [cap_nodes * inc_cap]
    float* inc_dist;              // [cap_nodes * inc_cap]
    int inc_cap;
    uint32_t* touched;            // [batch * mcap]
    int32_t* touched_cnt;         // [1]
    unsigned long long* stats;    // [0]=dist evals [1]=expansions [2]=dropped requests
    int vis_log2;
    const uint32_t* order;        // nullable: node of workgroup b is order[b] (b < count), nodes sorted by
    int64_t count;                //   level descending so that level >= layer is a prefix
    int64_t mw_max = 0;           // launches of at most this many inserts: one workgroup of 4 waves per insert
    int vis16 = 0;                // the layer searches' visited set is the compact 16-bit one (ids < 2^24)
    // The row-list form (nullable; the in-place update, update.hip): the batch is rows[n0 .. n1),
    // stored rows at their existing ids and levels, instead of the ids [n0, n1) themselves.
    // `order` holds row ids either way; cur_entry, inc_* and levels are indexed by row id.
    const uint32_t* rows = nullptr;
};
int launch_build_batch_search(const BatchBuildArgs& a, int lpr, int vpl, hipStream_t s);
// greedy descent of every node u in [n0, n1) through layers a.layer .. levels[u] + 1
int launch_build_batch_descend(const BatchBuildArgs& a, int lpr, int vpl, hipStream_t s);
int launch_build_batch_commit(const BatchBuildArgs& a, int lpr, int vpl, int64_t n_touched, hipStream_t s);
// The link pass (option "batch_link", build_link.hpp), after layer a.layer's commit: every
// batch row of the layer searches it again (a.ef: the link width) and stages its new row
// here; the reverse proposals go to a.inc_* / a.touched.  Rows are indexed by u - a.n0.
struct LinkArgs {
    int32_t* adj;             // [batch rows * stride] staged rows
    float* adjd;              // [batch rows * stride] their distances
    int32_t* deg;             // [batch rows] staged degree, -1: the row stays as it is
    int stride;               // >= the layer's row cap
    unsigned long long* cnt;  // [0] += rows staged, [1] += batch-mates new to their rows
};
int launch_build_batch_link(const BatchBuildArgs& a, const LinkArgs& k, int lpr, int vpl, hipStream_t s);
// the staged rows -> the adjacency (then launch_build_batch_commit merges the proposals)
int launch_build_batch_link_apply(const BatchBuildArgs& a, const LinkArgs& k, hipStream_t s);

// ---- exact / merge ----
// Brute-force path: approximate scores on MFMA (f32-input, or the bf16x3 split
// hi*hi + hi*lo + lo*hi), top-kk preselection, canonical re-rank of the kk,
// then a per-query certificate that no row outside the kk can belong to the
// canonical top-k; uncertified queries are redone by a full canonical sweep.
struct ExactArgs {
    const float* X;       // [N * pitch]
    const float* xnorm;   // [N]
    const uint8_t* dead;  // [N] 1 = deleted row (nullable)
    int64_t N;
    const float* Q;       // [B * pitch]
    const float* qnorm;   // [B] canonical |q|
    int64_t B;
    int pitch, dim, metric;
    float* scores;        // [B * ldS] workspace
    int64_t ldS;          // row stride of scores (multiple of 4, >= N)
    int kk;               // preselect width (<= 64)
    uint32_t* cand;       // [B * kk]
    float* bound;         // [B] k_select: kk-th preselected score (+inf when fewer)
    int nseg;             // k_select: row segments per query (<= 16), each seglen rows (multiple of 1024)
    int64_t seglen;
    float* seg_d;         // [B * nseg * kk] per-segment best scores / ids
    uint32_t* seg_i;
    const uint8_t* only;  // k_select: skip rows b with only[b] == 0 (nullable)
    const uint16_t* Xh;   // split mode: bf16 hi / lo planes of X, K-blocked (k_split_rows)
    const uint16_t* Xl;
    int64_t ldXs;         // rows per K-block of the X planes
    const uint16_t* Qh;   // split mode: bf16 hi / lo planes of Q, K-blocked
    const uint16_t* Ql;
    int64_t ldQs;
    const float* xinv;    // fp16 2-product mode: per-row / per-query unscale 2^-e (NaN: outside the bound)
    const float* qinv;
    // fp16 1-product ring (exact_precision 3)
    int tile_stride;          // sample pass: score every tile_stride-th row tile (1: every tile)
    int64_t nsample_tiles;    // ... how many (compact columns [0, nsample_tiles * BN) of scores)
    const float* ring_c;      // [>= roundup(B, 256)] filter constants (k_ring_prep; +inf pads)
    const float* ring_s;      // [same] L2: 1 / qi
    uint2* region;            // [tiles * rcap] passing pairs {row off | query off << 16, acc}
    int32_t* region_cnt;      // [tiles] pairs per tile (may exceed rcap: overflow)
    int rcap;                 // entries per tile region
    const float4* xw;         // [N] k_h1_pp: per-row filter constants (k_h1_rowconst)
};
int launch_exact_scores(const ExactArgs& a, hipStream_t s);     // f32-input MFMA
int launch_exact_scores_x3(const ExactArgs& a, int tile, hipStream_t s);  // bf16x3 split MFMA
// fp16 2-product split: (qh + ql) . xh on v_mfma_f32_32x32x16_f16 (Xl unused)
int launch_exact_scores_x2h(const ExactArgs& a, int tile, hipStream_t s);
// fp16 1-product ring: every score of the sampled row tiles, or the fused filter into regions
int launch_h1_sample(const ExactArgs& a, int variant, hipStream_t s);
int launch_h1_filter(const ExactArgs& a, int variant, hipStream_t s);
constexpr int H1_BN = 256;   // row tile of every launch_h1_* variant
constexpr int H1_BSUB = 16;     // sub-buckets per query (k_bucket)
constexpr int H1_CSTRIDE = 32;  // sub-bucket counters one 128-B line apart (no same-line atomics)
constexpr int H1_REC = 10;      // uint2 per record of the record-mode filter: {mb | lane << 8, 0}, pad, 16 accumulators
int h1_tile_bm(int variant);  // query tile of a variant (128 or 256)
bool h1_timing_diag(int variant);   // exact_tile 7-9, 11-13, 15-17, 19-20: timing diagnostics (no results)
int h1_region_split(int variant);   // regions per tile of the fused filter (rcap is split evenly)
bool h1_records(int variant);       // the variant's regions hold records (k_h1_pp16 REC), not pairs
int h1_effective_variant(int variant, int pitch, int64_t ld);  // the variant a search runs (0 -> default)
int launch_h1_rowconst(const float* xinv, const float* xnorm, const uint8_t* dead, int64_t n, int metric, float4* xw,
                       hipStream_t s);
int launch_ring_prep(const float* thr, const float* qnorm, const float* qinv, int64_t B, int metric, float* c,
                     float* sq, hipStream_t s);
// qcnt [B * H1_BSUB * H1_CSTRIDE], bucket [B * H1_BSUB * scap]
int launch_bucket(const uint2* region, const int32_t* region_cnt, int rcap, int64_t ntiles, int64_t nqt, int BM,
                  int BN, int64_t B, int32_t* qcnt, uint2* bucket, int scap, uint8_t* qovf, int rsub, int rec,
                  const ExactArgs& a, hipStream_t s);
int launch_select_bucket(const ExactArgs& a, const int32_t* qcnt, const uint2* bucket, int scap, const uint8_t* qovf,
                         const float* thr, hipStream_t s);
// err (nullable): running max of the rows' relative fp16 rounding |x' - x| / |x|
int launch_split_h16(const float* src, int64_t r0, int64_t r1, int pitch, int64_t rows, uint16_t* hi, uint16_t* lo,
                     float* inv, float* err, hipStream_t s);
int launch_exact_select(const ExactArgs& a, hipStream_t s);
int launch_split_rows(const float* src, int64_t r0, int64_t r1, int pitch, int64_t rows, uint16_t* hi, uint16_t* lo,
                      hipStream_t s);
// the planes of rows ids[0 .. m), each below `rows` (the in-place update)
int launch_split_rows_ids(const float* src, const uint32_t* ids, int64_t m, int pitch, int64_t rows, uint16_t* hi,
                          uint16_t* lo, hipStream_t s);
int launch_split_h16_ids(const float* src, const uint32_t* ids, int64_t m, int pitch, int64_t rows, uint16_t* hi,
                         uint16_t* lo, float* inv, float* err, hipStream_t s);
int launch_max_norm(const float* norms, int64_t n, float* out, hipStream_t s);

// ---- filtered exact search: the allowed rows as a dense row set (rowset.hip) ----
// The ascending ids of the rows whose filter bit is set (filter: fwords bitmap words) and whose
// `dead` byte (nullable) is clear -> ids[0 .. count), count <= cap; words [ceil(n / 32)], mask
// [32 ceil(n / 32)] (1 = not allowed) and block_cnt [rowset_blocks(n)] are its workspace.  The
// order is by ballot ranks and a prefix over blocks: the same list every time.
int64_t rowset_blocks(int64_t n);
int launch_rowset_compact(const uint32_t* filter, int64_t fwords, const uint8_t* dead, int64_t n, uint32_t* words,
                          uint8_t* mask, uint32_t* block_cnt, uint32_t* ids, int64_t cap, hipStream_t s);
// rows ids[0 .. m) of a K-blocked fp16 plane (ld_src rows per K-block) -> rows 0 .. m of dst
// (ld_dst rows per K-block), with their unscale and norm
int launch_rowset_gather(const uint16_t* src, int64_t ld_src, const uint32_t* ids, int64_t m, int pitch, uint16_t* dst,
                         int64_t ld_dst, const float* xinv, const float* xnorm, float* xinv_out, float* xnorm_out,
                         hipStream_t s);
// cand[i] (a position in the row set, or EMPTY_ID) -> ids[cand[i]]
int launch_rowset_remap(uint32_t* cand, int64_t total, const uint32_t* ids, int64_t m, hipStream_t s);

// ---- compaction: the deleted rows leave the store in place (compact.hip) ----
// newid[i] = live rows below i, -1 for a deleted row; src[newid[i]] = i (the live rows,
// ascending); block_cnt [compact_blocks(n)] is the workspace.  n > 0 rows, n entries each.
int64_t compact_blocks(int64_t n);
int launch_compact_map(const uint8_t* dead, int64_t n, uint32_t* block_cnt, int32_t* newid, uint32_t* src,
                       hipStream_t s);
// rows ids[0 .. rows) of base (row_bytes each, a multiple of 4) -> rows 0 .. rows of dst,
// which overlaps none of the rows read; member (nullable, a layer's deg indexed like base):
// rows with member < 0 are left out
int launch_compact_rows(const void* base, void* dst, const uint32_t* ids, int64_t rows, size_t row_bytes,
                        const int32_t* member, hipStream_t s);
// rows [0, rows) of a layer in place: every neighbour through newid, edges to deleted rows
// dropped (row order kept, degree shrinks) and counted in *dangling
int launch_compact_adj(int32_t* deg, int32_t* adj, float* adjd, int cap, int64_t rows, const int32_t* newid,
                       int64_t n_old, unsigned long long* dangling, hipStream_t s);
// out bit j = old bit src[j] for j < live, 0 above; nwords words each, out != old
int launch_compact_filter(const uint32_t* old, uint32_t* out, int64_t nwords, const uint32_t* src, int64_t live,
                          hipStream_t s);

// ---- update: stored rows re-embedded in place (update.hip) ----
// dead[ids[j]] = v for j < m: the chunk's rows are marked (UPDATE_MARK) while the delete repair
// detaches them, and unmarked (0) afterwards
constexpr uint8_t UPDATE_MARK = 2;  // a `dead` byte that is neither live (0) nor deleted (1)
int launch_update_mark(uint8_t* dead, const uint32_t* ids, int64_t m, uint8_t v, hipStream_t s);
// rows [0, rows) of a layer: a marked member loses its row (deg 0, adj -1, adjd 0); a deleted
// row drops its edges to marked rows (row order kept, as launch_compact_adj closes a row up)
int launch_update_detach(int32_t* deg, int32_t* adj, float* adjd, int cap, int64_t rows, const uint8_t* dead,
                         hipStream_t s);
// src row from[j] (padded) -> dst row ids[j] for j < m, in whole 16-byte words
int launch_update_scatter(const float* src, const uint32_t* ids, const uint32_t* from, int64_t m, int pitch, float* dst,
                          hipStream_t s);

// ---- analyzer: degree histogram, reachability, hop matrix (analyze.hip) ----
constexpr int AN_BINS = 256;      // degree bins on the device (a row cap past it is refused by the host)
constexpr int AN_MAX_KEYS = 128;  // sources of one hop BFS: one bit each of a row's 128-bit masks
// hist[d] += live members (deg != -2, dead byte clear; dead nullable) of degree d among rows [0, n)
int launch_an_degree(const int32_t* deg, const uint8_t* dead, int64_t n, unsigned long long* hist, hipStream_t s);
// The reachability bitmaps cover `rows` rows, a multiple of 64 at or past the row capacity; the
// queues hold `rows` entries.  seed: vis &= members of the layer (deg != -2), the rows left are
// queued (*qcnt += their number).  level: one BFS level from cur[0 .. ncur) -- rows visited
// first set their bit and join `next` (*ncnt += their number, any order); ids at or past capn
// set err bit 4 and are skipped.  count: cnt[0] += live members, cnt[1] += the visited ones,
// unr (nullable) = the live members not visited.
int launch_an_seed(const int32_t* deg, int64_t n, int64_t rows, uint32_t* vis, uint32_t* q, uint32_t* qcnt,
                   hipStream_t s);
int launch_an_level(const int32_t* deg, const int32_t* adj, int cap, uint32_t capn, const uint32_t* cur, uint32_t ncur,
                    uint32_t* vis, uint32_t* next, uint32_t* ncnt, int* err, hipStream_t s);
int launch_an_count(const int32_t* deg, const uint8_t* dead, int64_t n, int64_t rows, const uint32_t* vis, uint32_t* unr,
                    unsigned long long* cnt, hipStream_t s);
int launch_an_keys(const int64_t* keys, const uint32_t* ids, int64_t m, int64_t* out, hipStream_t s);  // out[i] = keys[ids[i]]
// Hop BFS from the ns <= AN_MAX_KEYS distinct rows src: seen / cur / next [4 * rows] words (zeroed),
// sidx [rows] (-1).  push + settle are one level; settle writes hops[i * ns + j] = level for
// source i reaching source row j now, and *any |= 1 while a frontier is left.
int launch_an_hops_init(const uint32_t* src, int ns, uint32_t* seen, uint32_t* cur, int32_t* sidx, hipStream_t s);
int launch_an_hops_push(const int32_t* deg, const int32_t* adj, int cap, uint32_t capn, int64_t n, const uint32_t* seen,
                        const uint32_t* cur, uint32_t* next, int* err, hipStream_t s);
int launch_an_hops_settle(int64_t rows, uint32_t* seen, uint32_t* cur, uint32_t* next, const int32_t* sidx, int ns,
                          int level, int32_t* hops, uint32_t* any, hipStream_t s);

// certificate of the re-rank (nullable pieces disable it)
struct CertArgs {
    const float* bound;          // [B] from k_select; nullptr = no certificate
    const float* qnorm;          // [B]
    const float* xmax;           // [1] largest row norm (L2)
    float eps_cos;               // cosine: |approx - canonical| distance bound
    float eps_dot, c_l2;         // L2: 2*eps_dot*|q|*xmax + c_l2*(|q|+xmax)^2 bounds |approx - canonical^2|
    uint8_t* flag;               // [B] out: 1 = not certified
    int32_t* flagged;            // [B] out: list of uncertified rows
    int32_t* nflag;              // [1] out: list length
    unsigned long long* stats;   // [0] += uncertified queries
    const uint8_t* only;         // re-rank only rows with only[b] != 0 (nullable)
    const float* xerr;           // fp16 2-product scores: max relative row rounding, added to the bound (nullable)
    const float* qerr;           // fp16 1-product scores: max relative query rounding of the batch (nullable)
};
int launch_rerank(const float* Q, const GraphDev& g, const uint32_t* cand, int kk, int64_t B, int lpr, int vpl, int k,
                  int64_t* out_keys, float* out_dist, int32_t* out_n, int32_t* out_ids, const CertArgs& c,
                  hipStream_t s);
// canonical distances of every row for the flagged queries (overwrites their score rows)
int launch_exact_fallback(const float* Q, const GraphDev& g, int64_t N, const int32_t* flagged, const int32_t* nflag,
                          float* scores, int64_t ldS, int lpr, int vpl, hipStream_t s);

// the fused path's fallback: canonical distances of every row streamed into per-segment
// top-kk lists (a.seg_d / a.seg_i, k_select's layout) for the queries a.only flags, then
// k_select_merge -> a.cand, a.bound (no score matrix)
int launch_fallback_select(const float* Q, const GraphDev& g, const ExactArgs& a, int lpr, int vpl, hipStream_t s);
int launch_merge_topk(const int64_t* keys_in, const float* dist_in, const int32_t* n_in, int shards, int64_t B,
                      int k, int64_t* out_keys, float* out_dist, int32_t* out_n, hipStream_t s);

// ---- range search (range.hip): every row within a per-query radius ----
// One chunk of queries (exact_run's chunking); lims / hits / stat belong to the whole call.
struct RangeArgs {
    GraphDev g;
    const float* Q;        // [B * pitch] the chunk's padded queries
    const float* radius;   // [B]
    int64_t B;
    int32_t* qcnt;         // the filter's sub-bucket counters (launch_bucket); slot 1 of each: the hits refine kept
    uint2* bucket;         // sub-buckets: candidates in, {row, distance bits} of the hits out (in place)
    int scap;
    const uint8_t* qovf;   // [B] a region of the query overflowed
    uint8_t* state;        // [B] 0: the filter covers the query, 1: sweep, 2: no hit possible (k_range_thr)
    uint8_t* sweep;        // [B] the sweep answers the query (state 1, or an overflow seen by refine)
    int32_t* cnt;          // [B] hits
    int32_t* cursor;       // [B] the sweep's write cursors
    int64_t* lims;         // [B + 1] the chunk's part of the call's prefix (lims[0]: the chunk's base)
    unsigned long long* hits;  // [hcap] {order image of the distance, row id}
    int64_t hcap, cap;     // hit buffer entries; the caller's capacity (queries starting at or past it write nothing)
    unsigned long long* stat;  // [0] pairs that reached refine, [1] queries the sweep answered
    // a filter's gathered row set (nullptr: every row of the index): the ascending ids of its m
    // rows; a bucket entry is then a position in the set's plane, and the sweep walks the list
    const uint32_t* ids;
    int64_t m;
};
int launch_range_thr(const RangeArgs& a, const float* qnorm, const float* qinv, const CertArgs& c, int fused, float* thr,
                     hipStream_t s);
int launch_range_refine(const RangeArgs& a, int lpr, int vpl, hipStream_t s);
int launch_range_gather(const RangeArgs& a, hipStream_t s);
// canonical sweep of rows [0, N) (of a row set: its N = a.m rows) for the queries a.sweep flags:
// write = false counts, true writes
int launch_range_sweep(const RangeArgs& a, int64_t N, int nseg, int64_t seglen, bool write, int lpr, int vpl,
                       hipStream_t s);
int launch_range_scan(const int32_t* cnt, int64_t B, int64_t* lims, int32_t* cursor, hipStream_t s);
int range_sort_temp_bytes(int64_t hcap, int64_t B, size_t* bytes);
int launch_range_order(const unsigned long long* hits, unsigned long long* sorted, int64_t hcap, const int64_t* lims,
                       int64_t B, int64_t cap, uint32_t* seg_b, uint32_t* seg_e, void* temp, size_t temp_bytes,
                       hipStream_t s);  // the sort alone (the wide exact search cuts the segments itself)
int launch_range_order_emit(const unsigned long long* hits, unsigned long long* sorted, int64_t hcap,
                            const int64_t* lims, int64_t B, int64_t cap, uint32_t* seg_b, uint32_t* seg_e, void* temp,
                            size_t temp_bytes, const GraphDev& g, int64_t* keys, float* dist, hipStream_t s);
// src_keys / src_dist [src_off[b] ..) -> keys / dist [lims[b], lims[b + 1]), one block per query
int launch_range_place(const int64_t* src_keys, const float* src_dist, const int64_t* src_off, const int64_t* lims,
                       int64_t B, int64_t* keys, float* dist, hipStream_t s);
// beam mode: the beam lists bk / bd / bn [B * ef] cut by the radius -> lims, keys, dist
int launch_range_beam(const int64_t* bk, const float* bd, const int32_t* bn, int ef, const float* radius, int64_t B,
                      int32_t* cnt, int64_t* lims, int64_t cap, int64_t* keys, float* dist, hipStream_t s);

// ---- wide exact search (wide.hip): exact top-k past k 256 through the range pipeline ----
// One chunk of queries: the J-th smallest of each query's ns sample scores (launch_h1_sample's
// compact matrix) as a distance radius, widened by the certificate's score error; NaN where no
// estimate can be made (force, ns < J, a zero query under cosine, a query outside the fp16
// bound -- qinv NaN --, a J-th score that is not finite).
struct WideRadiusArgs {
    const float* scores;  // [B * ldS]
    int64_t ldS, ns;
    int J;
    int metric;
    int force;            // test option wide_force_fallback: every radius NaN
    const float* qnorm;   // [B]
    const float* qinv;    // [B] (read only when ns >= J)
    CertArgs c;           // eps_cos / eps_dot / c_l2 / xmax / xerr / qerr
    int64_t B;
    float* radius;        // [B] out
};
int launch_wide_radius(const WideRadiusArgs& a, hipStream_t s);
// The cut, over the whole call: query b's sorted hits are sorted[lims[b] .. lims[b + 1]) when
// lims[b] < cap (else it wrote none).  >= k of them: the first k -> [b, :k], n[b] = k.  Fewer:
// b joins shortq (stat[0] counts the list; stat[1] += the hits that reached the sort).
struct WideEmitArgs {
    const unsigned long long* sorted;
    const int64_t* lims;  // [B + 1]
    int64_t B, cap;
    int k;                // <= 4096
    const int64_t* keys;  // row -> key
    uint32_t capn;
    int64_t* out_keys;    // [B * k]
    float* out_dist;      // [B * k]
    int32_t* out_n;       // [B]
    int32_t* out_ids;     // [B * k] (nullable)
    int32_t* shortq;      // [B]
    unsigned long long* stat;  // [2]
};
int launch_wide_emit(const WideEmitArgs& a, hipStream_t s);
// The short queries [g0, g0 + gn) of the list (none there: both kernels exit at once): the
// canonical distance of rows [0, N) of the index into wd [gn * ldW] (rows g.dead masks are
// skipped, as NaN distances are), then per query the min(k, qualifying) smallest by
// (distance, row id), sorted and written to [b, :k] with n[b]; Q: the call's padded queries.
int launch_wide_fallback(const float* Q, const GraphDev& g, int64_t N, const WideEmitArgs& a, int64_t g0, int64_t gn,
                         float* wd, int64_t ldW, int lpr, int vpl, hipStream_t s);

}  // namespace mh
