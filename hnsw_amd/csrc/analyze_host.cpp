// analyze_host.cpp -- the Analyzer's host side (analyzer.go; the kernels: analyze.hip): quality
// metrics, a layer's degree histogram, the hop matrix of a key set and the reachability of the
// rows from the searches' entry.  Read-only calls: they hold the handle's lock shared, wait for
// the last enqueued *_device search like a mutation does, and serialise among themselves on the
// analyzer's own lock (their scratch lives on the handle).
#include "index.hpp"

using namespace mhh;

namespace {

int an_refuse(mhnsw_index* h, bool needs_graph) {
    if (h->aliased)
        return fail(h, MHNSW_EUNSUPPORTED, "analyzer does not support a handle with a replaced or re-added key");
    if (needs_graph && h->build_mode == MHNSW_BUILD_FLAT)
        return fail(h, MHNSW_EUNSUPPORTED, "analyzer needs a compat or batch (build_mode 0 or 1) handle");
    return 0;
}

// rows the bitmaps and masks cover: the capacity, rounded up to whole waves
int64_t an_rows_of(const mhnsw_index* h) { return (std::max<int64_t>(h->capn, 1) + 63) / 64 * 64; }

// an_cnt: [0, AN_BINS) the histogram, then {members, reached} per layer, then 32-bit words: the
// two queue counters and the hop BFS's flag
constexpr size_t AN_CNT_LAYER = AN_BINS, AN_CNT_WORDS = AN_BINS + 2 * MH_MAXL, AN_CNT_TOTAL = AN_CNT_WORDS + 4;

int an_device_error(mhnsw_index* h) {
    int err = 0;
    HIPCHK(h, hipMemcpyAsync(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (err & 4) return fail(h, MHNSW_EINTERNAL, "out-of-range node id in adjacency (graph corrupt)");
    return 0;
}

// the exact degree histogram of layer l's live members
int an_hist(mhnsw_index* h, int l, unsigned long long* hist) {
    for (int i = 0; i < AN_BINS; ++i) hist[i] = 0;
    if (l < 0 || l >= (int)h->layers.size() || h->n == 0) return 0;
    const Layer& L = h->layers[l];
    if (L.cap > AN_BINS) return fail(h, MHNSW_EUNSUPPORTED, "analyzer supports at most %d neighbours per row", AN_BINS - 1);
    int r;
    if ((r = ensure_buf(h, h->an_cnt, AN_CNT_TOTAL))) return r;
    HIPCHK(h, hipMemsetAsync(h->an_cnt.p, 0, AN_BINS * sizeof(unsigned long long), h->stream));
    LCHK(h, launch_an_degree(L.deg, h->dead, h->n, h->an_cnt.p, h->stream));
    HIPCHK(h, hipMemcpyAsync(hist, h->an_cnt.p, AN_BINS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// hop matrix of the ns distinct live layer-0 rows src: out[i * ns + j], -1 beyond max_depth
int an_hops(mhnsw_index* h, const uint32_t* src, int ns, int max_depth, int32_t* out) {
    const int64_t rows = an_rows_of(h);
    const Layer& L = h->layers[0];
    hipStream_t s = h->stream;
    int r;
    if ((r = zero_err(h)) || (r = ensure_buf(h, h->an_hm, 12 * (size_t)rows)) ||
        (r = ensure_buf(h, h->an_sidx, (size_t)rows)) || (r = ensure_buf(h, h->an_hops, (size_t)AN_MAX_KEYS * AN_MAX_KEYS)) ||
        (r = ensure_buf(h, h->an_ids, (size_t)std::max<int64_t>(rows, AN_MAX_KEYS))) ||
        (r = ensure_buf(h, h->an_cnt, AN_CNT_TOTAL)))
        return r;
    uint32_t *seen = h->an_hm.p, *cur = seen + 4 * (size_t)rows, *next = cur + 4 * (size_t)rows;
    uint32_t* any = reinterpret_cast<uint32_t*>(h->an_cnt.p + AN_CNT_WORDS) + 2;
    for (int i = 0; i < ns; ++i)
        for (int j = 0; j < ns; ++j) out[(size_t)i * ns + j] = i == j ? 0 : -1;
    HIPCHK(h, hipMemsetAsync(h->an_hm.p, 0, 12 * (size_t)rows * 4, s));
    HIPCHK(h, hipMemsetAsync(h->an_sidx.p, 0xFF, (size_t)rows * 4, s));
    HIPCHK(h, hipMemcpyAsync(h->an_ids.p, src, (size_t)ns * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->an_hops.p, out, (size_t)ns * ns * 4, hipMemcpyHostToDevice, s));
    LCHK(h, launch_an_hops_init(h->an_ids.p, ns, seen, cur, h->an_sidx.p, s));
    for (int level = 1; level <= max_depth; ++level) {
        uint32_t left = 0;
        HIPCHK(h, hipMemsetAsync(any, 0, 4, s));
        LCHK(h, launch_an_hops_push(L.deg, L.adj, L.cap, (uint32_t)h->capn, h->n, seen, cur, next, h->d_err, s));
        LCHK(h, launch_an_hops_settle(rows, seen, cur, next, h->an_sidx.p, ns, level, h->an_hops.p, any, s));
        HIPCHK(h, hipMemcpyAsync(&left, any, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        if (!left) break;
    }
    HIPCHK(h, hipMemcpyAsync(out, h->an_hops.p, (size_t)ns * ns * 4, hipMemcpyDeviceToHost, s));
    return an_device_error(h);
}

// canonical distances among the rows src: out[i * S + j] = d(q = vec[src[i]], X = vec[src[j]])
int an_sample_dist(mhnsw_index* h, const uint32_t* src, int S, float* out) {
    hipStream_t s = h->stream;
    int r;
    if ((r = ensure_buf(h, h->an_rows, (size_t)S * h->pitch)) || (r = ensure_buf(h, h->an_dist, (size_t)S * S)) ||
        (r = ensure_buf(h, h->an_ids, (size_t)std::max<int64_t>(an_rows_of(h), AN_MAX_KEYS))))
        return r;
    HIPCHK(h, hipMemcpyAsync(h->an_ids.p, src, (size_t)S * 4, hipMemcpyHostToDevice, s));
    LCHK(h, launch_compact_rows(h->vecs, h->an_rows.p, h->an_ids.p, S, (size_t)h->pitch * 4, nullptr, s));
    for (int i = 0; i < S; ++i)
        LCHK(h, launch_sweep(h->an_rows.p + (size_t)i * h->pitch, h->an_rows.p, S, h->pitch, h->lpr, h->vpl, h->metric,
                             h->an_dist.p + (size_t)i * S, s));
    HIPCHK(h, hipMemcpyAsync(out, h->an_dist.p, (size_t)S * S * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}

bool an_live0(const mhnsw_index* h, int64_t row) { return !h->hdead[row] && in_layer(h, row, 0); }

// analyzer.go:245-279 calculateLayerBalance
double an_layer_balance(const mhnsw_index* h) {
    const int L = (int)h->layers.size();
    if (L <= 1) return 0.0;
    const double ml = h->ml;
    if (ml <= 0 || ml >= 1) return 0;
    const double base = (double)h->layers[0].count;
    if (base == 0) return 0;
    double sum = 0;
    for (int i = 1; i < L; ++i) {
        // (Go's math.Pow and std::pow may differ in the last bit: unpinned)
        const double expected = base * std::pow(ml, (double)i);
        const double actual = (double)h->layers[i].count;
        if (expected == 0) continue;
        double ratio = actual / expected;
        if (ratio > 1) ratio = 1 / ratio;
        sum += ratio;
    }
    return sum / (double)(L - 1);
}

// analyzer.go:135-189 calculateDistortionRatio over the engine's sample: the first
// min(100, NodeCount) live layer-0 rows in ascending row id
int an_distortion(mhnsw_index* h, int64_t node_count, double* out) {
    *out = 0;
    if (node_count < 10) return 0;
    std::vector<uint32_t> sample;
    for (int64_t i = 0; i < h->n && sample.size() < 100; ++i)
        if (an_live0(h, i)) sample.push_back((uint32_t)i);
    const int S = (int)sample.size();
    if (S < 5) return 0;
    std::vector<int32_t> hops((size_t)S * S);
    std::vector<float> dist((size_t)S * S);
    int r;
    if ((r = an_hops(h, sample.data(), S, 10, hops.data())) || (r = an_sample_dist(h, sample.data(), S, dist.data())))
        return r;
    double sum = 0;
    int64_t pairs = 0;
    for (int i = 0; i < S; ++i)
        for (int j = i + 1; j < S; ++j) {
            const int32_t g = hops[(size_t)i * S + j];
            const float a = dist[(size_t)i * S + j];
            if (g > 0 && !std::isnan(a) && !std::isinf(a)) {
                sum += (double)g / (double)a;
                ++pairs;
            }
        }
    if (pairs) *out = sum / (double)pairs;
    return 0;
}

// The BFS of one layer from the rows queued in q0 (their bits already set in vis); -> levels run
int an_bfs(mhnsw_index* h, const Layer& L, uint32_t* vis, uint32_t* q0, uint32_t* q1, uint32_t n0, uint32_t* qcnt,
           int32_t* depth) {
    hipStream_t s = h->stream;
    uint32_t ncur = n0;
    int slot = 0;
    *depth = 0;
    while (ncur > 0) {
        uint32_t* cnt = qcnt + (slot ^ 1);
        HIPCHK(h, hipMemsetAsync(cnt, 0, 4, s));
        LCHK(h, launch_an_level(L.deg, L.adj, L.cap, (uint32_t)h->capn, slot ? q1 : q0, ncur, vis, slot ? q0 : q1, cnt,
                                h->d_err, s));
        HIPCHK(h, hipMemcpyAsync(&ncur, cnt, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        ++*depth;
        slot ^= 1;
    }
    return 0;
}

int an_reach(mhnsw_index* h, int64_t* members, int64_t* reached, int32_t* depth) {
    const int nl = (int)h->layers.size();
    for (int l = 0; l < MH_MAXL; ++l) members[l] = reached[l] = 0, depth[l] = 0;
    h->an_unreach.clear();
    const int T = top_live_layer(h);
    if (T < 0 || h->layers[T].count == 0 || h->n == 0) return 0;
    const int64_t rows = an_rows_of(h), W = rows / 32;
    hipStream_t s = h->stream;
    int r;
    if ((r = zero_err(h)) || (r = ensure_buf(h, h->an_bits, 3 * (size_t)W)) || (r = ensure_buf(h, h->an_q, 2 * (size_t)rows)) ||
        (r = ensure_buf(h, h->an_cnt, AN_CNT_TOTAL)) || (r = ensure_buf(h, h->an_ids, (size_t)rows)) ||
        (r = ensure_buf(h, h->an_mask, (size_t)rows)) || (r = ensure_buf(h, h->an_blk, (size_t)rowset_blocks(rows) + 1)))
        return r;
    uint32_t *vis = h->an_bits.p, *unr = vis + W, *words = unr + W, *q0 = h->an_q.p, *q1 = q0 + rows;
    unsigned long long* lcnt = h->an_cnt.p + AN_CNT_LAYER;
    uint32_t* qcnt = reinterpret_cast<uint32_t*>(h->an_cnt.p + AN_CNT_WORDS);
    HIPCHK(h, hipMemsetAsync(lcnt, 0, 2 * MH_MAXL * sizeof(unsigned long long), s));
    HIPCHK(h, hipMemsetAsync(vis, 0, (size_t)W * 4, s));
    for (int l = T; l >= 0; --l) {
        const Layer& L = h->layers[l];
        uint32_t n0 = 0;
        if (l == T) {
            // the searches' entry of the top live layer
            const int64_t e = L.entry;
            if (e >= 0 && e < h->n) {
                const uint32_t bit = 1u << (e & 31), row = (uint32_t)e;
                HIPCHK(h, hipMemcpyAsync(vis + (e >> 5), &bit, 4, hipMemcpyHostToDevice, s));
                HIPCHK(h, hipMemcpyAsync(q0, &row, 4, hipMemcpyHostToDevice, s));
                HIPCHK(h, hipStreamSynchronize(s));
                n0 = 1;
            }
        } else {
            HIPCHK(h, hipMemsetAsync(qcnt, 0, 4, s));
            LCHK(h, launch_an_seed(L.deg, h->n, rows, vis, q0, qcnt, s));
            HIPCHK(h, hipMemcpyAsync(&n0, qcnt, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipStreamSynchronize(s));
        }
        if ((r = an_bfs(h, L, vis, q0, q1, n0, qcnt, &depth[l]))) return r;
        LCHK(h, launch_an_count(L.deg, h->dead, h->n, rows, vis, l == 0 ? unr : nullptr, lcnt + 2 * l, s));
    }
    unsigned long long c[2 * MH_MAXL];
    HIPCHK(h, hipMemcpyAsync(c, lcnt, sizeof(c), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int l = 0; l < nl; ++l) members[l] = (int64_t)c[2 * l], reached[l] = (int64_t)c[2 * l + 1];
    // the unreachable live layer-0 rows, ascending, and their keys
    const int64_t m = members[0] - reached[0];
    if (m > 0) {
        if ((r = ensure_buf(h, h->an_keys, (size_t)m))) return r;
        LCHK(h, launch_rowset_compact(unr, W, nullptr, rows, words, h->an_mask.p, h->an_blk.p, h->an_ids.p, m, s));
        LCHK(h, launch_an_keys(h->keys, h->an_ids.p, m, h->an_keys.p, s));
        h->an_unreach.resize((size_t)m);
        HIPCHK(h, hipMemcpyAsync(h->an_unreach.data(), h->an_keys.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    }
    return an_device_error(h);
}

}  // namespace

extern "C" {

int mhnsw_degree_histogram(mhnsw_index* h, int layer, int64_t* out) {
    if (!h || !out) return fail(h, MHNSW_EINVAL, "out must be non-NULL");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    std::lock_guard<std::mutex> alk(h->an_mu);
    int r;
    if ((r = drain(h)) || (r = an_refuse(h, false))) return r;
    if (layer < 0 || layer >= std::max<int>((int)h->layers.size(), 1)) return fail(h, MHNSW_EINVAL, "no layer %d", layer);
    unsigned long long hist[AN_BINS];
    if ((r = an_hist(h, layer, hist))) return r;
    for (int d = 64; d < AN_BINS; ++d)
        if (hist[d]) return fail(h, MHNSW_EUNSUPPORTED, "degree histogram holds degrees up to 63, the layer has %d", d);
    for (int d = 0; d < 64; ++d) out[d] = (int64_t)hist[d];
    return MHNSW_OK;
}

int mhnsw_hops(mhnsw_index* h, const int64_t* keys, int n, int max_depth, int32_t* out) {
    // (the argument checks come before the handle is touched)
    if (!keys || !out) return fail(h, MHNSW_EINVAL, "keys and out must be non-NULL");
    if (n > AN_MAX_KEYS) return fail(h, MHNSW_EUNSUPPORTED, "hops supports at most 128 keys");
    if (n < 1) return fail(h, MHNSW_EINVAL, "hops needs at least 1 key");
    if (max_depth < 1 || max_depth > 64) return fail(h, MHNSW_EINVAL, "max_depth must be in [1, 64], got %d", max_depth);
    if (!h) return fail(h, MHNSW_EINVAL, "handle must be non-NULL");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    std::lock_guard<std::mutex> alk(h->an_mu);
    int r;
    if ((r = drain(h)) || (r = an_refuse(h, true))) return r;
    std::vector<uint32_t> src((size_t)n);
    std::unordered_map<int64_t, int> seen;
    for (int i = 0; i < n; ++i) {
        if (!seen.emplace(keys[i], i).second) return fail(h, MHNSW_EINVAL, "duplicate key %lld in hops", (long long)keys[i]);
        auto it = h->key2id.find(keys[i]);
        if (it == h->key2id.end() || !an_live0(h, it->second))
            return fail(h, MHNSW_EINVAL, "key %lld has no live layer-0 row", (long long)keys[i]);
        src[i] = (uint32_t)it->second;
    }
    return an_hops(h, src.data(), n, max_depth, out);
}

int mhnsw_reachability(mhnsw_index* h, int64_t* members, int64_t* reached, int32_t* depth, int max_layers,
                       int64_t* out_unreachable) {
    if (!h) return fail(h, MHNSW_EINVAL, "handle must be non-NULL");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    std::lock_guard<std::mutex> alk(h->an_mu);
    int r;
    if ((r = drain(h)) || (r = an_refuse(h, true))) return r;
    if (!h->aev0) {
        HIPCHK(h, hipEventCreate(&h->aev0));
        HIPCHK(h, hipEventCreate(&h->aev1));
    }
    int64_t mem[MH_MAXL], rea[MH_MAXL];
    int32_t dep[MH_MAXL];
    h->have_reach_timing = false;
    HIPCHK(h, hipEventRecord(h->aev0, h->stream));
    if ((r = an_reach(h, mem, rea, dep))) return r;
    HIPCHK(h, hipEventRecord(h->aev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->aev1));
    h->have_reach_timing = true;
    const int nl = (int)h->layers.size();
    for (int l = 0; l < nl && l < max_layers; ++l) {
        if (members) members[l] = mem[l];
        if (reached) reached[l] = rea[l];
        if (depth) depth[l] = dep[l];
    }
    if (out_unreachable) *out_unreachable = (int64_t)h->an_unreach.size();
    return nl;
}

int mhnsw_unreachable_keys(mhnsw_index* h, int64_t* out_keys, int64_t cap) {
    if (!h) return fail(h, MHNSW_EINVAL, "handle must be non-NULL");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    std::lock_guard<std::mutex> alk(h->an_mu);
    const int64_t m = std::min<int64_t>(cap, (int64_t)h->an_unreach.size());
    if (m > 0 && !out_keys) return fail(h, MHNSW_EINVAL, "out_keys must be non-NULL");
    for (int64_t i = 0; i < m; ++i) out_keys[i] = h->an_unreach[i];
    return MHNSW_OK;
}

int mhnsw_quality_metrics(mhnsw_index* h, mhnsw_quality* out) {
    if (!h || !out) return fail(h, MHNSW_EINVAL, "out must be non-NULL");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    std::lock_guard<std::mutex> alk(h->an_mu);
    int r;
    if ((r = drain(h)) || (r = an_refuse(h, true))) return r;
    memset(out, 0, sizeof(*out));
    if (h->layers.empty()) return MHNSW_OK;  // analyzer.go:52-54
    unsigned long long hist[AN_BINS];
    if ((r = an_hist(h, 0, hist))) return r;
    int64_t nodes = 0, edges = 0;
    for (int d = 0; d < AN_BINS; ++d) nodes += (int64_t)hist[d], edges += (int64_t)hist[d] * d;
    out->node_count = nodes;
    out->graph_height = (int64_t)h->layers.size();
    if (nodes > 0) {
        // analyzer.go:93-130, the squared differences summed by degree in ascending order
        const double avg = (double)edges / (double)nodes;
        double ss = 0;
        for (int d = 0; d < AN_BINS; ++d)
            if (hist[d]) ss += (double)hist[d] * (((double)d - avg) * ((double)d - avg));
        out->avg_connectivity = avg;
        out->connectivity_std_dev = std::sqrt(ss / (double)nodes);
    }
    if ((r = an_distortion(h, nodes, &out->distortion_ratio))) return r;
    out->layer_balance = an_layer_balance(h);
    return MHNSW_OK;
}

}  // extern "C"
