// search_host.cpp -- host orchestration of the searches (graph.go:534-625, 1047-1110,
// 1116-1537).  An entry point describes its call as a SearchCall and runs in on_scratch
// (stream ordering of the *_device calls).  search_plain and search_filtered check the
// arguments in their own order, with the reference's error texts, and share stage (queries,
// outputs, error word), walk_args (the walk kernels' SearchArgs, the visited-set rule), finish
// and read_error / device_error.  The plain search is exact_prepare + exact_run (score GEMM,
// fused preselection, bucket select, canonical re-rank, certificate, fallback), beam_search
// or compat_search.  exact_prepare / exact_run work on a RowSet: every row of the index, or
// (search_filtered_exact) a filter's allowed rows gathered into a dense plane (rowset.hip).
// The range search (range_search, range_exact) runs over the same two kinds of row set, and in
// beam mode cuts the beam search's or the filtered walk's (filtered_walk) lists.
// Last, the negative-example re-ranking.
#include "index.hpp"

using namespace mhh;

namespace mhh {

// Mutations (Add / Delete / Reserve / Import) first let every enqueued
// search finish: they rewrite or reallocate what those kernels read.
// The beam search kernel is held to 2 waves per SIMD by its VGPRs (8 per CU),
// which leaves 20 KiB of the CU's 160 KiB LDS per wave: its visited set takes
// 1.25 * 2^vis_log2 entries (5,120 at the default), fewer resets at large ef.
int beam_vis_entries(const mhnsw_index* h) {
    if (h->vis_entries > 0) return h->vis_entries;
    return std::min(32768, 5 << (h->vis_log2 - 2));
}

int drain(mhnsw_index* h) {
    if (h->scr_valid) HIPCHK(h, hipEventSynchronize(h->scr_ev));
    h->scr_valid = false;
    return 0;
}

// A search's device error word as the call's error.  (Only the filtered kernel sets bit 8:
// the plain and negatives paths, which never tested it, report what they always did.)
int device_error(mhnsw_index* h, int err) {
    if (!err) return 0;
    if (err & 4) return fail(h, MHNSW_EINTERNAL, "out-of-range node id in adjacency (graph corrupt)");
    if (err & 8) return fail(h, MHNSW_EINVAL, "unknown filter in filter_of");
    return fail(h, MHNSW_EINTERNAL, "visited set overflow (raise vis_log2)");
}

// One search as its entry point describes it; dk .. errw are what stage() adds: the
// outputs on the device (the caller's, or scratch) and the kernels' error word.
struct SearchCall {
    const float* queries;  // [B * dim], on the host or (on_device) on the device, as the outputs
    bool on_device;
    int64_t B;
    int dim, k;
    int64_t* okeys;
    float* odist;
    int32_t* on;
    int32_t* out_ids;  // [B * k] internal ids (device, nullable)
    hipStream_t s;
    bool sticky;  // report into d_err[1] (a *_device call, mhnsw_device_status), else into d_err[0], zeroed first
    bool timing;  // ev0 / ev1 around the search kernels
    int64_t* dk;
    float* dd;
    int32_t* dn;
    int* errw;
};

// every search: after the scratch's previous user (another stream); the event is recorded on failure too
template <class Body>
static int on_scratch(mhnsw_index* h, hipStream_t s, Body body) {
    if (h->scr_valid && h->scr_stream != s) HIPCHK(h, hipStreamWaitEvent(s, h->scr_ev, 0));
    const int r = body();
    HIPCHK(h, hipEventRecord(h->scr_ev, s));
    h->scr_stream = s;
    h->scr_valid = true;
    return r;
}

// k, the dimension, the mode (a filtered search is a beam search) and the flat index, in this order
static int check_args(mhnsw_index* h, const SearchCall& c, int mode) {
    if (c.k <= 0) return fail(h, MHNSW_EK, "k must be greater than 0, got %d", c.k);  // graph.go:542-544
    if (h->layers_exist && h->dim != c.dim) {                                          // graph.go:547-552
        if (c.B == 1) return fail(h, MHNSW_EDIM, "embedding dimension mismatch: %d != %d", h->dim, c.dim);
        return fail(h, MHNSW_EDIM, "embedding dimension mismatch for query %d: %d != %d", 0, h->dim, c.dim);
    }
    if (mode < 0 || mode > 2) return fail(h, MHNSW_EINVAL, "unknown search mode %d", mode);
    if (h->build_mode == MHNSW_BUILD_FLAT && mode != MHNSW_MODE_EXACT)
        return fail(h, MHNSW_EUNSUPPORTED, "flat index (build_mode 2) supports exact search only");
    return 0;
}

// graph.go:554-556: an empty index (no layers, or no live row) answers nil, nil
static int zero_counts(mhnsw_index* h, const SearchCall& c) {
    if (c.on_device)
        HIPCHK(h, hipMemsetAsync(c.on, 0, c.B * 4, c.s));
    else
        memset(c.on, 0, c.B * 4);
    return 0;
}

// the queries padded into qpad, the device output buffers, the error word
static int stage(mhnsw_index* h, SearchCall& c) {
    int r;
    if ((r = ensure_buf(h, h->qpad, (size_t)c.B * h->pitch))) return r;
    if (!c.on_device) {
        if ((r = ensure_buf(h, h->tmp, (size_t)c.B * c.dim))) return r;
        HIPCHK(h, hipMemcpyAsync(h->tmp.p, c.queries, (size_t)c.B * c.dim * 4, hipMemcpyHostToDevice, c.s));
    }
    LCHK(h, launch_pad_rows(c.on_device ? c.queries : h->tmp.p, c.B, c.dim, h->qpad.p, h->pitch, c.s));
    if (!c.on_device && ((r = ensure_buf(h, h->okeys, (size_t)c.B * c.k)) ||
                         (r = ensure_buf(h, h->odist, (size_t)c.B * c.k)) || (r = ensure_buf(h, h->on, (size_t)c.B))))
        return r;
    c.dk = c.on_device ? c.okeys : h->okeys.p;
    c.dd = c.on_device ? c.odist : h->odist.p;
    c.dn = c.on_device ? c.on : h->on.p;
    c.errw = c.sticky ? h->d_err + 1 : h->d_err;
    if (!c.sticky) HIPCHK(h, hipMemsetAsync(h->d_err, 0, sizeof(int), c.s));
    return 0;
}

// d_err[0] once the stream's work is done, as the call's error
static int read_error(mhnsw_index* h, hipStream_t s) {
    int err = 0;
    HIPCHK(h, hipMemcpyAsync(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return device_error(h, err);
}

// a search whose kernels are enqueued: a host-pointer call waits for its results
static int finish(mhnsw_index* h, const SearchCall& c) {
    h->have_timing = c.timing;
    h->stats_host[6] += c.B;
    if (c.on_device) return 0;
    HIPCHK(h, hipMemcpyAsync(c.okeys, c.dk, (size_t)c.B * c.k * 8, hipMemcpyDeviceToHost, c.s));
    HIPCHK(h, hipMemcpyAsync(c.odist, c.dd, (size_t)c.B * c.k * 4, hipMemcpyDeviceToHost, c.s));
    HIPCHK(h, hipMemcpyAsync(c.on, c.dn, (size_t)c.B * 4, hipMemcpyDeviceToHost, c.s));
    return read_error(h, c.s);
}

// the search kernels run on the caller's stream; metadata goes up on the handle's
static int order_meta(mhnsw_index* h, hipStream_t s) {
    if (s == h->stream) return 0;
    HIPCHK(h, hipEventRecord(h->meta_ev, h->stream));
    HIPCHK(h, hipStreamWaitEvent(s, h->meta_ev, 0));
    return 0;
}

// The walk kernels' arguments (beam, compat, filtered), the graph's metadata brought up to date.
// ef: the walk's layer-0 list (the filtered search's route list); lds_tier: the launch keeps it in LDS.
static int walk_args(mhnsw_index* h, const SearchCall& c, int top, uint32_t entry, int ef, bool lds_tier, SearchArgs& a) {
    int r;
    if ((r = sync_layer_entries(h)) || (r = sync_layer_table(h)) || (r = order_meta(h, c.s))) return r;
    const int width = std::max(ef, c.k);
    a.g = graph_view(h);
    a.g.err = c.errw;
    a.q = h->qpad.p;
    a.B = c.B;
    a.k = c.k;
    a.ef = ef;
    a.top = top;
    a.entry = entry;
    a.layer_entry = h->d_layer_entry;
    a.out_keys = c.dk;
    a.out_dist = c.dd;
    a.out_n = c.dn;
    a.out_ids = c.out_ids;
    a.stats = h->d_stats;
    a.err = c.errw;
    a.vis_log2 = h->vis_log2;
    a.vis_n = beam_vis_entries(h);
    // the compact set holds 8,192 ids in 16 KiB (the 32-bit set 5,120 in 20 KiB):
    // fewer resets at large ef, the same results either way.  Below ef 129 the
    // 32-bit set rarely fills and its single-CAS probe is the cheaper one
    // (the compact probe cost 1 % at the headline ef 64).
    // (only where the compact set holds more ids than the 32-bit one in the LDS
    // it is given: a user who raised vis_entries past 8,192 keeps that set)
    a.vis16 = h->vis_compact && width > 128 && h->capn <= (int64_t(1) << 24) &&
              (int64_t)a.vis_n >= (int64_t)VIS16_WORDS && a.vis_n < VIS16_HOMES;
    // the LDS-list tier re-seeds up to `width` ids after a visited reset: an
    // automatically sized 32-bit set holds at least 4 width entries there (at
    // 5,120, resetting at 3/4 full, ef 2048 would reset every few steps).  An
    // explicit vis_entries is kept as given: the results do not depend on it.  (2048: the tier's limit)
    if (lds_tier && !a.vis16 && h->vis_entries <= 0) a.vis_n = std::max(a.vis_n, 4 * std::min(width, 2048));
    a.upper_ef = h->upper_ef;
    a.mw_max_b = h->beam_mw_max_b;
    a.expand = h->search_expand;
    return 0;
}

// The ordered beam search's sort key: the node the descent stood on when it left
// layer key_top in the most significant field, then the nodes of the
// ORDER_KEY_FIELDS - 1 layers below it (option search_order_fields), each in
// 64 / fields bits: the node id where it fits, else a hash of it.  The sort is
// then a walk of the descent tree: the queries of one cell of the lowest field
// are contiguous, and so are the cells under one parent.  key_top (option
// search_order_top, 0 = automatic): the lowest layer with at most
// B / ORDER_CELL_QUERIES nodes (measured, DESIGN.md "Query order").  A graph
// whose only layer is 0 has no field: every key is 0.
constexpr int ORDER_KEY_FIELDS = 3;
constexpr int64_t ORDER_CELL_QUERIES = 128;
static void order_key_layers(const mhnsw_index* h, int64_t B, int top, SearchArgs& a) {
    int bits = 1;
    while (bits < 31 && (int64_t(1) << bits) < h->capn) ++bits;
    int kt = h->search_order_top;
    if (kt <= 0) {
        kt = 1;
        while (kt < top && h->layers[kt].count > std::max<int64_t>(1, B / ORDER_CELL_QUERIES)) ++kt;
    }
    a.key_top = std::min(kt, top);
    a.key_n = std::min(h->search_order_fields > 0 ? h->search_order_fields : ORDER_KEY_FIELDS, a.key_top);
    a.key_id_bits = a.key_n > 0 ? std::min(bits, 64 / a.key_n) : 1;
    a.key_hash = a.key_id_bits < bits;
}

static int beam_search(mhnsw_index* h, const SearchCall& c, SearchArgs& a) {
    int r;
    const int64_t B = c.B;
    hipStream_t s = c.s;
    if (std::max(a.ef, a.k) > 2048) return fail(h, MHNSW_EUNSUPPORTED, "beam mode supports max(ef,k) <= 2048");
    a.lds_min_ef = h->beam_lds_min_ef;
    // ordered path: the descent as a pre-pass, the queries sorted by descent
    // path, layer 0 searched in that order (the one-wave kernels only)
    const bool ordered = h->search_order && B >= h->search_order_min_b && !beam_small_batch(a);
    size_t tmp_bytes = 0;
    if (ordered) {
        LCHK(h, order_sort_temp_bytes(B, &tmp_bytes));
        const size_t pstat_at = ((size_t)3 * B + 3) & ~(size_t)3;  // (16-byte aligned: one store per query)
        if ((r = ensure_buf(h, h->ordkey, (size_t)2 * B)) || (r = ensure_buf(h, h->ordval, pstat_at + (size_t)4 * B)) ||
            (r = ensure_buf(h, h->ordtmp, std::max<size_t>(tmp_bytes, 1))))
            return r;
        a.okey = h->ordkey.p;
        a.oidx = h->ordval.p;
        a.ep0 = h->ordval.p + 2 * B;
        a.pstat = h->ordval.p + pstat_at;
        order_key_layers(h, B, a.top, a);
        a.order_chunk = h->search_order_map == 0 ? (B + 7) / 8 : 0;
    }
    if (c.timing) HIPCHK(h, hipEventRecord(h->ev0, s));
    int lr = 0;
    if (ordered && !(lr = launch_beam_descend(a, h->lpr, h->vpl, s))) {
        LCHK(h, launch_order_sort(h->ordkey.p, h->ordkey.p + B, h->ordval.p, h->ordval.p + B, B,
                                  a.key_n * a.key_id_bits, h->ordtmp.p, tmp_bytes, s));
        a.order = h->ordval.p + B;
    }
    if (!lr) lr = launch_search_beam(a, h->lpr, h->vpl, s);
    if (lr == -2)
        return fail(h, MHNSW_EUNSUPPORTED, "beam search LDS budget exceeded (ef=%d, k=%d, vis_entries=%d)", a.ef, a.k,
                    a.vis_n);
    LCHK(h, lr);
    if (c.timing) HIPCHK(h, hipEventRecord(h->ev1, s));
    return 0;
}

static int compat_search(mhnsw_index* h, const SearchCall& c, const SearchArgs& a) {
    if (c.timing) HIPCHK(h, hipEventRecord(h->ev0, c.s));
    int lr = launch_search_compat(a, h->lpr, h->vpl, c.s);
    if (lr == -2) return fail(h, MHNSW_EUNSUPPORTED, "compat search LDS budget exceeded (ef=%d, k=%d)", a.ef, a.k);
    LCHK(h, lr);
    if (c.timing) HIPCHK(h, hipEventRecord(h->ev1, c.s));
    return 0;
}

// The rows the exact pipeline scores.  The plain search's is the identity: every row of the
// index, the planes and per-row constants the handle caches, deleted rows masked.  A filtered
// exact search's is the filter's allowed rows gathered into a dense plane (rowset.hip): n and
// ld are the host's count of them, exact_run fills the plane, and ids maps a position to its row.
struct RowSet {
    int64_t n, ld;        // rows, and rows per K-block of the plane
    int precision;        // exact_precision the scores run at
    const uint32_t* ids;  // position -> row id (nullptr: the identity)
    const uint32_t* filter;  // the allowed rows' bitmap of fwords words (a gathered set)
    int64_t fwords;
};

// what exact_prepare decides for exact_run (the names are the two functions' locals)
struct ExactPlan {
    bool split, h1, h2;
    int kk, nseg, ev, bm, stride, J, sseg, rcap, rsub, scap;
    int64_t ldS, qc, seglen, nnt, nsamp, sseglen;
    const uint8_t* xdead;
    GraphDev g;
    CertArgs cert;
    RowSet rs;
    int fnseg;  // a gathered set's fallback sweeps every row of the index: its segments
    int64_t fseglen;
};

// rows the brute force skips: deleted ones, and the live rows of a failed
// insert that never reached layer 0 (graph.go:1009 leaves them in upper
// layers only; Search cannot return them)
static int exact_skipped(mhnsw_index* h, hipStream_t s, const uint8_t*& xdead) {
    int r;
    xdead = h->any_dead ? h->dead : nullptr;
    if (h->partial_rows && h->xgone_epoch != h->mut_epoch) {  // rebuilt only after a mutation
        // a Delete or a replacement sweep may have killed the last partial rows
        std::vector<uint8_t> gone((size_t)h->n);
        int64_t partial = 0;
        for (int64_t i = 0; i < h->n; ++i) {
            const bool p = !h->hdead[i] && !in_layer(h, i, 0);
            partial += p;
            gone[i] = h->hdead[i] || p;
        }
        h->partial_rows = partial;
        if (partial) {
            if ((r = ensure_buf(h, h->xgone, (size_t)std::max<int64_t>(h->n, 1)))) return r;
            HIPCHK(h, hipMemcpyAsync(h->xgone.p, gone.data(), (size_t)h->n, hipMemcpyHostToDevice, s));
            HIPCHK(h, hipStreamSynchronize(s));
        }
        h->xgone_epoch = h->mut_epoch;
    }
    if (h->partial_rows) xdead = h->xgone.p;
    return 0;
}

// the sample pass's shape over N rows: every stride-th full row tile, nsamp of them (h1: the fused path runs)
static void sample_shape(const mhnsw_index* h, int64_t N, bool h1, int& stride, int64_t& nsamp) {
    const int64_t nnt = (N + H1_BN - 1) / H1_BN;
    stride = (int)std::max<int64_t>(1, std::min<int64_t>(128, (nnt + h->exact_sample - 1) / h->exact_sample));
    nsamp = h1 ? ((N / H1_BN) - 1) / stride + 1 : 0;
}

// Exact mode's limit on k, and whether the search takes the wide path (option "exact_wide":
// every k past 256, and the k from "exact_wide_min_k" up)
static int exact_k_limit(mhnsw_index* h, int k, bool& wide) {
    wide = h->exact_wide && (k > 256 || k >= h->exact_wide_min_k);
    if (h->exact_wide && k > 4096) return fail(h, MHNSW_EUNSUPPORTED, "exact mode supports k <= 4096");
    if (!h->exact_wide && k > 256) return fail(h, MHNSW_EUNSUPPORTED, "exact mode supports k <= 256");
    return 0;
}
int exact_k_check(mhnsw_index* h, int k) {
    bool wide;
    return exact_k_limit(h, k, wide);
}

// the exact path's workspace, the rows it skips and the certificate constants
// (expect > 0, a range search: the regions and sub-buckets are sized for that many passing
// rows per query over the whole index instead of J over the sample)
static int exact_prepare(mhnsw_index* h, const SearchCall& c, const RowSet& rs, ExactPlan& plan, int64_t expect = 0) {
    int r;
    const int k = c.k;
    hipStream_t s = c.s;
    if (k > 256) return fail(h, MHNSW_EUNSUPPORTED, "exact mode supports k <= 256");
    const int64_t N = rs.n;  // rows scored
    const bool split = rs.precision != 0;
    // fp16 1-product with the fused preselection (needs one full sample tile of rows)
    const bool h1 = rs.precision == 3 && N >= H1_BN;
    const bool h2 = rs.precision >= 2;  // fp16 row plane (1- and 2-product)
    // preselect width: the fp16 2-product scores carry a ~2x larger error bound, so the
    // kk-th score must sit further from the k-th distance for the certificate
    const int kk = h->exact_kk > 0 ? std::min(256, std::max(h->exact_kk, k))
                                   : std::min(256, h2 ? std::max(2 * k, 64) : std::max(2 * k, k + 16));
    const int64_t ldS = (N + 255) / 256 * 256;
    const int64_t budget = (int64_t)4 << 30;  // score workspace bytes
    int64_t qc = std::max<int64_t>(1, std::min<int64_t>(c.B, budget / (ldS * 4)));
    qc = std::min<int64_t>(qc, 4096);
    if ((r = ensure_buf(h, h->qnorm, (size_t)c.B)) ||
        (r = ensure_buf(h, h->cand, (size_t)qc * kk)) || (r = ensure_buf(h, h->xbound, (size_t)qc)) ||
        (r = ensure_buf(h, h->xflag, (size_t)qc)) || (r = ensure_buf(h, h->xflagged, (size_t)qc)) ||
        (r = ensure_buf(h, h->xnflag, 1)) || (r = ensure_buf(h, h->xmaxn, 1)))
        return r;
    // selection: enough (query, row-segment) waves to stream the score rows at full rate
    auto segs = [&](int64_t rows, int& ns, int64_t& sl) {
        ns = (int)std::min<int64_t>(16, std::max<int64_t>(1, (16384 + qc - 1) / qc));
        ns = (int)std::max<int64_t>(1, std::min<int64_t>(ns, (rows + 4095) / 4096));
        ns = std::max(1, std::min(ns, 1024 / kk));  // merge holds nseg * kk entries
        sl = ((rows + ns - 1) / ns + 1023) / 1024 * 1024;
    };
    int nseg;
    int64_t seglen;
    segs(N, nseg, seglen);
    int fnseg = nseg;
    int64_t fseglen = seglen;
    if (rs.ids) {
        segs(h->n, fnseg, fseglen);
        if ((r = ensure_buf(h, h->xsegd, (size_t)qc * fnseg * kk)) || (r = ensure_buf(h, h->xsegi, (size_t)qc * fnseg * kk)))
            return r;
    }
    if ((r = ensure_buf(h, h->xsegd, (size_t)qc * nseg * kk)) || (r = ensure_buf(h, h->xsegi, (size_t)qc * nseg * kk)))
        return r;
    // fused preselection (h1): the sample = every stride-th full row tile (about 32
    // tiles), its J-th best score per query is the threshold (J = kk when the
    // sample is every tile); a row passes at a rate of ~J / sample rows
    // the GEMM variant this search runs (exact_tile 0: the default, k_h1_pp16; a shape
    // it does not admit runs the ring kernel's filter)
    const int ev = h1_effective_variant(h->exact_tile, h->pitch, std::max<int64_t>(qc, rs.ld));
    const int bm = h1_tile_bm(ev);
    const int64_t nnt = (N + H1_BN - 1) / H1_BN, nqt = (qc + bm - 1) / bm;
    int stride;
    int64_t nsamp;  // sampled full tiles
    sample_shape(h, N, h1, stride, nsamp);
    const int J = stride < 8 ? kk : h->exact_thr_rank > 0 ? std::min(kk, std::max(k, h->exact_thr_rank)) : std::max(k, kk / 8);
    // the score workspace: every (query, row) score (precisions 0-2, and their
    // fallback), or only the sample's (fused path: its fallback streams distances
    // into per-segment lists, k_fallback_select)
    if ((r = ensure_buf(h, h->scores, (size_t)qc * (h1 ? (size_t)std::max<int64_t>(nsamp, 1) * H1_BN : (size_t)ldS))))
        return r;
    int sseg = 1;
    int64_t sseglen = 0;
    if (h1) {
        segs(nsamp * H1_BN, sseg, sseglen);
        sseg = std::max(1, std::min(sseg, 1024 / J));
    }
    // pairs per tile region / per query sub-bucket: 4x what the threshold lets
    // through on average (~J N / ns per query, ~bm J BN / ns per tile), with floors
    const int64_t ns = expect > 0 ? std::max<int64_t>(N, 1) : std::max<int64_t>(1, nsamp * H1_BN);
    const int64_t Jc = expect > 0 ? expect : J;
    // (a multiple of 8: k_h1_pp16 splits each tile's region among its 8 waves)
    // record-mode variants: per wave 4x the expected records (<= one per passing pair,
    // at most 8 block rows x 64 lanes), H1_REC uint2 each
    const int rcap = h1_records(ev)
                         ? 8 * H1_REC * (int)std::min<int64_t>(512, std::max<int64_t>(64, 4 * bm * Jc * H1_BN / ns / 8))
                         : (int)std::min<int64_t>((int64_t)bm * H1_BN, std::max<int64_t>(2048, 4 * bm * Jc * H1_BN / ns) + 7) / 8 * 8;
    const int rsub = h1_region_split(ev);
    // (a range search: 8x the expected hits, at least 128 per sub-bucket -- a query that passes
    // more is answered by the sweep, so the floor only has to cover what the radius lets through)
    // (a row tile goes to sub-bucket tile % H1_BSUB: a small index, or a selective filter's row
    // set, of fewer tiles than that uses only so many sub-buckets, and the range search spreads
    // its 8x over the ones in use)
    const int64_t subs = expect > 0 ? std::min<int64_t>(H1_BSUB, std::max<int64_t>(nnt, 1)) : H1_BSUB;
    const int scap = (int)std::min<int64_t>(std::max<int64_t>(N, 1),
                                            std::max<int64_t>(expect > 0 ? 128 : 512, 8 * Jc * N / ns / subs));
    if (h1 && ((r = ensure_buf(h, h->h1thr, (size_t)qc)) || (r = ensure_buf(h, h->h1c, (size_t)nqt * bm + 256)) ||
               (r = ensure_buf(h, h->h1s, (size_t)nqt * bm + 256)) ||
               (r = ensure_buf(h, h->h1region, (size_t)nqt * nnt * rcap)) ||
               (r = ensure_buf(h, h->h1rcnt, (size_t)nqt * nnt * rsub)) ||
               (r = ensure_buf(h, h->h1xw, (size_t)std::max<int64_t>(N, 1) * 4)) ||
               (r = ensure_buf(h, h->h1qcnt, (size_t)qc * H1_BSUB * H1_CSTRIDE)) || (r = ensure_buf(h, h->h1ovf, (size_t)qc)) ||
               (r = ensure_buf(h, h->h1bucket, (size_t)qc * H1_BSUB * scap)) || (r = ensure_buf(h, h->qerr, 1)) ||
               (r = ensure_buf(h, h->xsegd, (size_t)qc * sseg * J)) ||
               (r = ensure_buf(h, h->xsegi, (size_t)qc * sseg * J))))
        return r;
    if (split) {
        const int64_t plane = h->capn * h->pitch;
        const int kind = h2 ? 2 : 1;
        if (h->xsplit.n < (size_t)plane * 2 || h->xsplit_plane != plane || h->xsplit_kind != kind) {
            if ((r = ensure_buf(h, h->xsplit, (size_t)plane * 2))) return r;
            h->xsplit_rows = 0;
            h->xsplit_plane = plane;
            h->xsplit_kind = kind;
        }
        if ((r = ensure_buf(h, h->qsplit, (size_t)qc * h->pitch * 2))) return r;
        if (h2 && ((r = ensure_buf(h, h->xinv, (size_t)h->capn)) || (r = ensure_buf(h, h->qinv, (size_t)qc)) ||
                   (r = ensure_buf(h, h->xerr, 1))))
            return r;
    }
    LCHK(h, launch_norms(h->qpad.p, 0, c.B, h->pitch, h->lpr, h->vpl, h->qnorm.p, s));
    if ((r = sync_layer_table(h)) || (r = order_meta(h, s))) return r;
    GraphDev g = graph_view(h);
    g.err = c.errw;
    const uint8_t* xdead;
    if ((r = exact_skipped(h, s, xdead))) return r;
    g.dead = xdead;
    // certificate constants (u = 2^-24; gamma_n = n u / (1 - n u) bounds any
    // order of n-term f32 summation relative to the sum of magnitudes)
    const double u = std::ldexp(1.0, -24);
    auto gam = [&](double nn) { return nn * u / (1.0 - nn * u); };
    // products per element: f32 1, bf16x3 3, fp16 2-product 2, fp16 1-product 1.  Split
    // error: bf16x3 drops ql.xl and the planes' tails (3.02 * 2^-16); fp16 2-product
    // rounds the rows to fp16 (2^-11 |x|, Cauchy-Schwarz) and the queries to hi + lo
    // (2^-21); fp16 1-product rounds both once
    const double g_mfma = gam((h1 ? 1.0 : h2 ? 2.0 : split ? 3.0 : 1.0) * h->pitch + 1);
    // (fp16: the rows' part -- and the queries' in the 1-product -- is the measured
    // max |x' - x| / |x| <= 2^-11, added on the device)
    const double e_split = h1 ? 0.0 : h2 ? std::ldexp(1.0, -21) : split ? 3.02 * std::ldexp(1.0, -16) : 0.0;
    const double g_can = gam(4.0 * h->vpl + 8);  // canonical: 4*VPL fmaf per lane + 6 butterfly levels
    CertArgs cert{};
    cert.qnorm = h->qnorm.p;
    cert.xmax = h->xmaxn.p;
    cert.eps_cos = (float)(1.01 * ((g_mfma + e_split + g_can) * (1.0 + 1e-4) + 16 * u));
    cert.eps_dot = (float)(1.01 * (g_mfma + e_split + g_can));
    cert.c_l2 = (float)(1.01 * (2.0 * gam(4.0 * h->vpl + 10) + 16 * u));
    cert.flag = h->xflag.p;
    cert.flagged = h->xflagged.p;
    cert.nflag = h->xnflag.p;
    cert.stats = h->d_stats + 3;
    cert.xerr = h2 ? h->xerr.p : nullptr;
    cert.qerr = h1 ? h->qerr.p : nullptr;
    plan = ExactPlan{split, h1, h2, kk, nseg, ev, bm, stride, J, sseg, rcap, rsub, scap, ldS, qc, seglen, nnt, nsamp, sseglen,
                     xdead, g, cert, rs, fnseg, fseglen};
    return 0;
}

// the exact path's kernels: per chunk of qc queries the scores, the selection, the re-rank and the fallback
static int exact_run(mhnsw_index* h, const SearchCall& c, const ExactPlan& plan) {
    const auto& [split, h1, h2, kk, nseg, ev, bm, stride, J, sseg, rcap, rsub, scap, ldS, qc, seglen, nnt, nsamp, sseglen,
                 xdead, g, cert, rs, fnseg, fseglen] = plan;
    const int k = c.k;
    hipStream_t s = c.s;
    const bool gathered = rs.ids != nullptr;
    const bool marks = gathered && c.timing;  // the stage marks of a filtered exact search
    if (c.timing) HIPCHK(h, hipEventRecord(h->ev0, s));
    if (marks) HIPCHK(h, hipEventRecord(h->fxev[0], s));
    if (split && h->xsplit_rows < h->n) {
        uint16_t* xh = h->xsplit.p;
        uint16_t* xl = h->xsplit.p + (size_t)h->capn * h->pitch;
        if (h2) {
            if (h->xsplit_rows == 0) HIPCHK(h, hipMemsetAsync(h->xerr.p, 0, sizeof(float), s));
            LCHK(h, launch_split_h16(h->vecs, h->xsplit_rows, h->n, h->pitch, h->capn, xh, nullptr, h->xinv.p,
                                     h->xerr.p, s));
        }
        else
            LCHK(h, launch_split_rows(h->vecs, h->xsplit_rows, h->n, h->pitch, h->capn, xh, xl, s));
        h->xsplit_rows = h->n;
    }
    // the set's plane, per-row constants and masked rows: the handle's, or the allowed rows'
    // gathered from them (the measured rounding bound xerr of every row holds for a subset)
    const uint16_t* Xh = h->xsplit.p;
    int64_t ldX = h->capn;
    const float* xinv = h->xinv.p;
    const float* xnorm = h->norms;
    const uint8_t* sdead = xdead;
    if (gathered) {
        LCHK(h, launch_rowset_compact(rs.filter, rs.fwords, xdead, h->n, h->fxwords.p, h->fxmask.p, h->fxcnt.p,
                                      h->fxids.p, rs.n, s));
        if (marks) HIPCHK(h, hipEventRecord(h->fxev[1], s));
        LCHK(h, launch_rowset_gather(h->xsplit.p, h->capn, rs.ids, rs.n, h->pitch, h->fxplane.p, rs.ld, h->xinv.p,
                                     h->norms, h->fxinv.p, h->fxnorm.p, s));
        if (marks) HIPCHK(h, hipEventRecord(h->fxev[2], s));
        Xh = h->fxplane.p;
        ldX = rs.ld;
        xinv = h->fxinv.p;
        xnorm = h->fxnorm.p;
        sdead = nullptr;
    }
    if (h->metric == EUCLIDEAN) {
        HIPCHK(h, hipMemsetAsync(h->xmaxn.p, 0, sizeof(float), s));
        LCHK(h, launch_max_norm(h->norms, h->n, h->xmaxn.p, s));
    }
    for (int64_t q0 = 0; q0 < c.B; q0 += qc) {
        const int64_t nb = std::min(qc, c.B - q0);
        ExactArgs a{};
        a.X = h->vecs;
        a.xnorm = xnorm;
        a.dead = sdead;
        a.N = rs.n;
        a.Q = h->qpad.p + (size_t)q0 * h->pitch;
        a.qnorm = h->qnorm.p + q0;
        a.B = nb;
        a.pitch = h->pitch;
        a.dim = h->dim;
        a.metric = h->metric;
        a.scores = h->scores.p;
        a.ldS = ldS;
        a.kk = kk;
        a.cand = h->cand.p;
        a.bound = h->xbound.p;
        a.nseg = nseg;
        a.seglen = seglen;
        a.seg_d = h->xsegd.p;
        a.seg_i = h->xsegi.p;
        int64_t* ok_ = c.dk + q0 * k;
        float* od_ = c.dd + q0 * k;
        int32_t* on_ = c.dn + q0;
        int32_t* oi_ = c.out_ids ? c.out_ids + q0 * k : nullptr;
        if (split) {
            a.Xh = Xh;
            a.Xl = Xh + (size_t)ldX * h->pitch;  // (bf16x3 only: never a gathered set's)
            a.ldXs = ldX;
            a.Qh = h->qsplit.p;
            a.Ql = h->qsplit.p + (size_t)qc * h->pitch;
            a.ldQs = qc;
            if (h1) {
                a.xinv = xinv;
                a.qinv = h->qinv.p;
                HIPCHK(h, hipMemsetAsync(h->qerr.p, 0, sizeof(float), s));
                LCHK(h, launch_split_h16(a.Q, 0, nb, h->pitch, qc, h->qsplit.p, nullptr, h->qinv.p, h->qerr.p, s));
                // 1. sample: every score of the sampled row tiles -> the kk-th best per query
                ExactArgs as = a;
                as.tile_stride = stride;
                as.nsample_tiles = nsamp;
                as.ldS = nsamp * H1_BN;
                LCHK(h, launch_h1_sample(as, ev, s));
                as.N = nsamp * H1_BN;
                as.kk = J;
                as.nseg = sseg;
                as.seglen = sseglen;
                as.bound = h->h1thr.p;
                LCHK(h, launch_exact_select(as, s));
                // 2. the full GEMM keeps the pairs that can beat it; 3. per-query buckets; 4. top-kk
                LCHK(h, launch_ring_prep(h->h1thr.p, a.qnorm, a.qinv, nb, h->metric, h->h1c.p, h->h1s.p, s));
                HIPCHK(h, hipMemsetAsync(h->h1qcnt.p, 0, (size_t)nb * H1_BSUB * H1_CSTRIDE * 4, s));
                HIPCHK(h, hipMemsetAsync(h->h1ovf.p, 0, (size_t)nb, s));
                a.tile_stride = 1;
                a.ring_c = h->h1c.p;
                a.ring_s = h->h1s.p;
                a.region = h->h1region.p;
                a.region_cnt = h->h1rcnt.p;
                a.rcap = rcap;
                a.xw = reinterpret_cast<const float4*>(h->h1xw.p);
                if (q0 == 0)
                    LCHK(h, launch_h1_rowconst(xinv, xnorm, sdead, rs.n, h->metric,
                                               reinterpret_cast<float4*>(h->h1xw.p), s));
                if (c.timing && q0 == 0) HIPCHK(h, hipEventRecord(h->gev0, s));
                LCHK(h, launch_h1_filter(a, ev, s));
                if (c.timing && q0 == 0) {
                    HIPCHK(h, hipEventRecord(h->gev1, s));
                    h->have_gemm_timing = true;
                }
                const int64_t bqt = (nb + bm - 1) / bm;
                LCHK(h, launch_bucket(h->h1region.p, h->h1rcnt.p, rcap, bqt * nnt, bqt, bm, H1_BN, nb, h->h1qcnt.p,
                                      h->h1bucket.p, scap, h->h1ovf.p, rsub, h1_records(ev) ? 1 : 0, a, s));
                LCHK(h, launch_select_bucket(a, h->h1qcnt.p, h->h1bucket.p, scap, h->h1ovf.p, h->h1thr.p, s));
            } else if (h2) {
                a.xinv = xinv;
                a.qinv = h->qinv.p;
                LCHK(h, launch_split_h16(a.Q, 0, nb, h->pitch, qc, h->qsplit.p, h->qsplit.p + (size_t)qc * h->pitch,
                                         h->qinv.p, nullptr, s));
                LCHK(h, launch_exact_scores_x2h(a, h->exact_tile, s));
            } else {
                LCHK(h, launch_split_rows(a.Q, 0, nb, h->pitch, qc, h->qsplit.p,
                                          h->qsplit.p + (size_t)qc * h->pitch, s));
                LCHK(h, launch_exact_scores_x3(a, h->exact_tile, s));
            }
        } else {
            LCHK(h, launch_exact_scores(a, s));
        }
        if (!h1) LCHK(h, launch_exact_select(a, s));
        if (h1 && h1_timing_diag(ev)) continue;  // timing diagnostic: no re-rank, no results
        if (gathered) LCHK(h, launch_rowset_remap(h->cand.p, nb * kk, rs.ids, rs.n, s));
        const bool mark0 = marks && q0 == 0;
        if (mark0) HIPCHK(h, hipEventRecord(h->fxev[3], s));
        HIPCHK(h, hipMemsetAsync(h->xnflag.p, 0, sizeof(int32_t), s));
        CertArgs c1 = cert;
        c1.bound = h->xbound.p;
        c1.qnorm = h->qnorm.p + q0;
        LCHK(h, launch_rerank(a.Q, g, h->cand.p, kk, nb, h->lpr, h->vpl, k, ok_, od_, on_, oi_, c1, s));
        if (mark0) HIPCHK(h, hipEventRecord(h->fxev[4], s));
        // uncertified queries: canonical distances of every row, then select + re-rank again
        ExactArgs a2 = a;
        a2.only = h->xflag.p;
        a2.bound = nullptr;
        if (gathered) {
            // ... of every row of the index the call's mask lets through (the allowed rows: the
            // same canonical distances as the certified path's), candidates as row ids
            GraphDev gm = g;
            gm.dead = h->fxmask.p;
            a2.N = h->n;
            a2.nseg = fnseg;
            a2.seglen = fseglen;
            LCHK(h, launch_fallback_select(a.Q, gm, a2, h->lpr, h->vpl, s));
        } else if (h1) {
            LCHK(h, launch_fallback_select(a.Q, g, a2, h->lpr, h->vpl, s));
        } else {
            LCHK(h, launch_exact_fallback(a.Q, g, h->n, h->xflagged.p, h->xnflag.p, h->scores.p, ldS, h->lpr,
                                          h->vpl, s));
            LCHK(h, launch_exact_select(a2, s));
        }
        CertArgs c2{};
        c2.only = h->xflag.p;
        LCHK(h, launch_rerank(a.Q, g, h->cand.p, kk, nb, h->lpr, h->vpl, k, ok_, od_, on_, oi_, c2, s));
        if (mark0) HIPCHK(h, hipEventRecord(h->fxev[5], s));
    }
    if (c.timing) HIPCHK(h, hipEventRecord(h->ev1, s));
    h->have_fx_timing = marks;
    if (h1 && h1_timing_diag(ev))
        return fail(h, MHNSW_EUNSUPPORTED, "exact_tile %d is a timing diagnostic: no results", h->exact_tile);
    return 0;
}

static int wide_exact(mhnsw_index* h, SearchCall& c, const RowSet& rset);

// mhnsw_search*, and the candidate search of mhnsw_search_negatives
static int search_plain(mhnsw_index* h, SearchCall& c, int mode, int ef, const int64_t* entry_key) {
    int r = validate(h);
    if (r) return r;
    h->have_gemm_timing = false;  // last_gemm_ns describes this search or none
    if (mode == MHNSW_MODE_EXACT) h->wide_queries = 0;  // last_wide_* describe this exact search, however it ends
    if ((r = check_args(h, c, mode))) return r;
    if (c.B <= 0) return 0;
    if (!h->layers_exist || live_count(h) == 0) return zero_counts(h, c);
    if (ef <= 0) ef = h->ef;
    const int top = top_live_layer(h);
    uint32_t entry = (uint32_t)h->layers[top].entry;
    if (entry_key) {
        const int32_t e = key_row_in(h, *entry_key, top);
        if (e < 0) return fail(h, MHNSW_EINVAL, "entry key %lld not in top layer", (long long)*entry_key);
        entry = (uint32_t)e;
    }
    if ((r = stage(h, c))) return r;
    if (mode == MHNSW_MODE_EXACT) {
        ExactPlan plan;
        bool wide;
        if ((r = exact_k_limit(h, c.k, wide))) return r;
        if (wide) {  // (always at precision 3, as the range search)
            r = wide_exact(h, c, RowSet{h->n, h->capn, 3, nullptr, nullptr, 0});
            return r ? r : finish(h, c);
        }
        const RowSet every{h->n, h->capn, h->exact_precision, nullptr, nullptr, 0};
        if (!(r = exact_prepare(h, c, every, plan))) r = exact_run(h, c, plan);
    } else {
        const bool beam = mode == MHNSW_MODE_BEAM;
        SearchArgs a;
        if ((r = walk_args(h, c, top, entry, ef, beam && std::max(ef, c.k) >= h->beam_lds_min_ef, a))) return r;
        r = beam ? beam_search(h, c, a) : compat_search(h, c, a);
    }
    return r ? r : finish(h, c);
}

// The filtered walk's launch on c.s, for the filtered search and the filtered range search's
// beam mode: lists of the E best allowed rows per query (to c's outputs, staged here) through
// an LDS route list of W entries.  filter_of: a host array of checked ids (it is uploaded), or
// for a device call the device's.  timed: the walk's event pair is recorded.
static int filtered_walk(mhnsw_index* h, SearchCall& c, int E, int W, const int32_t* filter_of, bool timed) {
    int r;
    // a bitmap that has to grow with the rows moves: nothing enqueued may read it
    const size_t words = (size_t)((h->capn + 31) / 32);
    const auto grows = [&](const mhnsw_index::Filter& F) { return F.used && F.bits.size() < words; };
    if (std::any_of(h->filters.begin(), h->filters.end(), grows) && (r = drain(h))) return r;
    if ((r = filters_fit(h))) return r;
    const int top = top_live_layer(h);
    if (!c.on_device) {  // (the filtered call's own upload, next to stage()'s of the queries)
        if ((r = ensure_buf(h, h->fof, (size_t)c.B))) return r;
        HIPCHK(h, hipMemcpyAsync(h->fof.p, filter_of, (size_t)c.B * 4, hipMemcpyHostToDevice, c.s));
    }
    const FilterArgs f{h->d_filters, MHNSW_MAX_FILTERS, E, c.on_device ? filter_of : h->fof.p};
    if ((r = stage(h, c))) return r;
    SearchArgs a;  // (ef: the route list's width W, in LDS; FilterArgs::ef is the result list's)
    if ((r = walk_args(h, c, top, (uint32_t)h->layers[top].entry, W, true, a))) return r;
    a.mw_max_b = 0;
    a.expand = 1;
    if (timed) HIPCHK(h, hipEventRecord(h->ev0, c.s));
    const int lr = launch_search_beam_filtered(a, f, h->lpr, h->vpl, c.s);
    if (lr == -2)
        return fail(h, MHNSW_EUNSUPPORTED, "filtered search LDS budget exceeded (route=%d, vis_entries=%d)", W, a.vis_n);
    LCHK(h, lr);
    if (timed) HIPCHK(h, hipEventRecord(h->ev1, c.s));
    return 0;
}

// The filtered beam search (beam.hpp k_search_beam_filt): the fused launch over the LDS list of `route`
// entries, results from the list of max(ef, k) allowed rows.  Always timed (c.timing is set).
static int search_filtered(mhnsw_index* h, SearchCall& c, int ef, int route, const int32_t* filter_of) {
    int r = validate(h);
    if (r || (r = check_args(h, c, MHNSW_MODE_BEAM))) return r;
    if (ef <= 0) ef = h->ef;
    const int E = std::max(ef, c.k);
    if (E > 128) return fail(h, MHNSW_EUNSUPPORTED, "filtered search supports max(ef,k) <= 128");
    if (route <= 0) route = h->filter_route;
    const int W = std::max(route, E);
    if (W > 2048) return fail(h, MHNSW_EUNSUPPORTED, "filtered search supports route <= 2048");  // (LL_MAX_EF)
    if (c.B <= 0) return 0;
    if (!filter_of) return fail(h, MHNSW_EINVAL, "filter_of must be non-NULL");
    if (!c.on_device)
        for (int64_t b = 0; b < c.B; ++b) {
            const int32_t f = filter_of[b];
            if (f < -1 || (f >= 0 && (f >= (int)h->filters.size() || !h->filters[f].used)))
                return fail(h, MHNSW_EINVAL, "unknown filter %d", f);
        }
    if (!h->layers_exist || live_count(h) == 0) return zero_counts(h, c);
    if ((r = filtered_walk(h, c, E, W, filter_of, true))) return r;
    h->have_gemm_timing = false;
    return finish(h, c);
}

// The allowed rows of filter (a used slot) as a gathered row set, for the filtered exact search
// and the filtered range search: the host's count of them, the set's buffers sized for it, ids
// pointing at the list launch_rowset_compact fills.  rs.n == 0: nothing is allowed, and no
// buffer was touched.
static int filter_rowset(mhnsw_index* h, hipStream_t s, int filter, int precision, RowSet& rs) {
    int r;
    // a bitmap that has to grow with the rows moves: nothing enqueued may read it
    const size_t words = (size_t)((h->capn + 31) / 32);
    const auto grows = [&](const mhnsw_index::Filter& F) { return F.used && F.bits.size() < words; };
    if (std::any_of(h->filters.begin(), h->filters.end(), grows) && (r = drain(h))) return r;
    if ((r = filters_fit(h))) return r;
    const uint8_t* xdead;
    if ((r = exact_skipped(h, s, xdead))) return r;
    const mhnsw_index::Filter& F = h->filters[filter];
    const int64_t nwords = (h->n + 31) / 32, fwords = std::min<int64_t>(nwords, (int64_t)F.bits.size());
    int64_t m = 0;
    for (int64_t w = 0; w < fwords; ++w) {
        uint32_t bits = F.bits[(size_t)w];
        if (w == nwords - 1 && (h->n & 31)) bits &= (1u << (h->n & 31)) - 1u;
        if (!h->any_dead && !h->partial_rows) {
            m += __builtin_popcount(bits);
            continue;
        }
        for (; bits; bits &= bits - 1) {
            const int64_t i = w * 32 + __builtin_ctz(bits);
            m += !h->hdead[(size_t)i] && (!h->partial_rows || in_layer(h, i, 0));
        }
    }
    rs = RowSet{m, (m + 255) / 256 * 256, precision, nullptr, F.d, fwords};
    if (m == 0) return 0;
    if ((r = ensure_buf(h, h->fxwords, (size_t)nwords)) || (r = ensure_buf(h, h->fxmask, (size_t)nwords * 32)) ||
        (r = ensure_buf(h, h->fxcnt, (size_t)rowset_blocks(h->n))) || (r = ensure_buf(h, h->fxids, (size_t)m)) ||
        (r = ensure_buf(h, h->fxplane, (size_t)rs.ld * h->pitch)) || (r = ensure_buf(h, h->fxinv, (size_t)rs.ld)) ||
        (r = ensure_buf(h, h->fxnorm, (size_t)rs.ld)))
        return r;
    rs.ids = h->fxids.p;
    return 0;
}

// The filtered exact search of one filter (>= 0): the exact pipeline over the filter's allowed
// rows as a gathered row set.  The host's mirror of the bitmap sizes the launches (the same
// words and skipped rows the compaction kernel counts).  Always timed, with stage marks.
static int search_filtered_exact(mhnsw_index* h, SearchCall& c, int filter) {
    h->wide_queries = 0;  // last_wide_* describe this exact search, however it ends
    int r = validate(h);
    if (r || (r = check_args(h, c, MHNSW_MODE_EXACT))) return r;
    bool wide;
    if ((r = exact_k_limit(h, c.k, wide))) return r;
    if (filter < 0 || filter >= (int)h->filters.size() || !h->filters[filter].used)
        return fail(h, MHNSW_EINVAL, "unknown filter %d", filter);
    if (c.B <= 0) return 0;
    h->have_gemm_timing = false;
    h->have_fx_timing = false;
    if (!h->layers_exist || live_count(h) == 0) return zero_counts(h, c);
    // without an fp16 row plane (exact_precision 0 or 1) the call scores at precision 3
    RowSet rset;
    const int precision = wide ? 3 : h->exact_precision >= 2 ? h->exact_precision : 3;
    if ((r = filter_rowset(h, c.s, filter, precision, rset))) return r;
    if (rset.n == 0) {  // nothing allowed: no row, no error
        h->stats_host[6] += c.B;
        h->have_timing = false;
        return zero_counts(h, c);
    }
    if ((r = stage(h, c))) return r;
    if (wide) {
        r = wide_exact(h, c, rset);
        return r ? r : finish(h, c);
    }
    ExactPlan plan;
    if (!(r = exact_prepare(h, c, rset, plan))) r = exact_run(h, c, plan);
    return r ? r : finish(h, c);
}

int search_filtered_exact_impl(mhnsw_index* h, const float* queries, bool on_device, int64_t B, int dim, int k, int filter,
                               int64_t* okeys, float* odist, int32_t* on, hipStream_t s, bool sticky) {
    // filter -1 (every live row) is the plain exact search
    if (filter == -1) return search_impl(h, queries, on_device, B, dim, k, MHNSW_MODE_EXACT, 0, nullptr, okeys, odist, on, s,
                                         true, nullptr, sticky);
    SearchCall c{queries, on_device, B, dim, k, okeys, odist, on, nullptr, s, sticky, true};
    return on_scratch(h, s, [&] { return search_filtered_exact(h, c, filter); });
}

int search_impl(mhnsw_index* h, const float* queries, bool on_device, int64_t B, int dim, int k, int mode, int ef,
                const int64_t* entry_key, int64_t* okeys, float* odist, int32_t* on, hipStream_t s, bool timing,
                int32_t* out_ids, bool sticky) {
    SearchCall c{queries, on_device, B, dim, k, okeys, odist, on, out_ids, s, sticky, timing};
    return on_scratch(h, s, [&] { return search_plain(h, c, mode, ef, entry_key); });
}

int search_filtered_impl(mhnsw_index* h, const float* queries, bool on_device, int64_t B, int dim, int k, int ef, int route,
                         const int32_t* filter_of, int64_t* okeys, float* odist, int32_t* on, hipStream_t s,
                         bool sticky) {
    SearchCall c{queries, on_device, B, dim, k, okeys, odist, on, nullptr, s, sticky, true};
    return on_scratch(h, s, [&] { return search_filtered(h, c, ef, route, filter_of); });
}

// ---- range search: every row within a per-query radius (range.hip; DESIGN.md "Range search") ----
// Where a range search's ragged result goes, all on the device: lims [B + 1], keys / dist [cap].
struct RangeOut {
    const float* radius;  // [B]
    int64_t cap;
    int64_t* lims;
    int64_t* keys;
    float* dist;
};
// The rows a range search is over.  Exact mode: one filter for the call (-1: every live row).
// Beam mode: walk set, the filtered walk through a route list, a filter per query in filter_of
// (a host array, or for a device call nullptr: `filter` for every query).
struct RangeRows {
    int filter = -1;
    bool walk = false;
    int route = 0;
    const int32_t* filter_of = nullptr;
};

// Exact mode.  Per chunk of queries: the radius as the filter GEMM's threshold, the filter and
// the buckets as exact_run runs them, the canonical refine of the candidates, the sweep for the
// queries the filter does not cover; counts, then the chunk's part of lims, then the writes.
// Once per call: each query's segment of the hit buffer sorted, keys and distances emitted.
// The plan's row set is every row of the index, or a filter's allowed rows: then the id list
// is compacted and the rows' plane gathered first (as exact_run does), the GEMM runs over the
// gathered plane, refine maps its positions to row ids and the sweep walks the id list.
// A wide exact search (wide_exact) runs the same stages with two differences: each chunk's
// radii are estimated first (the sample pass and k_wide_radius write them into o.radius's
// buffer), and the sorted segments are cut at k into the call's [B, k] outputs, the short
// queries answered by the fallback select, instead of being emitted whole.
struct WideRun {
    int k, J;             // the call's k; the rank of the sample score that becomes the radius
    float* radius;        // [B] == o.radius
    int64_t* dk;          // the call's outputs on the device
    float* dd;
    int32_t* dn;
    int32_t* out_ids;
};
static int wide_cut(mhnsw_index* h, const SearchCall& c, const ExactPlan& plan, const RangeOut& o, const WideRun& w,
                    int64_t hcap, size_t tmp_bytes);

static int range_exact(mhnsw_index* h, const SearchCall& c, const ExactPlan& plan, const RangeOut& o,
                       const WideRun* w = nullptr) {
    int r;
    hipStream_t s = c.s;
    const RowSet& rs = plan.rs;
    const bool gathered = rs.ids != nullptr;
    const int force = w ? 0 : h->range_force_fallback;  // (the range search's test option is not the wide search's)
    const bool fused = plan.h1 && !force;
    const int64_t qc = plan.qc, B = c.B;
    const int64_t hcap = o.cap + rs.n;  // a query that starts below cap holds all its hits (<= the set's rows)
    if (hcap > (int64_t)0x7fffffff)
        return fail(h, MHNSW_EUNSUPPORTED, "range search supports cap + rows < 2^31");
    size_t tmp_bytes = 0;
    LCHK(h, range_sort_temp_bytes(hcap, B, &tmp_bytes));
    if ((r = ensure_buf(h, h->rthr, (size_t)qc)) || (r = ensure_buf(h, h->rstate, (size_t)qc)) ||
        (r = ensure_buf(h, h->rsweep, (size_t)qc)) || (r = ensure_buf(h, h->rcnt, (size_t)qc)) ||
        (r = ensure_buf(h, h->rcursor, (size_t)qc)) || (r = ensure_buf(h, h->rseg, (size_t)2 * B)) ||
        (r = ensure_buf(h, h->rhits, (size_t)2 * hcap)) || (r = ensure_buf(h, h->rtmp, std::max<size_t>(tmp_bytes, 1))))
        return r;
    if (fused && h->xsplit_rows < h->n) {
        if (h->xsplit_rows == 0) HIPCHK(h, hipMemsetAsync(h->xerr.p, 0, sizeof(float), s));
        LCHK(h, launch_split_h16(h->vecs, h->xsplit_rows, h->n, h->pitch, h->capn, h->xsplit.p, nullptr, h->xinv.p,
                                 h->xerr.p, s));
        h->xsplit_rows = h->n;
    }
    // the set's plane and per-row constants: the handle's, or the allowed rows' gathered from
    // them (xerr, and below the L2 xmax, stay maxima over every row: bounds that hold for a subset)
    const uint16_t* Xh = h->xsplit.p;
    int64_t ldX = h->capn;
    const float* xinv = h->xinv.p;
    const float* xnorm = h->norms;
    const uint8_t* sdead = plan.xdead;
    if (gathered) {
        const bool marks = c.timing;  // options last_fx_compact_ns / last_fx_gather_ns
        if (marks) HIPCHK(h, hipEventRecord(h->fxev[6], s));
        LCHK(h, launch_rowset_compact(rs.filter, rs.fwords, plan.xdead, h->n, h->fxwords.p, h->fxmask.p, h->fxcnt.p,
                                      h->fxids.p, rs.n, s));
        if (marks) HIPCHK(h, hipEventRecord(h->fxev[7], s));
        if (fused) {  // (a swept search reads the f32 rows through the id list: no plane)
            LCHK(h, launch_rowset_gather(h->xsplit.p, h->capn, rs.ids, rs.n, h->pitch, h->fxplane.p, rs.ld, h->xinv.p,
                                         h->norms, h->fxinv.p, h->fxnorm.p, s));
            Xh = h->fxplane.p;
            ldX = rs.ld;
            xinv = h->fxinv.p;
            xnorm = h->fxnorm.p;
            sdead = nullptr;
        }
        if (marks) HIPCHK(h, hipEventRecord(h->fxev[8], s));
        h->have_rs_timing = marks;
    }
    if (h->metric == EUCLIDEAN) {
        HIPCHK(h, hipMemsetAsync(h->xmaxn.p, 0, sizeof(float), s));
        LCHK(h, launch_max_norm(h->norms, h->n, h->xmaxn.p, s));
    }
    for (int64_t q0 = 0; q0 < B; q0 += qc) {
        const int64_t nb = std::min(qc, B - q0);
        RangeArgs ra{};
        ra.ids = rs.ids;
        ra.m = rs.n;
        ra.g = plan.g;
        ra.Q = h->qpad.p + (size_t)q0 * h->pitch;
        ra.radius = o.radius + q0;
        ra.B = nb;
        ra.qcnt = h->h1qcnt.p;
        ra.bucket = h->h1bucket.p;
        ra.scap = plan.scap;
        ra.qovf = h->h1ovf.p;
        ra.state = h->rstate.p;
        ra.sweep = h->rsweep.p;
        ra.cnt = h->rcnt.p;
        ra.cursor = h->rcursor.p;
        ra.lims = o.lims + q0;
        ra.hits = h->rhits.p;
        ra.hcap = hcap;
        ra.cap = o.cap;
        ra.stat = h->rstat.p;
        CertArgs c1 = plan.cert;
        c1.qnorm = h->qnorm.p + q0;
        const bool mark0 = c.timing && q0 == 0;  // the stage marks: the first chunk's stages, and the order stage
        if (mark0) HIPCHK(h, hipEventRecord(h->fxev[0], s));
        if (fused) {
            HIPCHK(h, hipMemsetAsync(h->qerr.p, 0, sizeof(float), s));
            LCHK(h, launch_split_h16(ra.Q, 0, nb, h->pitch, qc, h->qsplit.p, nullptr, h->qinv.p, h->qerr.p, s));
        }
        if (w) {
            // 0. (wide exact search) the sample pass as exact_run runs it, then the radii
            const bool wmark = c.timing && q0 == 0;
            if (wmark) HIPCHK(h, hipEventRecord(h->wev[0], s));
            const bool sample = fused && !h->wide_force_fallback && plan.nsamp * H1_BN >= w->J;
            if (sample) {
                ExactArgs as{};
                as.X = h->vecs;
                as.xnorm = xnorm;
                as.dead = sdead;
                as.N = rs.n;
                as.Q = ra.Q;
                as.qnorm = c1.qnorm;
                as.B = nb;
                as.pitch = h->pitch;
                as.dim = h->dim;
                as.metric = h->metric;
                as.scores = h->scores.p;
                as.Xh = Xh;
                as.Xl = Xh + (size_t)ldX * h->pitch;
                as.ldXs = ldX;
                as.Qh = h->qsplit.p;
                as.Ql = h->qsplit.p + (size_t)qc * h->pitch;
                as.ldQs = qc;
                as.xinv = xinv;
                as.qinv = h->qinv.p;
                as.tile_stride = plan.stride;
                as.nsample_tiles = plan.nsamp;
                as.ldS = plan.nsamp * H1_BN;
                LCHK(h, launch_h1_sample(as, plan.ev, s));
            }
            if (wmark) HIPCHK(h, hipEventRecord(h->wev[1], s));
            WideRadiusArgs wr{};
            wr.scores = h->scores.p;
            wr.ldS = plan.nsamp * H1_BN;
            wr.ns = sample ? plan.nsamp * H1_BN : 0;
            wr.J = w->J;
            wr.metric = h->metric;
            wr.force = h->wide_force_fallback;
            wr.qnorm = c1.qnorm;
            wr.qinv = h->qinv.p;
            wr.c = c1;
            wr.B = nb;
            wr.radius = w->radius + q0;
            LCHK(h, launch_wide_radius(wr, s));
            if (wmark) HIPCHK(h, hipEventRecord(h->wev[2], s));
        }
        // 1. the radius as the score threshold, and each query's path
        LCHK(h, launch_range_thr(ra, c1.qnorm, fused ? h->qinv.p : nullptr, c1, force ? -1 : fused ? 1 : 0, h->rthr.p, s));
        if (fused) {
            // 2. the filter GEMM and the per-query buckets, as the top-k search runs them
            ExactArgs a{};
            a.X = h->vecs;
            a.xnorm = xnorm;
            a.dead = sdead;
            a.N = rs.n;
            a.Q = ra.Q;
            a.qnorm = c1.qnorm;
            a.B = nb;
            a.pitch = h->pitch;
            a.dim = h->dim;
            a.metric = h->metric;
            a.Xh = Xh;
            a.Xl = Xh + (size_t)ldX * h->pitch;
            a.ldXs = ldX;
            a.Qh = h->qsplit.p;
            a.Ql = h->qsplit.p + (size_t)qc * h->pitch;
            a.ldQs = qc;
            a.xinv = xinv;
            a.qinv = h->qinv.p;
            LCHK(h, launch_ring_prep(h->rthr.p, a.qnorm, a.qinv, nb, h->metric, h->h1c.p, h->h1s.p, s));
            HIPCHK(h, hipMemsetAsync(h->h1qcnt.p, 0, (size_t)nb * H1_BSUB * H1_CSTRIDE * 4, s));
            HIPCHK(h, hipMemsetAsync(h->h1ovf.p, 0, (size_t)nb, s));
            a.tile_stride = 1;
            a.ring_c = h->h1c.p;
            a.ring_s = h->h1s.p;
            a.region = h->h1region.p;
            a.region_cnt = h->h1rcnt.p;
            a.rcap = plan.rcap;
            a.xw = reinterpret_cast<const float4*>(h->h1xw.p);
            if (q0 == 0)
                LCHK(h, launch_h1_rowconst(a.xinv, a.xnorm, a.dead, a.N, h->metric, reinterpret_cast<float4*>(h->h1xw.p), s));
            if (c.timing && q0 == 0) HIPCHK(h, hipEventRecord(h->gev0, s));
            LCHK(h, launch_h1_filter(a, plan.ev, s));
            if (c.timing && q0 == 0) {
                HIPCHK(h, hipEventRecord(h->gev1, s));
                h->have_gemm_timing = true;
            }
            const int64_t bqt = (nb + plan.bm - 1) / plan.bm;
            LCHK(h, launch_bucket(h->h1region.p, h->h1rcnt.p, plan.rcap, bqt * plan.nnt, bqt, plan.bm, H1_BN, nb,
                                  h->h1qcnt.p, h->h1bucket.p, plan.scap, h->h1ovf.p, plan.rsub,
                                  h1_records(plan.ev) ? 1 : 0, a, s));
            if (mark0) HIPCHK(h, hipEventRecord(h->fxev[1], s));
            // 3. canonical check of the candidates, the hits compacted in their sub-buckets
            LCHK(h, launch_range_refine(ra, h->lpr, h->vpl, s));
        } else if (mark0) {
            HIPCHK(h, hipEventRecord(h->fxev[1], s));
        }
        if (mark0) HIPCHK(h, hipEventRecord(h->fxev[2], s));
        // 4. the sweep's count, the chunk's prefix, then the writes into the queries' segments
        LCHK(h, launch_range_sweep(ra, rs.n, plan.nseg, plan.seglen, false, h->lpr, h->vpl, s));
        LCHK(h, launch_range_scan(h->rcnt.p, nb, ra.lims, h->rcursor.p, s));
        if (fused) LCHK(h, launch_range_gather(ra, s));
        LCHK(h, launch_range_sweep(ra, rs.n, plan.nseg, plan.seglen, true, h->lpr, h->vpl, s));
        if (mark0) HIPCHK(h, hipEventRecord(h->fxev[3], s));
        if (w && mark0) HIPCHK(h, hipEventRecord(h->wev[3], s));
    }
    if (c.timing) HIPCHK(h, hipEventRecord(h->fxev[4], s));
    // 5. order each query's segment by (distance, row id) and emit
    if (w) {
        if ((r = wide_cut(h, c, plan, o, *w, hcap, tmp_bytes))) return r;
    } else {
        LCHK(h, launch_range_order_emit(h->rhits.p, h->rhits.p + hcap, hcap, o.lims, B, o.cap, h->rseg.p, h->rseg.p + B,
                                        h->rtmp.p, tmp_bytes, plan.g, o.keys, o.dist, s));
    }
    if (c.timing) HIPCHK(h, hipEventRecord(h->fxev[5], s));
    h->have_range_timing = c.timing;
    if (fused && h1_timing_diag(plan.ev))
        return fail(h, MHNSW_EUNSUPPORTED, "exact_tile %d is a timing diagnostic: no results", h->exact_tile);
    return 0;
}

// ---- wide exact search: exact mode past k 256 (wide.hip; DESIGN.md "Wide exact search") ----
// The rank J of the sample score that becomes the radius, for a sample that holds the fraction
// f of the rows: the smallest J with P(Poisson(k f) >= J) <= 1e-5, at most k (wide.hip's
// header has the argument).  The pmf is summed in log space (k f reaches 4096).
static int wide_rank_for(int k, double f) {
    if (f >= 1.0) return k;
    const double lam = k * f, p = 1e-5;
    double cdf = 0.0;
    for (int j = 0; j < k; ++j) {  // cdf = P(X <= j - 1) here
        if (1.0 - cdf <= p) return std::max(j, 1);
        cdf += std::exp(-lam + j * std::log(lam) - std::lgamma(j + 1.0));
    }
    return k;
}

// Step 4 and 5 of a wide exact search, over the whole call: the segment sort, the cut at k,
// the fallback select for the short queries a group at a time (a group with no listed query
// exits at once, so nothing here waits for the list's length).
static int wide_cut(mhnsw_index* h, const SearchCall& c, const ExactPlan& plan, const RangeOut& o, const WideRun& w,
                    int64_t hcap, size_t tmp_bytes) {
    int r;
    hipStream_t s = c.s;
    const int64_t B = c.B;
    const int64_t ldW = (h->n + 63) / 64 * 64;
    const int64_t G = std::max<int64_t>(1, std::min<int64_t>(B, h->wide_fallback_bytes / (4 * ldW)));
    if ((r = ensure_buf(h, h->wdist, (size_t)G * ldW))) return r;
    if (c.timing) HIPCHK(h, hipEventRecord(h->wev[4], s));
    LCHK(h, launch_range_order(h->rhits.p, h->rhits.p + hcap, hcap, o.lims, B, o.cap, h->rseg.p, h->rseg.p + B,
                               h->rtmp.p, tmp_bytes, s));
    WideEmitArgs e{};
    e.sorted = h->rhits.p + hcap;
    e.lims = o.lims;
    e.B = B;
    e.cap = o.cap;
    e.k = w.k;
    e.keys = plan.g.keys;
    e.capn = plan.g.capn;
    e.out_keys = w.dk;
    e.out_dist = w.dd;
    e.out_n = w.dn;
    e.out_ids = w.out_ids;
    e.shortq = h->wshort.p;
    e.stat = h->wstat.p;
    LCHK(h, launch_wide_emit(e, s));
    if (c.timing) HIPCHK(h, hipEventRecord(h->wev[5], s));
    // the short queries: every row of the index the call's mask lets through (a filter's allowed
    // rows, as exact_run's gathered fallback reads them; else the rows the exact search skips)
    GraphDev gm = plan.g;
    if (plan.rs.ids) gm.dead = h->fxmask.p;
    for (int64_t g0 = 0; g0 < B; g0 += G)
        LCHK(h, launch_wide_fallback(h->qpad.p, gm, h->n, e, g0, std::min(G, B - g0), h->wdist.p, ldW, h->lpr, h->vpl, s));
    if (c.timing) HIPCHK(h, hipEventRecord(h->wev[6], s));
    h->have_wide_timing = c.timing;
    return 0;
}

// Exact mode at k up to 4096 over a row set (every row, or a filter's allowed rows): the range
// pipeline at radii estimated from the sample, cut at k (range_exact with a WideRun).  c is
// staged.  Room: the radius is the J-th smallest of a sample of fraction f, so the rows within
// it number about J / f with a standard deviation of sqrt(J (1 - f)) / f; the hit buffer holds
// (J + 4 sqrt(J (1 - f))) / f per query plus an eighth (the radius is widened by the score
// error) and 64, at most the row count.  Regions and sub-buckets are sized for the same number.
static int wide_exact(mhnsw_index* h, SearchCall& c, const RowSet& rset) {
    int r;
    hipStream_t s = c.s;
    const int k = c.k;
    const int64_t B = c.B, N = rset.n;
    for (auto& e : h->wev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    h->have_range_stats = false;
    h->have_range_timing = false;
    h->have_rs_timing = false;
    h->have_fx_timing = false;
    h->have_wide_timing = false;
    if (B > (int64_t)0x7fffffff) return fail(h, MHNSW_EUNSUPPORTED, "exact mode supports B < 2^31");
    int stride;
    int64_t nsamp;
    sample_shape(h, N, N >= H1_BN, stride, nsamp);
    const double f = N > 0 ? std::min(1.0, (double)(nsamp * H1_BN) / (double)N) : 0.0;
    const int J = f > 0.0 ? wide_rank_for(k, f) : k;
    int64_t room = 1;  // (no estimate: every query is short, and nothing reaches the hit buffer)
    if (f > 0.0 && J <= nsamp * H1_BN && !h->wide_force_fallback) {
        const double hits = (J + 4.0 * std::sqrt(J * (1.0 - f))) / f;
        room = std::min<int64_t>(N, (int64_t)std::ceil(hits * 1.125) + 64);
    }
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(B * room, (int64_t)0x7fffffff - N - 1));
    SearchCall c1 = c;
    c1.k = 1;  // (the exact path's workspace sizing, as the range search)
    ExactPlan plan;
    if ((r = exact_prepare(h, c1, rset, plan, room))) return r;
    if ((r = ensure_buf(h, h->wrad, (size_t)B)) || (r = ensure_buf(h, h->wlims, (size_t)B + 1)) ||
        (r = ensure_buf(h, h->wshort, (size_t)B)) || (r = ensure_buf(h, h->wstat, 2)) || (r = ensure_buf(h, h->rstat, 2)))
        return r;
    HIPCHK(h, hipMemsetAsync(h->wstat.p, 0, 16, s));
    HIPCHK(h, hipMemsetAsync(h->rstat.p, 0, 16, s));
    HIPCHK(h, hipMemsetAsync(h->wlims.p, 0, 8, s));
    if (c.timing) HIPCHK(h, hipEventRecord(h->ev0, s));
    const RangeOut o{h->wrad.p, cap, h->wlims.p, nullptr, nullptr};
    const WideRun w{k, J, h->wrad.p, c.dk, c.dd, c.dn, c.out_ids};
    if ((r = range_exact(h, c, plan, o, &w))) return r;
    if (c.timing) HIPCHK(h, hipEventRecord(h->ev1, s));
    h->wide_queries = B;
    h->wide_room = room;
    h->wide_rank = J;
    return 0;
}

// The kernels of one range search, enqueued on c.s.  c.k is set here: 1 in exact mode (the
// exact path's workspace sizing), ef in beam mode (the beam search's list).
static int range_search(mhnsw_index* h, SearchCall& c, int mode, int ef, const RangeOut& o,
                        const RangeRows& rows = RangeRows()) {
    int r = validate(h);
    if (r) return r;
    h->have_gemm_timing = false;
    h->have_range_stats = false;
    h->have_range_timing = false;
    h->have_rs_timing = false;
    h->have_fx_timing = false;  // (the stage events are shared with the filtered exact search)
    c.k = 1;
    if ((r = check_args(h, c, mode))) return r;
    if (mode == MHNSW_MODE_COMPAT) return fail(h, MHNSW_EUNSUPPORTED, "range search supports beam and exact mode");
    if (o.cap < 0) return fail(h, MHNSW_EINVAL, "cap must be >= 0, got %lld", (long long)o.cap);
    if (ef <= 0) ef = h->ef;
    const bool walk = rows.walk && mode == MHNSW_MODE_BEAM;
    int W = 0;
    if (walk) {  // the filtered walk's limits, in its words
        if (std::max(ef, 1) > 128) return fail(h, MHNSW_EUNSUPPORTED, "filtered search supports max(ef,k) <= 128");
        W = std::max(rows.route > 0 ? rows.route : h->filter_route, std::max(ef, 1));
        if (W > 2048) return fail(h, MHNSW_EUNSUPPORTED, "filtered search supports route <= 2048");  // (LL_MAX_EF)
    }
    if (mode == MHNSW_MODE_BEAM && std::max(ef, 1) > 2048)
        return fail(h, MHNSW_EUNSUPPORTED, "beam mode supports max(ef,k) <= 2048");
    const auto known = [&](int f) { return f == -1 || (f >= 0 && f < (int)h->filters.size() && h->filters[f].used); };
    if (!known(rows.filter)) return fail(h, MHNSW_EINVAL, "unknown filter %d", rows.filter);
    if (walk && rows.filter_of)
        for (int64_t b = 0; b < c.B; ++b)
            if (!known(rows.filter_of[b])) return fail(h, MHNSW_EINVAL, "unknown filter %d", rows.filter_of[b]);
    hipStream_t s = c.s;
    if (c.B <= 0 || !h->layers_exist || live_count(h) == 0) {  // no query or no row: all-zero lims
        HIPCHK(h, hipMemsetAsync(o.lims, 0, (size_t)(std::max<int64_t>(c.B, 0) + 1) * 8, s));
        if (!c.sticky) HIPCHK(h, hipMemsetAsync(h->d_err, 0, sizeof(int), s));
        return 0;
    }
    if (c.B > (int64_t)0x7fffffff) return fail(h, MHNSW_EUNSUPPORTED, "range search supports B < 2^31");
    if ((r = ensure_buf(h, h->rstat, 2))) return r;
    HIPCHK(h, hipMemsetAsync(h->rstat.p, 0, 16, s));
    HIPCHK(h, hipMemsetAsync(o.lims, 0, 8, s));
    const bool timing = c.timing;
    c.timing = false;  // the call's own bracket, below, not the beam search's
    if (mode == MHNSW_MODE_EXACT) {
        if ((r = stage(h, c))) return r;
        // like the filtered exact search, the call always scores at precision 3 (its results do
        // not depend on the precision)
        ExactPlan plan;
        RowSet rset{h->n, h->capn, 3, nullptr, nullptr, 0};
        if (rows.filter >= 0) {
            if ((r = filter_rowset(h, s, rows.filter, 3, rset))) return r;
            if (rset.n == 0) {  // nothing allowed: no hit, no error
                HIPCHK(h, hipMemsetAsync(o.lims, 0, (size_t)(c.B + 1) * 8, s));
                h->have_timing = false;
                h->have_range_stats = true;
                h->stats_host[6] += c.B;
                return 0;
            }
        }
        if ((r = exact_prepare(h, c, rset, plan, h->range_expect))) return r;
        if (timing) HIPCHK(h, hipEventRecord(h->ev0, s));
        c.timing = timing;
        if ((r = range_exact(h, c, plan, o))) return r;
    } else if (walk) {
        // the filtered walk at k = ef into the handle's scratch lists, then the cut
        c.k = std::max(ef, 1);
        if ((r = ensure_buf(h, h->okeys, (size_t)c.B * c.k)) || (r = ensure_buf(h, h->odist, (size_t)c.B * c.k)) ||
            (r = ensure_buf(h, h->on, (size_t)c.B)) || (r = ensure_buf(h, h->rcnt, (size_t)c.B)))
            return r;
        c.okeys = h->okeys.p;
        c.odist = h->odist.p;
        c.on = h->on.p;
        const int32_t* fof = rows.filter_of;
        if (c.on_device) {  // one id for the batch, filled on the stream
            if ((r = ensure_buf(h, h->fof, (size_t)c.B))) return r;
            HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->fof.p, rows.filter, (size_t)c.B, s));
            fof = h->fof.p;
        }
        if (timing) HIPCHK(h, hipEventRecord(h->ev0, s));
        if ((r = filtered_walk(h, c, c.k, W, fof, false))) return r;
        LCHK(h, launch_range_beam(h->okeys.p, h->odist.p, h->on.p, c.k, o.radius, c.B, h->rcnt.p, o.lims, o.cap, o.keys,
                                  o.dist, s));
    } else {
        c.k = std::max(ef, 1);
        const int top = top_live_layer(h);
        // the beam lists go to the handle's scratch, whoever owns the queries
        if ((r = ensure_buf(h, h->okeys, (size_t)c.B * c.k)) || (r = ensure_buf(h, h->odist, (size_t)c.B * c.k)) ||
            (r = ensure_buf(h, h->on, (size_t)c.B)) || (r = ensure_buf(h, h->rcnt, (size_t)c.B)))
            return r;
        c.okeys = h->okeys.p;
        c.odist = h->odist.p;
        c.on = h->on.p;
        if ((r = stage(h, c))) return r;
        SearchArgs a;
        if ((r = walk_args(h, c, top, (uint32_t)h->layers[top].entry, c.k, c.k >= h->beam_lds_min_ef, a))) return r;
        if (timing) HIPCHK(h, hipEventRecord(h->ev0, s));
        if ((r = beam_search(h, c, a))) return r;
        LCHK(h, launch_range_beam(h->okeys.p, h->odist.p, h->on.p, c.k, o.radius, c.B, h->rcnt.p, o.lims, o.cap, o.keys,
                                  o.dist, s));
    }
    if (timing) HIPCHK(h, hipEventRecord(h->ev1, s));
    h->have_timing = timing;
    h->have_range_stats = true;
    h->stats_host[6] += c.B;
    return 0;
}

int range_search_device_impl(mhnsw_index* h, const float* d_queries, int64_t B, int dim, const float* d_radius, int mode,
                             int ef, int64_t cap, int64_t* d_lims, int64_t* d_keys, float* d_dist, hipStream_t s) {
    SearchCall c{d_queries, true, B, dim, 1, nullptr, nullptr, nullptr, nullptr, s, true, true};
    const RangeOut o{d_radius, cap, d_lims, d_keys, d_dist};
    return on_scratch(h, s, [&] { return range_search(h, c, mode, ef, o); });
}

// the filtered range search on device buffers: one filter for the batch (-1: the plain call)
int range_search_filtered_device_impl(mhnsw_index* h, const float* d_queries, int64_t B, int dim, const float* d_radius,
                                      int mode, int ef, int route, int filter, int64_t cap, int64_t* d_lims,
                                      int64_t* d_keys, float* d_dist, hipStream_t s) {
    if (filter == -1) return range_search_device_impl(h, d_queries, B, dim, d_radius, mode, ef, cap, d_lims, d_keys, d_dist, s);
    SearchCall c{d_queries, true, B, dim, 1, nullptr, nullptr, nullptr, nullptr, s, true, true};
    const RangeOut o{d_radius, cap, d_lims, d_keys, d_dist};
    RangeRows rows;
    rows.filter = filter;
    rows.walk = true;
    rows.route = route;
    return on_scratch(h, s, [&] { return range_search(h, c, mode, ef, o, rows); });
}

// The host-pointer call: the device call into the handle's result buffers; when the hits did
// not fit, once more with room for exactly lims[B].  The results stay there for
// mhnsw_range_results.  (One pass on the handle's stream, inside on_scratch.)
static int range_host_pass(mhnsw_index* h, const float* queries, int64_t B, int dim, const float* radius, int mode,
                           int ef, const RangeRows& rows, int64_t* out_lims) {
    hipStream_t s = h->stream;
    int r;
    const int64_t nb = std::max<int64_t>(B, 0);
    if (nb > 0 && !radius) return fail(h, MHNSW_EINVAL, "radius must be non-NULL");
    if (!out_lims) return fail(h, MHNSW_EINVAL, "out_lims must be non-NULL");
    if ((r = ensure_buf(h, h->rrad, (size_t)std::max<int64_t>(nb, 1))) || (r = ensure_buf(h, h->rlims, (size_t)nb + 1)))
        return r;
    if (nb > 0) HIPCHK(h, hipMemcpyAsync(h->rrad.p, radius, (size_t)nb * 4, hipMemcpyHostToDevice, s));
    const int64_t room = std::max<int64_t>(0, (int64_t)0x7fffffff - h->n);
    int64_t cap = std::min(room, std::max<int64_t>({(int64_t)h->rkeys.n, 1024, nb * h->range_expect}));
    for (int pass = 0;; ++pass) {
        if ((r = ensure_buf(h, h->rkeys, (size_t)std::max<int64_t>(cap, 1))) ||
            (r = ensure_buf(h, h->rdist, (size_t)std::max<int64_t>(cap, 1))))
            return r;
        SearchCall c{queries, false, B, dim, 1, nullptr, nullptr, nullptr, nullptr, s, false, true};
        const RangeOut o{h->rrad.p, cap, h->rlims.p, h->rkeys.p, h->rdist.p};
        if ((r = range_search(h, c, mode, ef, o, rows))) return r;
        HIPCHK(h, hipMemcpyAsync(out_lims, h->rlims.p, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost, s));
        if ((r = read_error(h, s))) return r;
        if (out_lims[nb] <= cap) break;
        if (pass) return fail(h, MHNSW_EINTERNAL, "range search: %lld hits after room for %lld", (long long)out_lims[nb], (long long)cap);
        h->stats_host[6] -= nb;  // one search, run twice
        cap = out_lims[nb];
    }
    h->range_total = out_lims[nb];
    return 0;
}

int range_search_impl(mhnsw_index* h, const float* queries, int64_t B, int dim, const float* radius, int mode, int ef,
                      int64_t* out_lims) {
    h->range_total = -1;
    return on_scratch(h, h->stream,
                      [&] { return range_host_pass(h, queries, B, dim, radius, mode, ef, RangeRows(), out_lims); });
}

// b grown to `need` entries, its first `used` kept (a device copy on s)
template <class T>
static int grow_keep(mhnsw_index* h, DevBuf<T>& b, size_t used, size_t need, hipStream_t s) {
    if (b.n >= need) return 0;
    DevBuf<T> nb;
    int r = ensure_buf(h, nb, std::max(need, b.n * 2));
    if (r) return r;
    if (b.p && used) HIPCHK(h, hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (b.p) (void)hipFree(b.p);
    b = nb;
    return 0;
}

// The filtered host call.  Beam mode is one pass for any mix of filters (the walk takes one per
// query).  Exact mode runs one pass per distinct filter id (ascending) over that filter's
// queries; a pass leaves its sorted hits in the staging buffers, and once every count is known
// a device scatter (launch_range_place) moves each query's segment to its own place in the
// result -- only the passes' lims cross to the host.  The last_range_* options then describe
// the last pass.
int range_search_filtered_impl(mhnsw_index* h, const float* queries, int64_t B, int dim, const float* radius, int mode,
                               int ef, int route, const int32_t* filter_of, int64_t* out_lims) {
    h->range_total = -1;
    if (B > 0 && !filter_of) return fail(h, MHNSW_EINVAL, "filter_of must be non-NULL");
    std::map<int32_t, std::vector<int64_t>> groups;
    for (int64_t b = 0; b < B; ++b) groups[filter_of[b]].push_back(b);
    // filter -1 for every query is the plain range search
    if (groups.empty() || (groups.size() == 1 && groups.begin()->first == -1))
        return range_search_impl(h, queries, B, dim, radius, mode, ef, out_lims);
    hipStream_t s = h->stream;
    RangeRows rows;
    if (mode != MHNSW_MODE_EXACT || groups.size() == 1) {
        rows.walk = true;
        rows.route = route;
        rows.filter_of = filter_of;
        rows.filter = groups.size() == 1 ? groups.begin()->first : -1;
        return on_scratch(h, s, [&] { return range_host_pass(h, queries, B, dim, radius, mode, ef, rows, out_lims); });
    }
    // every argument error before the first pass leaves a result
    if (!radius) return fail(h, MHNSW_EINVAL, "radius must be non-NULL");
    if (!out_lims) return fail(h, MHNSW_EINVAL, "out_lims must be non-NULL");
    for (const auto& [f, qs] : groups)
        if (f < -1 || (f >= 0 && (f >= (int)h->filters.size() || !h->filters[f].used)))
            return fail(h, MHNSW_EINVAL, "unknown filter %d", f);
    return on_scratch(h, s, [&]() -> int {
        int r;
        std::vector<float> q, rad;
        std::vector<int64_t> glims, cnt((size_t)B), src((size_t)B);
        int64_t staged = 0;
        for (const auto& [f, qs] : groups) {
            const size_t R = qs.size();
            q.resize(R * (size_t)dim);
            rad.resize(R);
            glims.assign(R + 1, 0);
            for (size_t i = 0; i < R; ++i) {
                memcpy(&q[i * dim], queries + (size_t)qs[i] * dim, (size_t)dim * 4);
                rad[i] = radius[qs[i]];
            }
            rows.filter = f;
            if ((r = range_host_pass(h, q.data(), (int64_t)R, dim, rad.data(), mode, ef, rows, glims.data()))) {
                h->range_total = -1;
                return r;
            }
            const int64_t got = glims[R];
            h->range_total = -1;  // (the pass's hits are not the call's)
            if ((r = grow_keep(h, h->rgkeys, (size_t)staged, (size_t)(staged + got), s)) ||
                (r = grow_keep(h, h->rgdist, (size_t)staged, (size_t)(staged + got), s)))
                return r;
            if (got) {
                HIPCHK(h, hipMemcpyAsync(h->rgkeys.p + staged, h->rkeys.p, (size_t)got * 8, hipMemcpyDeviceToDevice, s));
                HIPCHK(h, hipMemcpyAsync(h->rgdist.p + staged, h->rdist.p, (size_t)got * 4, hipMemcpyDeviceToDevice, s));
            }
            for (size_t i = 0; i < R; ++i) {
                cnt[(size_t)qs[i]] = glims[i + 1] - glims[i];
                src[(size_t)qs[i]] = staged + glims[i];
            }
            staged += got;
        }
        out_lims[0] = 0;
        for (int64_t b = 0; b < B; ++b) out_lims[b + 1] = out_lims[b] + cnt[(size_t)b];
        const int64_t total = out_lims[B];
        if (total > (int64_t)0x7fffffff) return fail(h, MHNSW_EUNSUPPORTED, "range search supports cap + rows < 2^31");
        if ((r = ensure_buf(h, h->rlims, (size_t)B + 1)) || (r = ensure_buf(h, h->rgoff, (size_t)B)) ||
            (r = ensure_buf(h, h->rkeys, (size_t)std::max<int64_t>(total, 1))) ||
            (r = ensure_buf(h, h->rdist, (size_t)std::max<int64_t>(total, 1))))
            return r;
        HIPCHK(h, hipMemcpyAsync(h->rlims.p, out_lims, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(h->rgoff.p, src.data(), (size_t)B * 8, hipMemcpyHostToDevice, s));
        LCHK(h, launch_range_place(h->rgkeys.p, h->rgdist.p, h->rgoff.p, h->rlims.p, B, h->rkeys.p, h->rdist.p, s));
        HIPCHK(h, hipStreamSynchronize(s));
        h->range_total = total;
        return 0;
    });
}

}  // namespace mhh

extern "C" {

int mhnsw_search_negatives(mhnsw_index* h, const float* queries, int64_t B, int dim, const float* negatives,
                           const int32_t* neg_count, int k, float neg_weight, int mode, int ef, int flags,
                           int64_t* out_keys, float* out_score, int32_t* out_n) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    int r = validate(h);
    if (r) return r;
    if (k <= 0) return fail(h, MHNSW_EK, "k must be greater than 0, got %d", k);
    if (!(neg_weight >= 0.0f && neg_weight <= 1.0f))
        return fail(h, MHNSW_EINVAL, "negWeight must be between 0.0 and 1.0, got %f", (double)neg_weight);
    if (h->layers_exist && h->dim != dim)
        return fail(h, MHNSW_EDIM, "query embedding dimension mismatch: %d != %d", h->dim, dim);
    if (B <= 0) return 0;
    for (int64_t b = 0; b < B; ++b) out_n[b] = 0;
    if (!h->layers_exist || live_count(h) == 0) return 0;  // graph.go:1144-1146
    const int kx = std::max(3 * k, 10);                    // graph.go:1150-1153
    if (kx > NEG_MAX_CAND) return fail(h, MHNSW_EUNSUPPORTED, "negatives support k <= %d", NEG_MAX_CAND / 3);
    // queries without negatives are a plain Search(near, k) (graph.go:1395-1398)
    std::vector<int64_t> plain, rer;
    std::vector<int32_t> off(1, 0);
    for (int64_t b = 0; b < B; ++b) {
        if (neg_count[b] < 0) return fail(h, MHNSW_EINVAL, "negative count %d for query %lld", neg_count[b], (long long)b);
        (neg_count[b] == 0 ? plain : rer).push_back(b);
    }
    hipStream_t s = h->stream;
    auto scatter = [&](const std::vector<int64_t>& rows, const int64_t* kk, const float* ss, const int32_t* nn) {
        for (size_t i = 0; i < rows.size(); ++i) {
            memcpy(out_keys + (size_t)rows[i] * k, kk + i * k, (size_t)k * 8);
            memcpy(out_score + (size_t)rows[i] * k, ss + i * k, (size_t)k * 4);
            out_n[rows[i]] = nn[i];
        }
    };
    if (!plain.empty()) {
        std::vector<float> q(plain.size() * (size_t)dim);
        for (size_t i = 0; i < plain.size(); ++i)
            memcpy(&q[i * dim], queries + (size_t)plain[i] * dim, (size_t)dim * 4);
        std::vector<int64_t> kk(plain.size() * (size_t)k);
        std::vector<float> dd(plain.size() * (size_t)k);
        std::vector<int32_t> nn(plain.size());
        if ((r = search_impl(h, q.data(), false, (int64_t)plain.size(), dim, k, mode, ef, nullptr, kk.data(), dd.data(),
                             nn.data(), s, false)))
            return r;
        scatter(plain, kk.data(), dd.data(), nn.data());
    }
    if (rer.empty()) return 0;
    const int64_t R = (int64_t)rer.size();
    // gather the re-ranked queries; their negatives are `negatives` as given (the others have none)
    std::vector<float> q((size_t)R * dim);
    int64_t w = 0;
    for (int64_t i = 0; i < R; ++i) {
        const int64_t b = rer[(size_t)i];
        memcpy(&q[(size_t)i * dim], queries + (size_t)b * dim, (size_t)dim * 4);
        w += neg_count[b];
        off.push_back((int32_t)w);
    }
    if ((r = ensure_buf(h, h->nq, (size_t)R * dim)) || (r = ensure_buf(h, h->nneg, (size_t)std::max<int64_t>(w, 1) * h->pitch)) ||
        (r = ensure_buf(h, h->nck, (size_t)R * kx)) || (r = ensure_buf(h, h->ncd, (size_t)R * kx)) ||
        (r = ensure_buf(h, h->nci, (size_t)R * kx)) || (r = ensure_buf(h, h->ncn, (size_t)R)) ||
        (r = ensure_buf(h, h->noff, (size_t)R + 1)) || (r = ensure_buf(h, h->nok, (size_t)R * k)) ||
        (r = ensure_buf(h, h->nos, (size_t)R * k)) || (r = ensure_buf(h, h->non, (size_t)R)))
        return r;
    HIPCHK(h, hipMemcpyAsync(h->nq.p, q.data(), q.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->noff.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
    if (w > 0) {
        if ((r = ensure_buf(h, h->tmp, (size_t)w * dim))) return r;
        HIPCHK(h, hipMemcpyAsync(h->tmp.p, negatives, (size_t)w * dim * 4, hipMemcpyHostToDevice, s));
        LCHK(h, launch_pad_rows(h->tmp.p, w, dim, h->nneg.p, h->pitch, s));
    }
    // candidates: Search(near, kx) in the requested mode, internal ids kept
    if ((r = search_impl(h, h->nq.p, true, R, dim, kx, mode, ef, nullptr, h->nck.p, h->ncd.p, h->ncn.p, s, false,
                         h->nci.p)))
        return r;
    if ((r = sync_layer_table(h))) return r;
    NegArgs a;
    a.g = graph_view(h);
    a.neg = h->nneg.p;
    a.neg_off = h->noff.p;
    a.cand_ids = h->nci.p;
    a.cand_d = h->ncd.p;
    a.cand_n = h->ncn.p;
    a.B = R;
    a.kx = kx;
    a.k = k;
    a.w = neg_weight;
    a.flags = flags;
    a.out_keys = h->nok.p;
    a.out_score = h->nos.p;
    a.out_n = h->non.p;
    LCHK(h, launch_negatives(a, h->lpr, h->vpl, s));
    std::vector<int64_t> kk((size_t)R * k);
    std::vector<float> ss((size_t)R * k);
    std::vector<int32_t> nn((size_t)R);
    HIPCHK(h, hipMemcpyAsync(kk.data(), h->nok.p, kk.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(ss.data(), h->nos.p, ss.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(nn.data(), h->non.p, nn.size() * 4, hipMemcpyDeviceToHost, s));
    // the candidate search and the re-ranking report into d_err[0]
    if ((r = read_error(h, s))) return r;
    scatter(rer, kk.data(), ss.data(), nn.data());
    return 0;
}

}  // extern "C"
