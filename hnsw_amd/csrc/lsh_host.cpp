// lsh_host.cpp -- host side of the LSH index (hnsw-extensions/hybrid/lsh.go; kernels: lsh.hip;
// DESIGN.md §6 "LSH index"): the configuration and projections, the rows' codes kept current
// through the mutations, the lazily rebuilt tables, and the entry points that are not searches
// (mhnsw_lsh_enable / _hash / _codes / _projections).  The search itself is one more SearchCall
// of search_host.cpp (search_lsh).
#include "index.hpp"

using namespace mhh;

namespace mhh {

static int lsh_ppad(const mhnsw_index* h) {
    const int P = h->lsh_T * h->lsh_b;
    return (P + LSH_PPAD_UNIT - 1) / LSH_PPAD_UNIT * LSH_PPAD_UNIT;
}

// When is the MFMA's sign the canonical one?  Let S be the exact dot of x and p over d terms,
// s_m the MFMA's sum and s_c the canonical one (og_dev_sum).  Any order of d fused or unfused
// multiply-adds in f32 (u = 2^-24) is within gamma_d sum|x_i p_i| <= gamma_d |x| |p| of S,
// gamma_d = d u / (1 - d u) (Higham, Accuracy and Stability, §3.1; Cauchy-Schwarz).  So
// |s_m| > (gamma_m + gamma_c) |x| |p| gives |S| > gamma_c |x| |p|, hence sign(s_c) = sign(S) =
// sign(s_m).  gamma_c = gamma_d.  For the instruction nothing is documented beyond "f32
// multiply-accumulate": it is given 3 roundings per term (product, internal add, accumulator)
// instead of one, gamma_m = 3 gamma_d.  The stored norms are themselves computed in f32 (within
// (1 + gamma_d) of |x|, |p|) and the bound is evaluated in f32: another factor 1.01.  Hence
// margin = 4.04 gamma_d, twice the standard 2 gamma_d.  Absolute terms, for what the relative
// bound does not cover: a subnormal element the instruction may flush (each at most 2^-126
// times the other vector's element, over d terms: d 2^-126 (|x| + |p|) covers both sides) and
// a flushed subnormal sum or a product that underflows (d 2^-120, generously).  A NaN or
// infinite sum or bound is never trusted (the kernel tests !(|s| > bound)).
static void lsh_margin(int d, float& margin, float& abs_rel, float& abs_min) {
    const double u = 5.9604644775390625e-08, g = d * u / (1.0 - d * u);
    margin = (float)(4.04 * g * (1.0 + 1e-6));
    abs_rel = (float)((double)d * 1.1754943508222875e-38);  // d 2^-126
    abs_min = (float)((double)d * 7.52316384526264e-37);    // d 2^-120
}

void lsh_free(mhnsw_index* h) {
    auto F = [](auto*& p) {
        if (p) (void)hipFree(p);
        p = nullptr;
    };
    F(h->lsh_dproj);
    F(h->lsh_pnorm);
    F(h->lsh_work);
    F(h->lsh_wcnt);
    F(h->lsh_stat);
    F(h->lsh_codes.p);
    F(h->lsh_scode.p);
    F(h->lsh_sid.p);
    F(h->lsh_qcodes.p);
    F(h->lsh_key.p);
    F(h->lsh_val.p);
    F(h->lsh_tmp.p);
    F(h->lsh_ncand.p);
    h->lsh_codes.n = h->lsh_scode.n = h->lsh_sid.n = h->lsh_qcodes.n = h->lsh_key.n = h->lsh_val.n = 0;
    h->lsh_tmp.n = h->lsh_ncand.n = 0;
    if (h->lev0) (void)hipEventDestroy(h->lev0);
    if (h->lev1) (void)hipEventDestroy(h->lev1);
    h->lev0 = h->lev1 = nullptr;
}

// The projections on the device for the handle's dimension: generated ones are drawn now
// (lsh.go:64-92's order, one SplitMix64 stream from the seed; the reference's positive scale
// 1 / sum p^2 cannot change a sign and is left out), a caller's must have that dimension.
static int lsh_prepare(mhnsw_index* h) {
    if (!h->lsh_T || h->dim <= 0) return 0;
    const int P = h->lsh_T * h->lsh_b, ppad = lsh_ppad(h);
    if (h->lsh_dproj && h->lsh_pdim == h->dim) return 0;
    if (h->lsh_user_proj) {
        if (h->lsh_proj.size() != (size_t)P * h->dim)
            return fail(h, MHNSW_EDIM, "LSH projections have dimension %d, the index %d", (int)(h->lsh_proj.size() / P),
                        h->dim);
    } else {
        uint64_t st = h->lsh_seed;
        h->lsh_proj.resize((size_t)P * h->dim);
        for (float& v : h->lsh_proj) v = (float)(rng_next(&st) * 2.0 - 1.0);
    }
    if (h->lsh_dproj) (void)hipFree(h->lsh_dproj);
    if (h->lsh_pnorm) (void)hipFree(h->lsh_pnorm);
    h->lsh_dproj = h->lsh_pnorm = nullptr;
    h->lsh_rows = 0;
    h->lsh_stale = true;
    const size_t pbytes = (size_t)ppad * h->pitch * 4;
    if (hipMalloc(&h->lsh_dproj, pbytes) != hipSuccess || hipMalloc(&h->lsh_pnorm, (size_t)ppad * 4) != hipSuccess)
        return fail(h, MHNSW_ENOMEM, "device allocation of %zu bytes failed", pbytes);
    if (!h->lsh_work) {
        if (hipMalloc(&h->lsh_work, (size_t)LSH_WORK_MAX * sizeof(uint2)) != hipSuccess ||
            hipMalloc(&h->lsh_wcnt, 4) != hipSuccess || hipMalloc(&h->lsh_stat, 16) != hipSuccess)
            return fail(h, MHNSW_ENOMEM, "device allocation of the LSH worklist failed");
        HIPCHK(h, hipMemsetAsync(h->lsh_wcnt, 0, 4, h->stream));
        HIPCHK(h, hipMemsetAsync(h->lsh_stat, 0, 16, h->stream));
    }
    HIPCHK(h, hipMemsetAsync(h->lsh_dproj, 0, pbytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->lsh_pnorm, 0, (size_t)ppad * 4, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(h->lsh_dproj, (size_t)h->pitch * 4, h->lsh_proj.data(), (size_t)h->dim * 4,
                               (size_t)h->dim * 4, (size_t)P, hipMemcpyHostToDevice, h->stream));
    LCHK(h, launch_norms(h->lsh_dproj, 0, P, h->pitch, h->lpr, h->vpl, h->lsh_pnorm, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->lsh_pdim = h->dim;
    return 0;
}

// codes [capn * T], the hashed prefix kept across a reallocation
static int lsh_codes_fit(mhnsw_index* h, hipStream_t s) {
    const size_t need = (size_t)std::max<int64_t>(h->capn, 1) * h->lsh_T;
    if (h->lsh_codes.n >= need) return 0;
    uint32_t* np = nullptr;
    if (hipMalloc(&np, need * 4) != hipSuccess) return fail(h, MHNSW_ENOMEM, "device allocation of %zu bytes failed", need * 4);
    const size_t keep = std::min((size_t)h->lsh_rows * h->lsh_T, h->lsh_codes.n);
    if (h->lsh_codes.p && keep) HIPCHK(h, hipMemcpyAsync(np, h->lsh_codes.p, keep * 4, hipMemcpyDeviceToDevice, s));
    if (h->lsh_codes.p) {
        HIPCHK(h, hipStreamSynchronize(s));
        (void)hipFree(h->lsh_codes.p);
    }
    h->lsh_codes.p = np;
    h->lsh_codes.n = need;
    return 0;
}

// positions [r0, r1) of X (rows, a row list, or padded queries) -> codes, in launches of 65,536
// rows so that the worklist's fixed capacity is per launch
int lsh_hash_rows(mhnsw_index* h, const float* X, const float* xnorm, const uint32_t* d_ids, int64_t r0, int64_t r1,
                  uint32_t* codes, hipStream_t s) {
    LshHashArgs a;
    a.X = X;
    a.xnorm = xnorm;
    a.ids = d_ids;
    a.pitch = h->pitch;
    a.P = h->lsh_dproj;
    a.pnorm = h->lsh_pnorm;
    a.T = h->lsh_T;
    a.b = h->lsh_b;
    lsh_margin(h->dim, a.margin, a.abs_rel, a.abs_min);
    a.codes = codes;
    a.work = h->lsh_work;
    a.work_cap = std::min(h->lsh_work_cap, LSH_WORK_MAX);
    a.work_cnt = h->lsh_wcnt;
    a.stat = h->lsh_stat;
    for (int64_t c0 = r0; c0 < r1; c0 += 65536) {
        a.r0 = c0;
        a.r1 = std::min(c0 + 65536, r1);
        LCHK(h, launch_lsh_hash(a, h->lpr, h->vpl, s));
    }
    return 0;
}

int lsh_note_rows(mhnsw_index* h, int64_t r0, int64_t r1) {
    if (!h->lsh_T || h->dim <= 0 || r1 <= r0) return 0;
    int r;
    if ((r = lsh_prepare(h))) return r;
    h->lsh_stale = true;
    if (r0 > h->lsh_rows) return 0;  // the rows below are not hashed yet: the next search hashes [lsh_rows, n)
    if ((r = lsh_codes_fit(h, h->stream))) return r;
    if ((r = lsh_hash_rows(h, h->vecs, h->norms, nullptr, r0, r1, h->lsh_codes.p, h->stream))) return r;
    h->lsh_rows = std::max(h->lsh_rows, r1);
    return 0;
}

int lsh_note_ids(mhnsw_index* h, const uint32_t* d_ids, int64_t m, hipStream_t s) {
    if (!h->lsh_T || h->dim <= 0 || m <= 0) return 0;
    h->lsh_stale = true;
    if (!h->lsh_dproj || h->lsh_pdim != h->dim || h->lsh_codes.n < (size_t)h->capn * h->lsh_T) {
        h->lsh_rows = 0;  // nothing current to patch: the next search hashes every row
        return 0;
    }
    return lsh_hash_rows(h, h->vecs, h->norms, d_ids, 0, m, h->lsh_codes.p, s);
}

void lsh_note_all(mhnsw_index* h) {
    h->lsh_rows = 0;
    h->lsh_stale = true;
}

int lsh_sync(mhnsw_index* h, hipStream_t s) {
    std::lock_guard<std::mutex> lk(h->lsh_mu);
    if (!h->lsh_T) return fail(h, MHNSW_EINVAL, "LSH index is not enabled (mhnsw_lsh_enable)");
    if (h->dim <= 0 || h->n <= 0) return 0;
    int r;
    if ((r = lsh_prepare(h))) return r;
    if (s != h->stream) {  // rows and codes written on the handle's stream
        HIPCHK(h, hipEventRecord(h->meta_ev, h->stream));
        HIPCHK(h, hipStreamWaitEvent(s, h->meta_ev, 0));
    }
    h->lsh_rows = std::min(h->lsh_rows, h->n);
    if (h->lsh_rows < h->n) {
        if ((r = lsh_codes_fit(h, s))) return r;
        if ((r = lsh_hash_rows(h, h->vecs, h->norms, nullptr, h->lsh_rows, h->n, h->lsh_codes.p, s))) return r;
        h->lsh_rows = h->n;
        h->lsh_stale = true;
    }
    if (!h->lsh_stale && h->lsh_tab_n == h->n) return 0;
    const int64_t n = h->n;
    const int T = h->lsh_T;
    size_t tb = 0;
    if (lsh_sort_temp_bytes(n, &tb)) return fail(h, MHNSW_EDEVICE, "radix sort sizing failed");
    if ((r = ensure_buf(h, h->lsh_scode, (size_t)T * n)) || (r = ensure_buf(h, h->lsh_sid, (size_t)T * n)) ||
        (r = ensure_buf(h, h->lsh_key, (size_t)n)) || (r = ensure_buf(h, h->lsh_val, (size_t)n)) ||
        (r = ensure_buf(h, h->lsh_tmp, std::max<size_t>(tb, 16))))
        return r;
    if (!h->lev0) {
        HIPCHK(h, hipEventCreate(&h->lev0));
        HIPCHK(h, hipEventCreate(&h->lev1));
    }
    HIPCHK(h, hipEventRecord(h->lev0, s));
    for (int t = 0; t < T; ++t)
        LCHK(h, launch_lsh_table(h->lsh_codes.p, T, t, h->lsh_b, n, h->lsh_key.p, h->lsh_val.p, h->lsh_scode.p,
                                 h->lsh_sid.p, h->lsh_tmp.p, h->lsh_tmp.n, s));
    HIPCHK(h, hipEventRecord(h->lev1, s));
    h->have_lsh_rebuild = true;
    h->lsh_tab_n = n;
    h->lsh_stale = false;
    return 0;
}

}  // namespace mhh

extern "C" {

int mhnsw_lsh_enable(mhnsw_index* h, int tables, int bits, uint64_t seed, const float* projections, int dim) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    if (tables <= 0) tables = 4;  // lsh.go:38-45
    if (bits <= 0) bits = 8;
    if (tables > 32) return fail(h, MHNSW_EINVAL, "LSH tables must be at most 32, got %d", tables);
    if (bits > 32) return fail(h, MHNSW_EINVAL, "LSH bits must be at most 32, got %d", bits);
    if (tables * bits > LSH_MAX_P)
        return fail(h, MHNSW_EINVAL, "LSH tables x bits must be at most %d, got %d", LSH_MAX_P, tables * bits);
    if (projections) {
        if (dim <= 0) return fail(h, MHNSW_EDIM, "LSH projections need a dimension, got %d", dim);
        if (h->dim > 0 && dim != h->dim) return fail(h, MHNSW_EDIM, "embedding dimension mismatch: %d != %d", h->dim, dim);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->lsh_T = tables;
    h->lsh_b = bits;
    h->lsh_seed = seed;
    h->lsh_user_proj = projections != nullptr;
    if (projections)
        h->lsh_proj.assign(projections, projections + (size_t)tables * bits * dim);
    else
        h->lsh_proj.clear();
    if (h->lsh_dproj) (void)hipFree(h->lsh_dproj);
    if (h->lsh_pnorm) (void)hipFree(h->lsh_pnorm);
    h->lsh_dproj = h->lsh_pnorm = nullptr;
    if (h->lsh_codes.p) (void)hipFree(h->lsh_codes.p);  // (its row stride is T)
    h->lsh_codes.p = nullptr;
    h->lsh_codes.n = 0;
    h->lsh_pdim = 0;
    if (h->lsh_stat) HIPCHK(h, hipMemset(h->lsh_stat, 0, 16));
    lsh_note_all(h);
    int r;
    if (h->dim > 0 && h->n > 0) {  // a handle that already holds rows: all of them now
        if ((r = lsh_note_rows(h, 0, h->n))) return r;
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

int mhnsw_lsh_hash(mhnsw_index* h, const float* vecs, int64_t n, int dim, uint32_t* out_codes) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    if (!h->lsh_T) return fail(h, MHNSW_EINVAL, "LSH index is not enabled (mhnsw_lsh_enable)");
    if (n <= 0) return 0;
    if (!vecs || !out_codes) return fail(h, MHNSW_EINVAL, "vecs and out_codes must be non-NULL");
    if (h->dim <= 0) return fail(h, MHNSW_EINVAL, "LSH projections wait for the first Add's dimension");
    if (dim != h->dim) return fail(h, MHNSW_EDIM, "embedding dimension mismatch: %d != %d", h->dim, dim);
    int r;
    if ((r = lsh_prepare(h))) return r;
    hipStream_t s = h->stream;
    if ((r = ensure_buf(h, h->tmp, (size_t)n * dim)) || (r = ensure_buf(h, h->qpad, (size_t)n * h->pitch)) ||
        (r = ensure_buf(h, h->qnorm, (size_t)n)) || (r = ensure_buf(h, h->lsh_qcodes, (size_t)n * h->lsh_T)))
        return r;
    HIPCHK(h, hipMemcpyAsync(h->tmp.p, vecs, (size_t)n * dim * 4, hipMemcpyHostToDevice, s));
    LCHK(h, launch_pad_rows(h->tmp.p, n, dim, h->qpad.p, h->pitch, s));
    LCHK(h, launch_norms(h->qpad.p, 0, n, h->pitch, h->lpr, h->vpl, h->qnorm.p, s));
    if ((r = lsh_hash_rows(h, h->qpad.p, h->qnorm.p, nullptr, 0, n, h->lsh_qcodes.p, s))) return r;
    HIPCHK(h, hipMemcpyAsync(out_codes, h->lsh_qcodes.p, (size_t)n * h->lsh_T * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}

int mhnsw_lsh_codes(mhnsw_index* h, uint32_t* out) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    if (int r = lsh_sync(h, h->stream)) return r;
    if (h->n <= 0 || h->dim <= 0) return 0;
    if (!out) return fail(h, MHNSW_EINVAL, "out must be non-NULL");
    HIPCHK(h, hipMemcpyAsync(out, h->lsh_codes.p, (size_t)h->n * h->lsh_T * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int mhnsw_lsh_projections(mhnsw_index* h, float* out) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (!h->lsh_T) return fail(h, MHNSW_EINVAL, "LSH index is not enabled (mhnsw_lsh_enable)");
    if (int r = lsh_prepare(h)) return r;
    if (h->lsh_proj.empty()) return fail(h, MHNSW_EINVAL, "LSH projections wait for the first Add's dimension");
    if (!out) return fail(h, MHNSW_EINVAL, "out must be non-NULL");
    std::memcpy(out, h->lsh_proj.data(), h->lsh_proj.size() * 4);
    return 0;
}

int mhnsw_search_lsh(mhnsw_index* h, const float* queries, int64_t B, int dim, int k, int64_t* out_keys, float* out_dist,
                     int32_t* out_n, int32_t* out_ncand) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    return search_lsh_impl(h, queries, false, B, dim, k, out_keys, out_dist, out_n, out_ncand, h->stream, false);
}

int mhnsw_search_lsh_device(mhnsw_index* h, const float* d_queries, int64_t B, int dim, int k, int64_t* d_keys,
                            float* d_dist, int32_t* d_n, int32_t* d_ncand, void* stream) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    return search_lsh_impl(h, d_queries, true, B, dim, k, d_keys, d_dist, d_n, d_ncand, (hipStream_t)stream, true);
}

}  // extern "C"
