// part_host.cpp -- host side of the partitions (hnsw-extensions/hybrid/partitioner.go; kernels:
// part.hip; DESIGN.md §6 "Partitions"): the configuration and centroids, the rows' stored
// partitions kept through the mutations, the lazily rebuilt id lists, the centroid update,
// Rebalance and Train, and the entry points that are not searches.  The search itself is one
// more SearchCall of search_host.cpp (search_part).
#include "index.hpp"

using namespace mhh;

namespace mhh {

static int part_ppad(const mhnsw_index* h) { return (h->part_P + PART_PAD_UNIT - 1) / PART_PAD_UNIT * PART_PAD_UNIT; }

// When does the MFMA's dot decide the canonical argmin?  u = 2^-24, d the dimension, gamma_d =
// d u / (1 - d u) <= 1.001 d u for d <= 4096.  As in lsh_margin the instruction's dot s_m is
// given three roundings per term: |s_m - x.c| <= 3 gamma_d |x| |c|.  The stored norms are
// nx = fl(sqrt(canonical sum of squares)): nx^2 = |x|^2 (1 + e), |e| <= gamma_{d+1} + 2 u.
//
// Euclidean.  The canonical distance is fl(sqrt(S_c)), S_c the canonical f32 sum of
// fl(x_i - c_i)^2: every term is non-negative, so S_c = S (1 + t), |t| <= gamma_{d+2}, S the
// true squared distance (a term below 2^-126 may be flushed: at most d 2^-126 in all).  The
// kernel forms A = nx^2 + nc^2 - 2 s_m in f32:
//   |A - S| <= (gamma_{d+1} + 2 u)(nx^2 + nc^2)   the two norms
//            + 6 gamma_d |x| |c|                  the dot; 2 |x| |c| <= |x|^2 + |c|^2
//            + 8 u (nx^2 + nc^2)                  four roundings of values <= 2 (nx^2 + nc^2)
//           <= (4.1 d + 12) u (nx^2 + nc^2).
// e_rel = (4.2 d + 40) u, and e_abs = d 2^-120 for the flushed terms.  With E = e_rel (nx^2 +
// nc^2) + e_abs the canonical sum lies in [(A - E)(1 - e_mul), (A + E)(1 + e_mul)], e_mul =
// (1.01 d + 40) u >= gamma_{d+2} + 8 u + the roundings of the bounds themselves.  The 8 u: the
// test "upper end of the best < lower end of every other" then gives S_c(best) (1 + 8 u) <
// S_c(other), so the correctly rounded square roots differ (sqrt(1 + 8 u) > (1 + u) / (1 - u)):
// the canonical f32 distance of the best is strictly below every other.
//
// Cosine.  The canonical distance is fl(1 - fl(s_c / fl(nx nc))) with |s_c - x.c| <= gamma_d
// |x| |c| and fl(nx nc) = |x| |c| (1 + e), |e| <= (d + 5) u: the quotient is within (2 d + 6)
// 1.01 u of the true cosine (|cos| <= 1), the kernel's s_m / (nx nc) within (4 d + 6) 1.01 u,
// so the two differ by at most R = (6 d + 12) 1.02 u.  Two f32 values 1 - q that differ by more
// than 2^-22 round to different floats in [0, 2].  With e_abs = (6.2 d + 60) u >= R + 2^-23 +
// the roundings of A and its bounds, "upper end of the best < lower end of the other" puts the
// canonical quotients more than 2^-22 apart.  A product nx nc below den_min = 2^-60 (a zero
// vector among them), and any NaN or infinite value, is never trusted.
//
// Everything here errs wide: an uncertain row costs one canonical pass, a wrong certain row
// breaks parity.
static void part_radius(int d, int metric, PartAssignArgs& a) {
    const double u = 5.9604644775390625e-08;
    if (metric == EUCLIDEAN) {
        a.e_rel = (float)((4.2 * d + 40) * u);
        a.e_mul = (float)((1.01 * d + 40) * u);
        a.e_abs = (float)((double)d * 7.52316384526264e-37);  // d 2^-120
        a.den_min = 0.f;
    } else {
        a.e_rel = a.e_mul = 0.f;
        a.e_abs = (float)((6.2 * d + 60) * u);
        a.den_min = 8.673617379884035e-19f;  // 2^-60
    }
}

void part_free(mhnsw_index* h) {
    auto F = [](auto*& p) {
        if (p) (void)hipFree(p);
        p = nullptr;
    };
    F(h->part_dcent);
    F(h->part_cnorm);
    F(h->part_work);
    F(h->part_wcnt);
    F(h->part_stat);
    F(h->part_of.p);
    F(h->part_off.p);
    F(h->part_probe.p);
    F(h->part_ncand.p);
    F(h->part_cbase.p);
    F(h->part_out.p);
    F(h->part_key.p);
    F(h->part_val.p);
    F(h->part_skey.p);
    F(h->part_sid.p);
    F(h->part_tmp.p);
    F(h->part_partial.p);
    h->part_of.n = h->part_off.n = h->part_probe.n = h->part_ncand.n = h->part_cbase.n = h->part_out.n = 0;
    h->part_key.n = h->part_val.n = h->part_skey.n = h->part_sid.n = h->part_tmp.n = h->part_partial.n = 0;
    F(h->ps_seed_d.p);
    F(h->ps_thr.p);
    F(h->ps_sscore.p);
    F(h->ps_seed_i.p);
    F(h->ps_pairs.p);
    F(h->ps_scnt.p);
    F(h->ps_surv.p);
    F(h->ps_tab.p);
    F(h->ps_tmp.p);
    F(h->ps_stat.p);
    h->ps_seed_d.n = h->ps_thr.n = h->ps_seed_i.n = h->ps_pairs.n = h->ps_scnt.n = h->ps_surv.n = 0;
    h->ps_tab.n = h->ps_tmp.n = h->ps_stat.n = h->ps_sscore.n = 0;
    h->have_part_scan_timing = false;
    for (hipEvent_t& e : h->pev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    for (hipEvent_t& e : h->psev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

// The centroids on the device for the handle's dimension.  Generated ones are drawn now
// (partitioner.go:58-78: one SplitMix64 stream from the seed, element (float)(u * 2 - 1), the
// row scaled by (float)(1 / (double)sum) with sum the sequential f32 sum of squares -- the
// reference's own "normalisation", kept because it changes Euclidean assignments; Go's
// math/rand stream is not reproduced).  A caller's must have that dimension.
static int part_prepare(mhnsw_index* h) {
    if (!h->part_P || h->dim <= 0) return 0;
    const int P = h->part_P, ppad = part_ppad(h);
    if (h->part_dcent && h->part_cdim == h->dim) return 0;
    if (h->part_user) {
        if (h->part_init.size() != (size_t)P * h->dim)
            return fail(h, MHNSW_EDIM, "partition centroids have dimension %d, the index %d",
                        (int)(h->part_init.size() / P), h->dim);
    } else {
        uint64_t st = h->part_seed;
        h->part_init.resize((size_t)P * h->dim);
        for (int p = 0; p < P; ++p) {
            float* c = &h->part_init[(size_t)p * h->dim];
            float sum = 0.f;
            for (int j = 0; j < h->dim; ++j) {
                c[j] = (float)(rng_next(&st) * 2.0 - 1.0);
                sum += c[j] * c[j];
            }
            const float norm = (float)(1.0 / (double)sum);
            for (int j = 0; j < h->dim; ++j) c[j] *= norm;
        }
    }
    if (h->part_dcent) (void)hipFree(h->part_dcent);
    if (h->part_cnorm) (void)hipFree(h->part_cnorm);
    h->part_dcent = h->part_cnorm = nullptr;
    h->part_rows = 0;
    h->part_stale = true;
    const size_t cbytes = (size_t)ppad * h->pitch * 4;
    if (hipMalloc(&h->part_dcent, cbytes) != hipSuccess || hipMalloc(&h->part_cnorm, (size_t)ppad * 4) != hipSuccess)
        return fail(h, MHNSW_ENOMEM, "device allocation of %zu bytes failed", cbytes);
    if (!h->part_work) {
        if (hipMalloc(&h->part_work, (size_t)PART_WORK_MAX * 4) != hipSuccess || hipMalloc(&h->part_wcnt, 4) != hipSuccess ||
            hipMalloc(&h->part_stat, 32) != hipSuccess)
            return fail(h, MHNSW_ENOMEM, "device allocation of the partition worklist failed");
        HIPCHK(h, hipMemsetAsync(h->part_wcnt, 0, 4, h->stream));
        HIPCHK(h, hipMemsetAsync(h->part_stat, 0, 32, h->stream));
    }
    HIPCHK(h, hipMemsetAsync(h->part_dcent, 0, cbytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->part_cnorm, 0, (size_t)ppad * 4, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(h->part_dcent, (size_t)h->pitch * 4, h->part_init.data(), (size_t)h->dim * 4,
                               (size_t)h->dim * 4, (size_t)P, hipMemcpyHostToDevice, h->stream));
    LCHK(h, launch_norms(h->part_dcent, 0, P, h->pitch, h->lpr, h->vpl, h->part_cnorm, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->part_cdim = h->dim;
    return 0;
}

// part_of [capn], the assigned prefix kept across a reallocation
static int part_fit(mhnsw_index* h, hipStream_t s) {
    const size_t need = (size_t)std::max<int64_t>(h->capn, 1);
    if (h->part_of.n >= need) return 0;
    int32_t* np = nullptr;
    if (hipMalloc(&np, need * 4) != hipSuccess) return fail(h, MHNSW_ENOMEM, "device allocation of %zu bytes failed", need * 4);
    HIPCHK(h, hipMemsetAsync(np, 0xFF, need * 4, s));
    const size_t keep = std::min((size_t)h->part_rows, h->part_of.n);
    if (h->part_of.p && keep) HIPCHK(h, hipMemcpyAsync(np, h->part_of.p, keep * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (h->part_of.p) (void)hipFree(h->part_of.p);
    h->part_of.p = np;
    h->part_of.n = need;
    return 0;
}

// positions [r0, r1) of X (rows, a row list, or padded vectors) -> part, in launches of 65,536
// rows so that the worklist's fixed capacity is per launch
static int part_assign_rows(mhnsw_index* h, const float* X, const float* xnorm, const uint32_t* d_ids, int64_t r0,
                            int64_t r1, int32_t* part, unsigned long long* moved, hipStream_t s) {
    PartAssignArgs a;
    a.X = X;
    a.xnorm = xnorm;
    a.ids = d_ids;
    a.pitch = h->pitch;
    a.metric = h->metric;
    a.Cn = h->part_dcent;
    a.cnorm = h->part_cnorm;
    a.P = h->part_P;
    part_radius(h->dim, h->metric, a);
    a.part = part;
    a.work = h->part_work;
    a.work_cap = std::min(h->part_work_cap, PART_WORK_MAX);
    a.work_cnt = h->part_wcnt;
    a.force = h->part_force_canon;
    a.dead = moved && h->any_dead ? h->dead : nullptr;
    a.stat = h->part_stat;
    a.moved = moved;
    for (int64_t c0 = r0; c0 < r1; c0 += 65536) {
        a.r0 = c0;
        a.r1 = std::min(c0 + 65536, r1);
        LCHK(h, launch_part_assign(a, h->lpr, h->vpl, s));
    }
    return 0;
}

void part_note_added(mhnsw_index* h) {
    if (h->part_P) h->part_stale = true;
}

int part_note_range(mhnsw_index* h, int64_t r0, int64_t r1) {
    if (!h->part_P || h->dim <= 0 || r1 <= r0) return 0;
    h->part_stale = true;
    if (!h->part_dcent || h->part_cdim != h->dim || r1 > h->part_rows) return 0;  // (pending rows are assigned later anyway)
    int r;
    if ((r = part_fit(h, h->stream))) return r;
    return part_assign_rows(h, h->vecs, h->norms, nullptr, r0, r1, h->part_of.p, nullptr, h->stream);
}

int part_note_ids(mhnsw_index* h, const uint32_t* d_ids, int64_t m, hipStream_t s) {
    if (!h->part_P || h->dim <= 0 || m <= 0) return 0;
    h->part_stale = true;
    if (!h->part_dcent || h->part_cdim != h->dim || h->part_rows <= 0) return 0;  // every row is pending
    int r;
    if ((r = part_fit(h, s))) return r;
    // (a listed row above part_rows is written too: the flush gives it the same value)
    return part_assign_rows(h, h->vecs, h->norms, d_ids, 0, m, h->part_of.p, nullptr, s);
}

void part_note_all(mhnsw_index* h) {
    h->part_rows = 0;
    h->part_stale = true;
}

void part_compacted(mhnsw_index* h, int64_t live) {
    if (!h->part_P) return;
    h->part_rows = h->part_rows > 0 ? live : 0;
    h->part_stale = true;
}

int part_flush(mhnsw_index* h, hipStream_t s) {
    if (!h->part_P || h->dim <= 0 || h->n <= 0) return 0;
    int r;
    if ((r = part_prepare(h)) || (r = part_fit(h, s))) return r;
    h->part_rows = std::min(h->part_rows, h->n);
    if (h->part_rows < h->n) {
        if ((r = part_assign_rows(h, h->vecs, h->norms, nullptr, h->part_rows, h->n, h->part_of.p, nullptr, s))) return r;
        h->part_rows = h->n;
        h->part_stale = true;
    }
    return 0;
}

int part_sync(mhnsw_index* h, hipStream_t s, bool strict) {
    std::lock_guard<std::mutex> lk(h->part_mu);
    if (!h->part_P) return fail(h, MHNSW_EINVAL, "partitions are not enabled (mhnsw_part_enable)");
    if (h->dim <= 0 || h->n <= 0) return 0;
    int r;
    if ((r = part_prepare(h))) return r;
    if (s != h->stream) {  // rows and partitions written on the handle's stream
        HIPCHK(h, hipEventRecord(h->meta_ev, h->stream));
        HIPCHK(h, hipStreamWaitEvent(s, h->meta_ev, 0));
    }
    if ((r = part_flush(h, s))) return r;
    if (!h->part_stale && h->part_list_n == h->n && (!strict || h->part_list_epoch == h->mut_epoch)) return 0;
    const int64_t n = h->n;
    size_t tb = 0;
    if (part_sort_temp_bytes(n, &tb)) return fail(h, MHNSW_EDEVICE, "radix sort sizing failed");
    if ((r = ensure_buf(h, h->part_skey, (size_t)n)) || (r = ensure_buf(h, h->part_sid, (size_t)n)) ||
        (r = ensure_buf(h, h->part_key, (size_t)n)) || (r = ensure_buf(h, h->part_val, (size_t)n)) ||
        (r = ensure_buf(h, h->part_off, (size_t)PART_MAX_P + 2)) || (r = ensure_buf(h, h->part_tmp, std::max<size_t>(tb, 16))))
        return r;
    if (!h->pev[0])
        for (hipEvent_t& e : h->pev) HIPCHK(h, hipEventCreate(&e));
    HIPCHK(h, hipEventRecord(h->pev[0], s));
    LCHK(h, launch_part_lists(h->part_of.p, h->any_dead ? h->dead : nullptr, h->part_P, n, h->part_key.p, h->part_val.p,
                              h->part_skey.p, h->part_sid.p, h->part_off.p, h->part_tmp.p, h->part_tmp.n, s));
    HIPCHK(h, hipEventRecord(h->pev[1], s));
    h->have_part_rebuild = true;
    h->part_list_n = n;
    h->part_list_epoch = h->mut_epoch;
    h->part_stale = false;
    return 0;
}

// partitioner.go:163-206 on the handle's stream; the lists hold live rows only (strict sync)
static int part_update_centroids(mhnsw_index* h) {
    int r;
    if ((r = part_sync(h, h->stream, true))) return r;
    if (h->dim <= 0 || h->n <= 0) return 0;
    const int P = h->part_P;
    std::vector<int32_t> off((size_t)P + 2), cbase((size_t)P + 1);
    HIPCHK(h, hipMemcpyAsync(off.data(), h->part_off.p, off.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int chunks = 0;
    for (int p = 0; p < P; ++p) {
        cbase[p] = chunks;
        chunks += (off[p + 1] - off[p] + PART_CHUNK - 1) / PART_CHUNK;
    }
    cbase[P] = chunks;
    if ((r = ensure_buf(h, h->part_cbase, (size_t)PART_MAX_P + 1)) ||
        (r = ensure_buf(h, h->part_partial, (size_t)std::max(chunks, 1) * h->pitch)))
        return r;
    HIPCHK(h, hipMemcpyAsync(h->part_cbase.p, cbase.data(), cbase.size() * 4, hipMemcpyHostToDevice, h->stream));
    LCHK(h, launch_part_update(h->vecs, h->pitch, h->part_sid.p, h->part_off.p, h->part_cbase.p, P, chunks,
                               h->part_partial.p, h->part_dcent, h->stream));
    LCHK(h, launch_norms(h->part_dcent, 0, P, h->pitch, h->lpr, h->vpl, h->part_cnorm, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (cbase is read from this frame)
    return 0;
}

// partitioner.go:210-222: every row against the current centroids; the live rows that moved
static int part_rebalance(mhnsw_index* h, int64_t* moved) {
    *moved = 0;
    int r;
    if ((r = part_flush(h, h->stream))) return r;
    if (h->dim <= 0 || h->n <= 0) return 0;
    HIPCHK(h, hipMemsetAsync(h->part_stat + 2, 0, 8, h->stream));
    if ((r = part_assign_rows(h, h->vecs, h->norms, nullptr, 0, h->n, h->part_of.p, h->part_stat + 2, h->stream))) return r;
    unsigned long long mv = 0;
    HIPCHK(h, hipMemcpyAsync(&mv, h->part_stat + 2, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->part_stale = true;
    *moved = (int64_t)mv;
    return 0;
}

// ---- the partition-major scan (part_scan.hip; DESIGN.md §6 "Partition scan") ----
// Option "part_scan": from part_scan_min_b queries and two probes on -- one probe at
// part_scan_seed = 0, where no probe is kept for a seed walk.  (The items' count is a 32-bit
// prefix: a shape whose bound on it does not fit keeps the walk.)
bool part_scan_wanted(const mhnsw_index* h, int64_t B, int nprobe) {
    if (!h->part_scan || nprobe < (h->part_scan_seed == 0 ? 1 : 2) || B < h->part_scan_min_b) return false;
    const int64_t qt = B * nprobe / PSCAN_BM + h->part_P, rt = h->part_list_n / PSCAN_BN + 1;
    return B * nprobe < ((int64_t)1 << 31) && qt * rt < ((int64_t)1 << 31);
}

// The ranking of a partition search whose probe order is written (a: launch_part_search's
// arguments), all on s from the handle's buffers, no host synchronisation.  The scores run on
// the exact path's fp16 row plane (brought up to date here as exact_run does) at precision 3,
// whatever exact_precision the handle keeps.
int part_scan_search(mhnsw_index* h, const PartSearchArgs& a, bool timing, hipStream_t s) {
    int r;
    const int64_t B = a.B;
    const int nprobe = a.nprobe, P = h->part_P;
    const int seed = std::min(h->part_scan_seed, nprobe - 1), room = h->part_scan_room;
    // (no list is longer than the rows the lists hold: the score rows need no more)
    const int seed_room = (int)std::min<int64_t>(h->part_scan_seed_room, std::max<int64_t>(a.n, 1));
    const int64_t pairs = B * (nprobe - seed);
    size_t tb = 0, tb0 = 0;
    if (part_scan_temp_bytes(pairs, &tb) || (seed == 0 && part_scan_temp_bytes(B, &tb0)))
        return fail(h, MHNSW_EDEVICE, "radix sort sizing failed");
    tb = std::max(tb, tb0);
    const int64_t plane = h->capn * h->pitch;
    if (h->xsplit.n < (size_t)plane * 2 || h->xsplit_plane != plane || h->xsplit_kind != 2) {
        if ((r = ensure_buf(h, h->xsplit, (size_t)plane * 2))) return r;
        h->xsplit_rows = 0;
        h->xsplit_plane = plane;
        h->xsplit_kind = 2;
    }
    if ((r = ensure_buf(h, h->xinv, (size_t)h->capn)) || (r = ensure_buf(h, h->xerr, 1)) || (r = ensure_buf(h, h->qerr, 1)) ||
        (r = ensure_buf(h, h->xmaxn, 1)) || (r = ensure_buf(h, h->qnorm, (size_t)B)) || (r = ensure_buf(h, h->qinv, (size_t)B)) ||
        (r = ensure_buf(h, h->qsplit, (size_t)B * h->pitch)) || (r = ensure_buf(h, h->ps_seed_d, (size_t)B * a.k)) ||
        (r = ensure_buf(h, h->ps_seed_i, (size_t)B * a.k)) || (r = ensure_buf(h, h->ps_thr, (size_t)B)) ||
        (r = ensure_buf(h, h->ps_pairs, (size_t)4 * pairs)) || (r = ensure_buf(h, h->ps_tab, (size_t)3 * PART_MAX_P + 8)) ||
        (r = ensure_buf(h, h->ps_scnt, (size_t)B)) || (r = ensure_buf(h, h->ps_surv, (size_t)B * room)) ||
        (r = ensure_buf(h, h->ps_stat, 2)) || (r = ensure_buf(h, h->ps_tmp, std::max<size_t>(tb, 16))) ||
        (seed == 0 && (r = ensure_buf(h, h->ps_sscore, (size_t)B * seed_room))))
        return r;
    if (!h->psev[0])
        for (hipEvent_t& e : h->psev) HIPCHK(h, hipEventCreate(&e));
    if (h->xsplit_rows < h->n) {
        if (h->xsplit_rows == 0) HIPCHK(h, hipMemsetAsync(h->xerr.p, 0, sizeof(float), s));
        LCHK(h, launch_split_h16(h->vecs, h->xsplit_rows, h->n, h->pitch, h->capn, h->xsplit.p, nullptr, h->xinv.p,
                                 h->xerr.p, s));
        h->xsplit_rows = h->n;
    }
    LCHK(h, launch_norms(h->qpad.p, 0, B, h->pitch, h->lpr, h->vpl, h->qnorm.p, s));
    HIPCHK(h, hipMemsetAsync(h->qerr.p, 0, sizeof(float), s));
    LCHK(h, launch_split_h16(h->qpad.p, 0, B, h->pitch, B, h->qsplit.p, nullptr, h->qinv.p, h->qerr.p, s));
    if (h->metric == EUCLIDEAN) {
        HIPCHK(h, hipMemsetAsync(h->xmaxn.p, 0, sizeof(float), s));
        LCHK(h, launch_max_norm(h->norms, h->n, h->xmaxn.p, s));
    }
    HIPCHK(h, hipMemsetAsync(h->ps_stat.p, 0, 16, s));
    PartScanArgs p{};
    p.s = a;
    p.P = P;
    p.seed = seed;
    p.room = room;
    p.pitch = h->pitch;
    p.qnorm = h->qnorm.p;
    p.qinv = h->qinv.p;
    p.Qh = h->qsplit.p;
    p.ldQ = B;
    p.Xh = h->xsplit.p;
    p.ldX = h->capn;
    p.xinv = h->xinv.p;
    exact_cert_consts(h, 1.0, 0.0, p.c);  // (fp16 1-product: both roundings are the measured xerr / qerr)
    p.c.xmax = h->xmaxn.p;
    p.c.xerr = h->xerr.p;
    p.c.qerr = h->qerr.p;
    p.seed_d = h->ps_seed_d.p;
    p.seed_i = h->ps_seed_i.p;
    p.thr = h->ps_thr.p;
    p.pkey = h->ps_pairs.p;
    p.pval = p.pkey + pairs;
    p.skey = p.pval + pairs;
    p.sval = p.skey + pairs;
    p.poff = h->ps_tab.p;
    p.ibase = p.poff + PART_MAX_P + 2;
    p.live = p.ibase + PART_MAX_P + 1;
    p.scnt = h->ps_scnt.p;
    p.surv = h->ps_surv.p;
    p.stat = h->ps_stat.p;
    p.temp = h->ps_tmp.p;
    p.temp_bytes = h->ps_tmp.n;
    if (seed == 0) {  // the radius from the scan: the nearest lists scored, k rows of each evaluated
        p.seed_room = seed_room;
        p.sscore = h->ps_sscore.p;
        if (timing) HIPCHK(h, hipEventRecord(h->psev[0], s));
        PartScanArgs p0 = p;
        p0.seed_pass = 1;
        LCHK(h, launch_part_scan_invert(p0, s));
        LCHK(h, launch_part_scan_seed_tiles(p0, s));
        LCHK(h, launch_part_scan_pick(p, h->lpr, h->vpl, s));
    } else {
        LCHK(h, launch_part_scan_seed(p, h->lpr, h->vpl, s));
        if (timing) HIPCHK(h, hipEventRecord(h->psev[0], s));
    }
    LCHK(h, launch_part_scan_invert(p, s));
    LCHK(h, launch_part_scan_tiles(p, s));
    if (timing) HIPCHK(h, hipEventRecord(h->psev[1], s));
    LCHK(h, launch_part_scan_finish(p, h->lpr, h->vpl, s));
    h->part_scan_queries = B;
    h->have_part_scan_timing = timing;
    return 0;
}

static int part_enabled(mhnsw_index* h) {
    return h->part_P ? 0 : fail(h, MHNSW_EINVAL, "partitions are not enabled (mhnsw_part_enable)");
}

}  // namespace mhh

extern "C" {

int mhnsw_part_enable(mhnsw_index* h, int partitions, uint64_t seed, const float* centroids, int dim) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    if (partitions <= 0) partitions = 10;  // partitioner.go:32-34
    if (partitions > PART_MAX_P) return fail(h, MHNSW_EINVAL, "partitions must be at most %d, got %d", PART_MAX_P, partitions);
    if (centroids) {
        if (dim <= 0) return fail(h, MHNSW_EDIM, "partition centroids need a dimension, got %d", dim);
        if (h->dim > 0 && dim != h->dim) return fail(h, MHNSW_EDIM, "embedding dimension mismatch: %d != %d", h->dim, dim);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->part_P = partitions;
    h->part_seed = seed;
    h->part_user = centroids != nullptr;
    if (centroids)
        h->part_init.assign(centroids, centroids + (size_t)partitions * dim);
    else
        h->part_init.clear();
    if (h->part_dcent) (void)hipFree(h->part_dcent);
    if (h->part_cnorm) (void)hipFree(h->part_cnorm);
    h->part_dcent = h->part_cnorm = nullptr;
    h->part_cdim = 0;
    if (h->part_stat) HIPCHK(h, hipMemset(h->part_stat, 0, 32));
    part_note_all(h);
    if (h->dim > 0 && h->n > 0) {  // a handle that already holds rows: all of them now
        if (int r = part_flush(h, h->stream)) return r;
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

int mhnsw_part_assign(mhnsw_index* h, const float* vecs, int64_t n, int dim, int nprobe, int32_t* out_parts) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    int r;
    if ((r = part_enabled(h))) return r;
    if (nprobe < 1 || nprobe > std::min(h->part_P, PART_MAX_PROBE))
        return fail(h, MHNSW_EINVAL, "nprobe must be in [1, %d], got %d", std::min(h->part_P, PART_MAX_PROBE), nprobe);
    if (n <= 0) return 0;
    if (!vecs || !out_parts) return fail(h, MHNSW_EINVAL, "vecs and out_parts must be non-NULL");
    if (h->dim <= 0) return fail(h, MHNSW_EINVAL, "partition centroids wait for the first Add's dimension");
    if (dim != h->dim) return fail(h, MHNSW_EDIM, "embedding dimension mismatch: %d != %d", h->dim, dim);
    if ((r = part_prepare(h))) return r;
    hipStream_t s = h->stream;
    if ((r = ensure_buf(h, h->tmp, (size_t)n * dim)) || (r = ensure_buf(h, h->qpad, (size_t)n * h->pitch)) ||
        (r = ensure_buf(h, h->qnorm, (size_t)n)) || (r = ensure_buf(h, h->part_out, (size_t)n * nprobe)))
        return r;
    HIPCHK(h, hipMemcpyAsync(h->tmp.p, vecs, (size_t)n * dim * 4, hipMemcpyHostToDevice, s));
    LCHK(h, launch_pad_rows(h->tmp.p, n, dim, h->qpad.p, h->pitch, s));
    if (nprobe == 1) {
        LCHK(h, launch_norms(h->qpad.p, 0, n, h->pitch, h->lpr, h->vpl, h->qnorm.p, s));
        if ((r = part_assign_rows(h, h->qpad.p, h->qnorm.p, nullptr, 0, n, h->part_out.p, nullptr, s))) return r;
    } else {
        LCHK(h, launch_part_probe(h->qpad.p, n, h->pitch, h->metric, h->part_dcent, h->part_cnorm, h->part_P, nprobe,
                                  h->part_out.p, h->lpr, h->vpl, s));
    }
    HIPCHK(h, hipMemcpyAsync(out_parts, h->part_out.p, (size_t)n * nprobe * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}

int mhnsw_part_rows(mhnsw_index* h, int32_t* out) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    int r;
    if ((r = part_enabled(h)) || (r = part_flush(h, h->stream))) return r;
    if (h->n <= 0 || h->dim <= 0) return 0;
    if (!out) return fail(h, MHNSW_EINVAL, "out must be non-NULL");
    HIPCHK(h, hipMemcpyAsync(out, h->part_of.p, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < h->n; ++i)
        if (h->hdead[i]) out[i] = -1;
    return 0;
}

int mhnsw_part_centroids(mhnsw_index* h, float* out) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    int r;
    if ((r = part_enabled(h)) || (r = part_prepare(h))) return r;
    if (!h->part_dcent) return fail(h, MHNSW_EINVAL, "partition centroids wait for the first Add's dimension");
    if (!out) return fail(h, MHNSW_EINVAL, "out must be non-NULL");
    HIPCHK(h, hipMemcpy2DAsync(out, (size_t)h->dim * 4, h->part_dcent, (size_t)h->pitch * 4, (size_t)h->dim * 4,
                               (size_t)h->part_P, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int mhnsw_part_stats(mhnsw_index* h, int64_t* out) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    int r;
    if ((r = part_enabled(h)) || (r = part_flush(h, h->stream))) return r;
    if (!out) return fail(h, MHNSW_EINVAL, "out must be non-NULL");
    std::memset(out, 0, (size_t)h->part_P * 8);
    if (h->n <= 0 || h->dim <= 0) return 0;
    if ((r = ensure_buf(h, h->part_partial, (size_t)h->part_P))) return r;  // (8-byte counters)
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(h->part_partial.p);
    HIPCHK(h, hipMemsetAsync(cnt, 0, (size_t)h->part_P * 8, h->stream));
    LCHK(h, launch_part_stats(h->part_of.p, h->any_dead ? h->dead : nullptr, h->n, h->part_P, cnt, h->stream));
    HIPCHK(h, hipMemcpyAsync(out, cnt, (size_t)h->part_P * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int mhnsw_part_update_centroids(mhnsw_index* h) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    if (int r = part_enabled(h)) return r;
    return part_update_centroids(h);
}

int mhnsw_part_rebalance(mhnsw_index* h, int64_t* out_moved) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    if (int r = part_enabled(h)) return r;
    int64_t mv = 0;
    const int r = part_rebalance(h, &mv);
    if (out_moved) *out_moved = mv;
    return r;
}

int mhnsw_part_train(mhnsw_index* h, int iters, int64_t* out_moved) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (int r0 = drain(h)) return r0;
    int r;
    if ((r = part_enabled(h))) return r;
    if (out_moved) *out_moved = 0;
    if (iters <= 0 || h->dim <= 0 || h->n <= 0) return 0;
    if ((r = part_sync(h, h->stream, true))) return r;  // (creates the events)
    HIPCHK(h, hipEventRecord(h->pev[2], h->stream));
    int64_t mv = 0;
    for (int it = 0; it < iters; ++it) {
        if ((r = part_update_centroids(h)) || (r = part_rebalance(h, &mv))) return r;
        if (mv == 0) break;
    }
    HIPCHK(h, hipEventRecord(h->pev[3], h->stream));
    h->have_part_train = true;
    if (out_moved) *out_moved = mv;
    return 0;
}

int mhnsw_search_part(mhnsw_index* h, const float* queries, int64_t B, int dim, int k, int nprobe, int64_t* out_keys,
                      float* out_dist, int32_t* out_n, int32_t* out_ncand) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    return search_part_impl(h, queries, false, B, dim, k, nprobe, out_keys, out_dist, out_n, out_ncand, h->stream, false);
}

int mhnsw_search_part_device(mhnsw_index* h, const float* d_queries, int64_t B, int dim, int k, int nprobe,
                             int64_t* d_keys, float* d_dist, int32_t* d_n, int32_t* d_ncand, void* stream) {
    std::unique_lock<std::shared_mutex> lk(h->mu);
    return search_part_impl(h, d_queries, true, B, dim, k, nprobe, d_keys, d_dist, d_n, d_ncand, (hipStream_t)stream, true);
}

}  // extern "C"
