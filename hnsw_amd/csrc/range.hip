// range.hip -- range search (search_host.cpp range_search): every row within a per-query
// radius, as a ragged result.  Exact mode reuses the exact path's fp16 filter GEMM with the
// radius as the threshold; the kernels here are everything around it:
//
//  k_range_thr    : per query the score threshold t_q the filter GEMM keeps (the certificate's
//                   inequality read the other way: a row with canonical distance <= r scores
//                   <= t_q), and which path the query takes (fused / sweep / no hit possible).
//  k_range_refine : 4 waves per query walk its sub-buckets, evaluate the candidates with the
//                   canonical row engine and compact the hits in place at the front of each
//                   sub-bucket; a query whose region or sub-bucket overflowed goes to the sweep.
//  k_range_sweep  : canonical distances of every row for the queries the filter cannot cover
//                   (k_exact_fallback's arithmetic), once to count and once to write.
//  (SET: the rows are a filter's gathered row set -- a candidate is a position in the set's
//   plane, mapped through the ascending id list as it is loaded, and the sweep walks the list.)
//  k_range_scan   : the chunk's counts -> lims (exclusive prefix, carried over the chunks).
//  k_range_gather : a fused query's hits from its sub-buckets to its segment of the hit buffer.
//  k_range_segs + rocPRIM's segmented radix sort: each query's segment by (distance, row id);
//                   a hit is one 64-bit key {order image of the distance bits, row id}.
//  k_range_emit   : sorted hits -> keys / distances below the caller's capacity.
//  k_range_cut / k_range_emit_beam : beam mode, the cut of each sorted beam list by the radius.
//
// Counts come before writes (two passes), so a query's hits have a fixed segment
// [lims[b], lims[b + 1]) whatever order the waves finish in, lims is true even when the
// results do not fit, and what is written below the capacity is the same every time.
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>

#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

// order-preserving image of a non-NaN distance's bits, and back
__device__ __forceinline__ uint32_t range_ord(float d) {
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float range_unord(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ unsigned long long range_key(float d, uint32_t row) {
    return ((unsigned long long)range_ord(d) << 32) | row;
}
// d is a hit of radius r: inclusive, on the canonical distance; NaN and +inf never are
__device__ __forceinline__ bool range_hit(float d, float r) {
    return d <= r && d < __int_as_float(0x7f800000);
}

__global__ void k_range_thr(RangeArgs a, const float* __restrict__ qnorm, const float* __restrict__ qinv, CertArgs c,
                            int fused, float* __restrict__ thr) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const float r = a.radius[b];
    const float nan = __int_as_float(0x7fc00000);
    a.cnt[b] = 0;
    int st = 0;
    float t = nan;
    if (fused < 0) {
        st = 1;  // test option range_force_fallback: every query takes the sweep
    } else if (r != r || (a.g.metric == EUCLIDEAN && r < 0.f) || (a.g.metric == COSINE && qnorm[b] == 0.f)) {
        // a NaN radius, a negative one under L2 (d >= 0), a zero query under cosine (every distance
        // NaN): no hit.  (A negative radius under cosine takes the filter: a distance can round
        // a few ulps below 0.)
        st = 2;
    } else if (!fused || qinv[b] != qinv[b]) {
        st = 1;
    } else {
        const double xe = c.xerr ? (double)*c.xerr : 0.0, qe = c.qerr ? (double)*c.qerr : 0.0;
        double td;
        if (a.g.metric == COSINE) {
            // k_rerank: |score - d| <= eps_cos + ex
            const double ex = 1.01 * (1.0 + 1e-4) * (xe + qe + xe * qe);
            td = (double)r + (double)c.eps_cos + ex;
        } else {
            // k_rerank: |score - d^2| <= delta(q); d = sqrtf(s) <= r only if s <= r^2 (1 + 2^-23 + ..)
            const double qnd = qnorm[b], xm = *c.xmax;
            const double ed = c.eps_dot + 1.01 * (xe + qe + xe * qe);
            const double delta = 2.0 * ed * qnd * xm + c.c_l2 * (qnd + xm) * (qnd + xm);
            td = (double)r * (double)r * (1.0 + 0x1p-22) + delta;
        }
        t = (float)td;
        if ((double)t < td)  // round up
            t = t > 0.f ? __uint_as_float(__float_as_uint(t) + 1u) : t < 0.f ? __uint_as_float(__float_as_uint(t) - 1u) : 1e-45f;
        if (!isfinite(t)) {
            st = 1;
            t = nan;
        }
    }
    thr[b] = t;
    a.state[b] = (uint8_t)st;
    a.sweep[b] = st == 1;
}

template <class C, int G, bool SET>
__global__ __launch_bounds__(256) void k_range_refine(RangeArgs a) {
    const int64_t b = blockIdx.x;
    if (b >= a.B || a.state[b] != 0) return;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    // a lost pair anywhere: the sweep answers the query
    const int n16 = lane < H1_BSUB ? a.qcnt[(b * H1_BSUB + lane) * H1_CSTRIDE] : 0;
    if (a.qovf[b] || __ballot(n16 > a.scap) != 0ull) {
        if (threadIdx.x == 0) a.sweep[b] = 1;
        return;
    }
    const float r = a.radius[b];
    QReg<C> q;
    load_query(q, a.Q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    int total = 0, ncand = 0;
    for (int sb = wave; sb < H1_BSUB; sb += 4) {
        int32_t* cw = a.qcnt + (b * H1_BSUB + sb) * H1_CSTRIDE;
        const int n = uni(cw[0]);
        uint2* bk = a.bucket + (b * H1_BSUB + sb) * (int64_t)a.scap;
        int out = 0;
        for (int base = 0; base < n; base += 64) {
            const int e = base + lane;
            uint32_t row = e < n ? bk[e].x : EMPTY_ID;
            // (positions ascend with the row ids: the order of the hits downstream is the same)
            if constexpr (SET) row = row < (uint32_t)a.m ? a.ids[row] : EMPTY_ID;
            int cnt;
            const uint32_t cid = compact(row, SET ? row != EMPTY_ID : e < n, cnt);
            float myd = __int_as_float(0x7f800000);
            int j = 0;
            eval_list<C, G>(a.g, q, qn, cid, cnt, a.g.metric, [&](float d, uint32_t) {
                if (lane == j) myd = d;
                ++j;
            });
            const bool hit = lane < cnt && range_hit(myd, r);
            const unsigned long long m = __ballot(hit);
            const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            // in place: out <= base, and this batch's entries are already in registers
            if (hit) bk[out + before] = make_uint2(cid, __float_as_uint(myd));
            out += __popcll(m);
        }
        if (lane == 0) cw[1] = out;
        total += out;
        ncand += n;
    }
    if (lane == 0) {
        if (total) atomicAdd(&a.cnt[b], total);
        if (ncand) atomicAdd(a.stat, (unsigned long long)ncand);
    }
}

// the fused queries' hits, sub-bucket after sub-bucket, into [lims[b], lims[b + 1])
__global__ __launch_bounds__(64) void k_range_gather(RangeArgs a) {
    const int64_t b = blockIdx.x;
    if (b >= a.B || a.state[b] != 0 || a.sweep[b]) return;
    const int64_t base = a.lims[b];
    if (base >= a.cap) return;  // nothing of this query is returned
    const int lane = lane_id();
    int64_t off = base;
    for (int sb = 0; sb < H1_BSUB; ++sb) {
        const int n = a.qcnt[(b * H1_BSUB + sb) * H1_CSTRIDE + 1];
        const uint2* bk = a.bucket + (b * H1_BSUB + sb) * (int64_t)a.scap;
        for (int e = lane; e < n; e += 64) {
            const uint2 v = bk[e];
            if (off + e < a.hcap) a.hits[off + e] = range_key(__uint_as_float(v.y), v.x);
        }
        off += n;
    }
}

// Block (b, s): query b (sweep[b] set, else it exits at once), row segment s; its 4 waves take
// a quarter of the segment each.  WRITE = false counts the hits, WRITE = true writes them at
// the query's cursor: per 64-row step one integer atomic per wave that has a hit.
// SET: N is the row set's size and a "row" below a position of its id list -- the rows read
// are a.ids[position], none of them skipped (the list holds no deleted row).
template <class C, int G, bool WRITE, bool SET>
__global__ __launch_bounds__(256) void k_range_sweep(RangeArgs a, int64_t N, int nseg, int64_t seglen) {
    using RM = RowMap<C, G>;
    constexpr int GROUP = C::LPR >> RM::LG;
    const int64_t b = blockIdx.x / nseg;
    const int sg = (int)(blockIdx.x % nseg);
    if (!a.sweep[b]) return;
    const int64_t qbase = WRITE ? a.lims[b] : 0;
    if (WRITE && qbase >= a.cap) return;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const float inf = __int_as_float(0x7f800000);
    const float r = a.radius[b];
    const GraphDev& g = a.g;
    QReg<C> q;
    load_query(q, a.Q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    const int64_t lo = (int64_t)sg * seglen, hi = min(lo + seglen, N);
    const int64_t sub = (max<int64_t>(hi - lo, 0) + 3) / 4;
    const int64_t wlo = lo + w * sub, whi = min(wlo + sub, hi);
    int total = 0;
    for (int64_t base = wlo; base < whi; base += RM::T) {
        uint32_t ids[G];
        bool valid[G];
#pragma unroll
        for (int gg = 0; gg < G; ++gg) {
            const int64_t rr = base + RM::reg_row(gg, lane);
            valid[gg] = rr < whi;
            if constexpr (SET)
                ids[gg] = valid[gg] ? a.ids[rr] : 0u;
            else
                ids[gg] = valid[gg] ? (uint32_t)rr : 0u;
        }
        const float sacc = g.metric == EUCLIDEAN ? eval_rows<C, G, true>(q, g.vecs, g.pitch, ids, valid)
                                                 : eval_rows<C, G, false>(q, g.vecs, g.pitch, ids, valid);
        const int64_t rown = base + RM::owned_row(lane);
        const bool own = rown < whi && (lane & (GROUP - 1)) == 0;
        float d = inf;
        uint32_t rid = (uint32_t)rown;
        if (own) {
            if constexpr (SET) rid = a.ids[rown];
            const float xn = g.metric == COSINE ? g.norms[rid] : 1.f;
            d = finalize(g.metric, sacc, xn, qn);
            if constexpr (!SET)
                if (g.dead && g.dead[rown]) d = inf;
        }
        const bool hit = own && range_hit(d, r);
        const unsigned long long m = __ballot(hit);
        if (!m) continue;
        const int nh = __popcll(m);
        if constexpr (WRITE) {
            int at = 0;
            if (lane == 0) at = atomicAdd(&a.cursor[b], nh);
            at = uni(at);
            const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            const int64_t slot = qbase + at + before;
            if (hit && slot < a.hcap) a.hits[slot] = range_key(d, rid);
        } else {
            total += nh;
        }
    }
    if constexpr (!WRITE) {
        if (lane == 0 && total) atomicAdd(&a.cnt[b], total);
        if (threadIdx.x == 0 && sg == 0) atomicAdd(a.stat + 1, 1ull);
    }
}

// One block: lims[b + 1] = lims[0] + the inclusive prefix of cnt (lims points at the chunk's
// first query, whose entry the previous chunk wrote); the sweep's cursors are zeroed.
__global__ __launch_bounds__(256) void k_range_scan(const int32_t* __restrict__ cnt, int64_t B, int64_t* lims,
                                                    int32_t* __restrict__ cursor) {
    __shared__ int64_t wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t carry = lims[0];
    for (int64_t b0 = 0; b0 < B; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        long long inc = b < B ? cnt[b] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int64_t before = 0;
        for (int i = 0; i < w; ++i) before += wsum[i];
        const int64_t tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (b < B) {
            lims[b + 1] = carry + before + inc;
            if (cursor) cursor[b] = 0;
        }
        carry += tot;
        __syncthreads();
    }
}

// the segments the sort orders: a query none of whose hits is returned has none
__global__ void k_range_segs(const int64_t* __restrict__ lims, int64_t B, int64_t cap, uint32_t* __restrict__ seg_b,
                             uint32_t* __restrict__ seg_e) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const bool active = lims[b] < cap;
    seg_b[b] = active ? (uint32_t)lims[b] : 0u;
    seg_e[b] = active ? (uint32_t)lims[b + 1] : 0u;
}

__global__ __launch_bounds__(256) void k_range_emit(const unsigned long long* __restrict__ sorted,
                                                    const int64_t* __restrict__ total, int64_t cap,
                                                    const int64_t* __restrict__ gkeys, uint32_t capn,
                                                    int64_t* __restrict__ keys, float* __restrict__ dist) {
    const int64_t n = min(*total, cap);
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const unsigned long long v = sorted[p];
        const uint32_t row = (uint32_t)v;
        keys[p] = row < capn ? gkeys[row] : (int64_t)-1;
        dist[p] = range_unord((uint32_t)(v >> 32));
    }
}

// beam mode: the entries of each beam list within the radius (the list is sorted: a prefix)
__global__ __launch_bounds__(64) void k_range_cut(const float* __restrict__ bd, const int32_t* __restrict__ bn, int ef,
                                                  const float* __restrict__ radius, int64_t B,
                                                  int32_t* __restrict__ cnt) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const int lane = lane_id();
    const float r = radius[b];
    const int n = min(bn[b], ef);
    int total = 0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        total += __popcll(__ballot(e < n && range_hit(bd[b * ef + e], r)));
    }
    if (lane == 0) cnt[b] = total;
}

__global__ __launch_bounds__(64) void k_range_emit_beam(const int64_t* __restrict__ bk, const float* __restrict__ bd,
                                                        const int32_t* __restrict__ bn, int ef,
                                                        const float* __restrict__ radius, int64_t B,
                                                        const int64_t* __restrict__ lims, int64_t cap,
                                                        int64_t* __restrict__ keys, float* __restrict__ dist) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const int lane = lane_id();
    const float r = radius[b];
    const int n = min(bn[b], ef);
    int64_t off = lims[b];
    for (int e0 = 0; e0 < n && off < cap; e0 += 64) {
        const int e = e0 + lane;
        const float d = e < n ? bd[b * ef + e] : 0.f;
        const bool hit = e < n && range_hit(d, r);
        const unsigned long long m = __ballot(hit);
        const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        const int64_t p = off + before;
        if (hit && p < cap) {
            keys[p] = bk[b * ef + e];
            dist[p] = d;
        }
        off += __popcll(m);
    }
}

// A host batch of several filters: query b's sorted hits, left at src_off[b] of the staging
// buffers by its filter's pass, to its own segment [lims[b], lims[b + 1]) of the result.
__global__ __launch_bounds__(256) void k_range_place(const int64_t* __restrict__ src_keys,
                                                     const float* __restrict__ src_dist,
                                                     const int64_t* __restrict__ src_off,
                                                     const int64_t* __restrict__ lims, int64_t B,
                                                     int64_t* __restrict__ keys, float* __restrict__ dist) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const int64_t from = src_off[b], to = lims[b], n = lims[b + 1] - to;
    for (int64_t e = threadIdx.x; e < n; e += 256) {
        keys[to + e] = src_keys[from + e];
        dist[to + e] = src_dist[from + e];
    }
}

// ---------------------------------------------------------------------------
int launch_range_thr(const RangeArgs& a, const float* qnorm, const float* qinv, const CertArgs& c, int fused, float* thr,
                     hipStream_t s) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(k_range_thr, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, s, a, qnorm, qinv, c, fused, thr);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_range_refine(const RangeArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.B <= 0) return 0;
    return with_cfg(lpr, vpl, [&](auto cfg) {
        if (a.ids)
            hipLaunchKernelGGL((k_range_refine<Cfg<cfg.L, cfg.V>, cfg.G, true>), dim3((unsigned)a.B), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((k_range_refine<Cfg<cfg.L, cfg.V>, cfg.G, false>), dim3((unsigned)a.B), dim3(256), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

int launch_range_gather(const RangeArgs& a, hipStream_t s) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(k_range_gather, dim3((unsigned)a.B), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_range_sweep(const RangeArgs& a, int64_t N, int nseg, int64_t seglen, bool write, int lpr, int vpl,
                       hipStream_t s) {
    if (a.B <= 0 || N <= 0) return 0;
    if (nseg < 1 || seglen < 1 || (a.ids && N != a.m)) return -4;
    const dim3 grid((unsigned)(a.B * nseg));
    return with_cfg(lpr, vpl, [&](auto c) {
        using C = Cfg<c.L, c.V>;
        constexpr int GF = c.G < 4 ? c.G : 4;
        if (a.ids && write)
            hipLaunchKernelGGL((k_range_sweep<C, GF, true, true>), grid, dim3(256), 0, s, a, N, nseg, seglen);
        else if (a.ids)
            hipLaunchKernelGGL((k_range_sweep<C, GF, false, true>), grid, dim3(256), 0, s, a, N, nseg, seglen);
        else if (write)
            hipLaunchKernelGGL((k_range_sweep<C, GF, true, false>), grid, dim3(256), 0, s, a, N, nseg, seglen);
        else
            hipLaunchKernelGGL((k_range_sweep<C, GF, false, false>), grid, dim3(256), 0, s, a, N, nseg, seglen);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

int launch_range_scan(const int32_t* cnt, int64_t B, int64_t* lims, int32_t* cursor, hipStream_t s) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(256), 0, s, cnt, B, lims, cursor);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int range_sort_temp_bytes(int64_t hcap, int64_t B, size_t* bytes) {
    *bytes = 0;
    const hipError_t e = rocprim::segmented_radix_sort_keys(
        nullptr, *bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned)hcap, (unsigned)B,
        (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, 64u, (hipStream_t) nullptr);
    return e == hipSuccess ? 0 : -1;
}

// hits[seg] sorted into sorted[seg] per query
int launch_range_order(const unsigned long long* hits, unsigned long long* sorted, int64_t hcap, const int64_t* lims,
                       int64_t B, int64_t cap, uint32_t* seg_b, uint32_t* seg_e, void* temp, size_t temp_bytes,
                       hipStream_t s) {
    if (B <= 0) return 0;
    if (hcap <= 0 || hcap > (int64_t)0x7fffffff || B > (int64_t)0x7fffffff) return -4;
    hipLaunchKernelGGL(k_range_segs, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, lims, B, cap, seg_b, seg_e);
    if (hipGetLastError() != hipSuccess) return -1;
    const hipError_t e = rocprim::segmented_radix_sort_keys(temp, temp_bytes, hits, sorted, (unsigned)hcap, (unsigned)B,
                                                            (const uint32_t*)seg_b, (const uint32_t*)seg_e, 0u, 64u, s);
    return e == hipSuccess ? 0 : -1;
}

// ... then the keys and distances below cap
int launch_range_order_emit(const unsigned long long* hits, unsigned long long* sorted, int64_t hcap,
                            const int64_t* lims, int64_t B, int64_t cap, uint32_t* seg_b, uint32_t* seg_e, void* temp,
                            size_t temp_bytes, const GraphDev& g, int64_t* keys, float* dist, hipStream_t s) {
    if (B <= 0) return 0;
    if (const int r = launch_range_order(hits, sorted, hcap, lims, B, cap, seg_b, seg_e, temp, temp_bytes, s)) return r;
    if (cap <= 0) return 0;
    const int64_t blocks = std::min<int64_t>((cap + 255) / 256, 8192);
    hipLaunchKernelGGL(k_range_emit, dim3((unsigned)blocks), dim3(256), 0, s, sorted, lims + B, cap, g.keys, g.capn, keys,
                       dist);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_range_place(const int64_t* src_keys, const float* src_dist, const int64_t* src_off, const int64_t* lims,
                       int64_t B, int64_t* keys, float* dist, hipStream_t s) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(k_range_place, dim3((unsigned)B), dim3(256), 0, s, src_keys, src_dist, src_off, lims, B, keys,
                       dist);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_range_beam(const int64_t* bk, const float* bd, const int32_t* bn, int ef, const float* radius, int64_t B,
                      int32_t* cnt, int64_t* lims, int64_t cap, int64_t* keys, float* dist, hipStream_t s) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(k_range_cut, dim3((unsigned)B), dim3(64), 0, s, bd, bn, ef, radius, B, cnt);
    hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(256), 0, s, cnt, B, lims, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_range_emit_beam, dim3((unsigned)B), dim3(64), 0, s, bk, bd, bn, ef, radius, B, lims, cap, keys,
                       dist);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mh
