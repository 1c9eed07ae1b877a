// wide.hip -- exact search past k 256 (search_host.cpp wide_exact; option "exact_wide"): the
// range pipeline run at a per-query radius estimated from the sample pass, then a cut at k.
// The kernels here are the three steps around range.hip's:
//
//  k_wide_radius : per query the J-th smallest score of the sample (a radix select on the
//                  order image of the score bits, one byte per pass), turned into a distance
//                  radius and widened by the certificate's bound |score - distance|, so that
//                  the J sample rows at or below the score all lie within it.
//  k_wide_emit   : a query whose sorted segment holds >= k hits writes its first k to [b, :k];
//                  every other query joins the list of short queries.
//  k_wide_dist + k_wide_select : the short queries, a group at a time: the canonical distance
//                  of every row (k_exact_fallback's arithmetic; NaN marks a row that is
//                  skipped), a radix select of the min(k, qualifying) smallest 64-bit keys
//                  {order image of the distance, row id}, a bitonic sort of them in LDS, the
//                  emit.  A group past the end of the list exits at once: the host never
//                  learns the list's length.
//
// Choice of J (search_host.cpp wide_rank_for).  The sample is a subset of the rows, a fraction
// f of them.  Let X be the number of the query's k nearest rows that fell into the sample.  If
// X < J the J-th smallest sample score belongs to a row outside the k nearest, so the radius
// holds the k nearest.  X is hypergeometric, dominated in its upper tail by Poisson(k f): J is
// the smallest rank with P(Poisson(k f) >= J) <= 1e-5, and never more than k (the J = k-th
// sample score bounds k rows whatever f is -- at f = 1 the estimate is exact).  A query whose
// J exceeds the sample, whose J-th sample score is not finite, or that cannot be scored in
// fp16 gets a NaN radius: the range pipeline finds no hit and the query is short.
//
// Ties.  A hit is ordered by its 64-bit key in the segment sort and here alike, so rows at
// the k-th distance come out in row-id order on either path.
#include <algorithm>

#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

// order-preserving image of a distance's bits (range.hip range_ord); NaN sorts last
__device__ __forceinline__ uint32_t wide_ord(float d) {
    if (d != d) return 0xFFFFFFFFu;
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float wide_unord(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
constexpr uint32_t WIDE_ORD_INF = 0xFF800000u;  // wide_ord(+inf)

// The want-th smallest (1-based) of the keys load(i, key) yields for i in [0, n), at least
// `want` of them: a radix select from the top byte down.  Every thread of the block calls it;
// hist is 256 words of LDS, sh two.  A wave first merges the lanes that share its first
// lane's bin into one atomic (scores of one query mostly share their top bytes).
template <class K, class Load>
__device__ __forceinline__ K wide_rank(int64_t n, uint32_t want, Load load, uint32_t* hist, uint32_t* sh) {
    K prefix = 0, mask = 0;
    const int64_t steps = (n + blockDim.x - 1) / blockDim.x;
    for (int shift = 8 * (int)sizeof(K) - 8; shift >= 0; shift -= 8) {
        for (int t = threadIdx.x; t < 256; t += blockDim.x) hist[t] = 0u;
        __syncthreads();
        for (int64_t st = 0; st < steps; ++st) {
            const int64_t i = st * blockDim.x + threadIdx.x;
            K key = 0;
            const bool in = i < n && load(i, key) && (key & mask) == prefix;
            const uint32_t bin = (uint32_t)(key >> shift) & 255u;
            const unsigned long long act = __ballot(in);
            if (!act) continue;
            const uint32_t b0 = (uint32_t)__shfl((int)bin, __builtin_ctzll(act), 64);
            const unsigned long long same = __ballot(in && bin == b0);
            if (in && bin != b0)
                atomicAdd(&hist[bin], 1u);
            else if (in && (same & ((1ull << lane_id()) - 1ull)) == 0ull)
                atomicAdd(&hist[b0], (uint32_t)__popcll(same));
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const uint32_t sum = c0 + c1 + c2 + c3;
            uint32_t inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
                if (lane >= o) inc += t;
            }
            const uint32_t exc = inc - sum;
            if (exc < want && want <= inc) {  // one lane: the bin that holds the rank
                uint32_t before = exc;
                int bin = 4 * lane;
                if (want > before + c0) {
                    before += c0;
                    bin = 4 * lane + 1;
                    if (want > before + c1) {
                        before += c1;
                        bin = 4 * lane + 2;
                        if (want > before + c2) {
                            before += c2;
                            bin = 4 * lane + 3;
                        }
                    }
                }
                sh[0] = (uint32_t)bin;
                sh[1] = before;
            }
        }
        __syncthreads();
        prefix |= (K)sh[0] << shift;
        mask |= (K)0xFFu << shift;
        want -= sh[1];
        __syncthreads();
    }
    return prefix;
}

__global__ __launch_bounds__(256) void k_wide_radius(WideRadiusArgs a) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[2];
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;
    const float nan = __int_as_float(0x7fc00000);
    // (block-uniform) no estimate: the test option, a sample smaller than J, a zero query under
    // cosine, a query outside the fp16 bound
    bool ok = !a.force && a.J >= 1 && a.ns >= (int64_t)a.J;
    if (ok) ok = !(a.metric == COSINE && a.qnorm[b] == 0.f) && a.qinv[b] == a.qinv[b];
    if (!ok) {
        if (threadIdx.x == 0) a.radius[b] = nan;
        return;
    }
    const float* __restrict__ row = a.scores + (size_t)b * a.ldS;
    const uint32_t img = wide_rank<uint32_t>(
        a.ns, (uint32_t)a.J,
        [&](int64_t i, uint32_t& key) {
            key = wide_ord(row[i]);
            return true;
        },
        hist, sh);
    if (threadIdx.x != 0) return;
    float r = nan;
    if (img < WIDE_ORD_INF) {
        const double sc = (double)wide_unord(img);
        const CertArgs& c = a.c;
        const double xe = c.xerr ? (double)*c.xerr : 0.0, qe = c.qerr ? (double)*c.qerr : 0.0;
        double rd;
        if (a.metric == COSINE) {
            // k_rerank: |score - d| <= eps_cos + ex
            rd = sc + (double)c.eps_cos + 1.01 * (1.0 + 1e-4) * (xe + qe + xe * qe);
        } else {
            // k_rerank: |score - d^2| <= delta(q), d = sqrtf(d^2)
            const double qnd = a.qnorm[b], xm = *c.xmax;
            const double ed = c.eps_dot + 1.01 * (xe + qe + xe * qe);
            const double delta = 2.0 * ed * qnd * xm + c.c_l2 * (qnd + xm) * (qnd + xm);
            rd = sqrt(fmax(sc + delta, 0.0)) * (1.0 + 0x1p-22);
        }
        r = (float)rd;
        if ((double)r < rd)  // round up
            r = r > 0.f ? __uint_as_float(__float_as_uint(r) + 1u) : r < 0.f ? __uint_as_float(__float_as_uint(r) - 1u) : 1e-45f;
        if (!isfinite(r)) r = nan;
    }
    a.radius[b] = r;
}

// stat[0] += short queries (their list index), stat[1] += hits that reached the sort
__global__ __launch_bounds__(256) void k_wide_emit(WideEmitArgs a) {
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;
    const int64_t lo = a.lims[b], cnt = a.lims[b + 1] - lo;
    const bool room = lo < a.cap;  // (a query that starts past cap wrote nothing)
    if (threadIdx.x == 0 && room && cnt > 0) atomicAdd(a.stat + 1, (unsigned long long)cnt);
    if (!room || cnt < a.k) {
        if (threadIdx.x == 0) a.shortq[atomicAdd(a.stat, 1ull)] = (int32_t)b;
        return;
    }
    for (int e = threadIdx.x; e < a.k; e += 256) {
        const unsigned long long v = a.sorted[lo + e];
        const uint32_t row = (uint32_t)v;
        a.out_keys[b * a.k + e] = row < a.capn ? a.keys[row] : (int64_t)-1;
        a.out_dist[b * a.k + e] = wide_unord((uint32_t)(v >> 32));
        if (a.out_ids) a.out_ids[b * a.k + e] = (int32_t)row;
    }
    if (threadIdx.x == 0) a.out_n[b] = a.k;
}

// Canonical distance of every row of the index for the short queries [g0, g0 + G) of the list
// (k_exact_fallback's arithmetic), row f - g0 of wd; a row g.dead masks gets NaN, as a NaN
// distance: neither is returned.  Rows outside, queries inside: a row group is read once from
// memory and then from the caches.
template <class C, int G>
__global__ __launch_bounds__(256) void k_wide_dist(const float* __restrict__ Q, GraphDev g, int64_t N,
                                                   const int32_t* __restrict__ shortq,
                                                   const unsigned long long* __restrict__ stat, int64_t g0, int64_t gn,
                                                   float* __restrict__ wd, int64_t ldW) {
    using RM = RowMap<C, G>;
    constexpr int GROUP = C::LPR >> RM::LG;
    const int64_t ns = (int64_t)*stat;
    if (ns <= g0) return;
    const int nf = (int)min(gn, ns - g0);
    const int lane = lane_id();
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;
    const int64_t ngroups = (N + RM::T - 1) / RM::T;
    for (int64_t grp = gw; grp < ngroups; grp += nw) {
        const int64_t base = grp * RM::T;
        uint32_t ids[G];
        bool valid[G];
#pragma unroll
        for (int gg = 0; gg < G; ++gg) {
            const int64_t r = base + RM::reg_row(gg, lane);
            valid[gg] = r < N;
            ids[gg] = valid[gg] ? (uint32_t)r : 0u;
        }
        const int64_t rown = base + RM::owned_row(lane);
        const bool own = rown < N && (lane & (GROUP - 1)) == 0;
        const float xn = own && g.metric == COSINE ? g.norms[rown] : 1.f;
        const bool gone = own && g.dead && g.dead[rown];
        for (int f = 0; f < nf; ++f) {
            const int64_t b = shortq[g0 + f];
            QReg<C> q;
            load_query(q, Q + (size_t)b * C::PITCH);
            const float qn = query_norm(q);
            const float sacc = g.metric == EUCLIDEAN ? eval_rows<C, G, true>(q, g.vecs, g.pitch, ids, valid)
                                                     : eval_rows<C, G, false>(q, g.vecs, g.pitch, ids, valid);
            if (own) wd[(size_t)f * ldW + rown] = gone ? __int_as_float(0x7fc00000) : finalize(g.metric, sacc, xn, qn);
        }
    }
}

constexpr int WIDE_MAX_K = 4096;

// Block f: short query g0 + f of the list (past its end: exit).  The min(k, qualifying)
// smallest keys of its distance row, sorted, emitted; the rest of [b, :k] is padded as
// k_rerank pads it.
__global__ __launch_bounds__(1024) void k_wide_select(WideEmitArgs a, const unsigned long long* __restrict__ stat,
                                                      int64_t g0, int64_t N, const float* __restrict__ wd,
                                                      int64_t ldW) {
    __shared__ unsigned long long keys[WIDE_MAX_K];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[2];
    __shared__ uint32_t cnt[2];
    const int64_t f = blockIdx.x;
    if ((int64_t)*stat <= g0 + f) return;
    const int64_t b = a.shortq[g0 + f];
    const float* __restrict__ row = wd + (size_t)f * ldW;
    const int tid = threadIdx.x, nth = blockDim.x;
    if (tid < 2) cnt[tid] = 0u;
    __syncthreads();
    // the rows that qualify: every distance but NaN (+inf is a distance)
    uint32_t mine = 0;
    for (int64_t i = tid; i < N; i += nth) mine += row[i] == row[i];
    for (int o = 32; o >= 1; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o, 64);
    if ((tid & 63) == 0 && mine) atomicAdd(&cnt[0], mine);
    __syncthreads();
    const int kq = (int)min((uint32_t)a.k, cnt[0]);
    const auto load = [&](int64_t i, unsigned long long& key) {
        const float d = row[i];
        key = ((unsigned long long)wide_ord(d) << 32) | (uint32_t)i;
        return d == d;
    };
    int P = 1;
    if (kq > 0) {
        const unsigned long long T = wide_rank<unsigned long long>(N, (uint32_t)kq, load, hist, sh);
        while (P < kq) P <<= 1;
        for (int e = kq + tid; e < P; e += nth) keys[e] = ~0ull;
        for (int64_t i = tid; i < N; i += nth) {
            unsigned long long key;
            if (load(i, key) && key <= T) {
                const uint32_t at = atomicAdd(&cnt[1], 1u);
                if (at < (uint32_t)kq) keys[at] = key;  // (the keys are distinct: exactly kq of them)
            }
        }
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (P >> 1); t += nth) {
                    const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const unsigned long long x = keys[i], y = keys[j];
                    if ((x > y) == ((i & size) == 0)) {
                        keys[i] = y;
                        keys[j] = x;
                    }
                }
                __syncthreads();
            }
    }
    for (int e = tid; e < a.k; e += nth) {
        const bool okr = e < kq;
        const unsigned long long v = okr ? keys[e] : 0ull;
        const uint32_t id = (uint32_t)v;
        a.out_keys[b * a.k + e] = okr && id < a.capn ? a.keys[id] : (int64_t)-1;
        a.out_dist[b * a.k + e] = okr ? wide_unord((uint32_t)(v >> 32)) : __int_as_float(0x7f800000);
        if (a.out_ids) a.out_ids[b * a.k + e] = okr ? (int32_t)id : -1;
    }
    if (tid == 0) a.out_n[b] = kq;
}

// ---------------------------------------------------------------------------
int launch_wide_radius(const WideRadiusArgs& a, hipStream_t s) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(k_wide_radius, dim3((unsigned)a.B), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_wide_emit(const WideEmitArgs& a, hipStream_t s) {
    if (a.B <= 0) return 0;
    if (a.k < 1 || a.k > WIDE_MAX_K) return -4;
    hipLaunchKernelGGL(k_wide_emit, dim3((unsigned)a.B), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_wide_fallback(const float* Q, const GraphDev& g, int64_t N, const WideEmitArgs& a, int64_t g0, int64_t gn,
                         float* wd, int64_t ldW, int lpr, int vpl, hipStream_t s) {
    if (gn <= 0 || N <= 0) return 0;
    if (a.k < 1 || a.k > WIDE_MAX_K || ldW < N || N > (int64_t)0x7fffffff) return -4;
    const int r = with_cfg(lpr, vpl, [&](auto c) {
        hipLaunchKernelGGL((k_wide_dist<Cfg<c.L, c.V>, (c.G < 4 ? c.G : 4)>), dim3(1024), dim3(256), 0, s, Q, g, N,
                           a.shortq, a.stat, g0, gn, wd, ldW);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
    if (r) return r;
    hipLaunchKernelGGL(k_wide_select, dim3((unsigned)gn), dim3(1024), 0, s, a, a.stat, g0, N, wd, ldW);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mh
