// part_scan.hip -- the partition search run partition-major (DESIGN.md §6 "Partition scan"): the
// rows of a probed partition are read once per tile of the queries that probe it and scored on
// v_mfma_f32_16x16x32_f16, instead of once per query by k_part_search's one-wave walk.  The
// results are the walk's, bit for bit: the scan only decides which rows reach the canonical row
// engine.
//
//  k_ps_rank<FIN = false> : the seed.  One wave per query walks its first `seed` probes exactly
//                  as k_part_search does (the ranking body restated: that kernel is left as it
//                  is) and writes its list.  A full list's k-th distance w is a radius no row
//                  outside it can beat from above: the certificate (cert.hpp cert_score_thr)
//                  turns it into the score threshold t -- distance <= w implies score <= t.
//                  No finite threshold (a short list, a zero query under cosine, a query
//                  outside the fp16 bound): t = NaN, the query walks.
//  k_ps_live     : the live rows of each list (the walk's own test), for out_ncand.
//  k_ps_pairs + rocPRIM radix_sort_pairs + k_ps_plan : the probes seed .. nprobe - 1 of the
//                  queries with a threshold as (partition, query) pairs by partition; per
//                  partition its queries' offsets and the first of its items, an item being
//                  one (query tile, row tile) of the partition.
//  k_part_scan   : a persistent grid over the items, query tiles fastest.  One workgroup per
//                  item, 4 waves of 32 queries x 64 rows (2 x 4 accumulator blocks of 16 x 16).
//                  The tile's rows are gathered from the K-blocked fp16 plane through the id
//                  list, its queries through the sorted pairs: per 32-deep K-slice a thread
//                  moves one 16-byte half of a row's 32-byte K-block run for a query and two
//                  rows, through registers into a double-buffered LDS image of 80-byte rows
//                  (64 + 16 of padding: the 16 rows a quarter of a ds_read_b128 touches land in
//                  16 distinct 16-byte slots of the 256-byte bank window).  The epilogue forms
//                  split_score from the accumulator and appends the rows with score <= t to
//                  the query's survivor segment: one atomic per 16-lane group (one query) that
//                  has any.  Past `room` an append only counts.  No dot is written.
//  k_ps_rank<FIN = true> : the finish.  The seed list reloaded, the survivors ranked by
//                  eval_list and (distance, row id) -- the survivors are a superset of the
//                  rows that can enter, and the list's order does not depend on theirs.  A
//                  query without a threshold or with more survivors than room: the walk over
//                  all its probes, from an empty list.
//
// part_scan_seed = 0 takes the radius from the scan itself; no partition is walked for it:
//  k_ps_pairs .. k_ps_plan over probe 0 alone, of the queries that can have a threshold and
//                  whose nearest list fits `seed_room` scores.
//  k_part_seed_scan : the tile body again with another epilogue: the scores are written, the
//                  score of position j of the query's nearest list to sscore[b][j] (+inf: a dead
//                  row, an id past n, a NaN score), straight from the accumulator layout -- the
//                  16 lanes of a group hold 16 consecutive positions of one query, a 64-byte run.
//  k_ps_pick     : one wave per query selects its k best-scored positions, evaluates those k
//                  rows canonically and turns their largest distance w into the threshold.  The
//                  k rows are distinct live probed rows, so the true k-th distance is <= w
//                  whatever the fp16 scores chose; they come back as survivors of their own
//                  partition (the pairs then run over every probe) and the finish ranks from an
//                  empty list.
#include <rocprim/device/device_radix_sort.hpp>

#include "cert.hpp"
#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

typedef float ps_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 ps_f16x8 __attribute__((ext_vector_type(8)));

constexpr int PS_RB = 80;  // bytes of an image row: a 32-deep fp16 K-slice and the padding
constexpr int PS_IMG = (PSCAN_BM + PSCAN_BN) * PS_RB;
constexpr int PS_GRID = 2048;

// ---- seed and finish ----
// k_part_search's walk over the probes [t0, t1) into L; returns the live rows met
template <class C, int G, int R, bool SCREEN>
__device__ __forceinline__ int ps_walk(const PartSearchArgs& a, int64_t b, const QReg<C>& q, float qn, BList<R>& L, int t0,
                                       int t1) {
    const int lane = lane_id();
    const float inf = __int_as_float(0x7f800000);
    const bool screen = SCREEN && a.g.h16 && h16_query_ok(qn);
    float margin = 0.f;
    if constexpr (SCREEN) {
        const float e = a.g.h16err ? *a.g.h16err : 0.00048828125f;
        margin = (a.g.metric == EUCLIDEAN ? h16_margin_l2(e) : h16_margin_cos(e)) + MH_SCREEN_PAD;
    }
    int ncand = 0;
    unsigned long long s16 = 0;
    const uint32_t n = (uint32_t)a.n;
    auto sink = [&](float d, uint32_t u) { bl_insert(L, a.k, d, u); };
    for (int t = t0; t < t1; ++t) {
        const int p = a.probe[b * a.nprobe + t];
        const uint32_t lo = (uint32_t)a.off[p], ub = min((uint32_t)a.off[p + 1], n);
        for (uint32_t j0 = lo; j0 < ub; j0 += 64) {
            const uint32_t j = j0 + lane;
            const uint32_t id = j < ub ? a.sorted_id[j] : EMPTY_ID;
            const bool keep = j < ub && id < n && id < a.g.capn && !is_dead(a.g, id);
            int cnt;
            const uint32_t cid = compact(id, keep, cnt);
            if (cnt == 0) continue;
            ncand += cnt;
            float wd;
            uint32_t wi;
            bl_at(L, a.k - 1, wd, wi);
            if (SCREEN && screen && wi != EMPTY_ID && wd < inf)
                eval_screened<C, G>(a.g, q, qn, cid, cnt, a.g.metric, wd, sink, s16, margin);
            else
                eval_list<C, G>(a.g, q, qn, cid, cnt, a.g.metric, sink);
        }
    }
    return ncand;
}

template <int LPR, int VPL, int R, int G, bool SCREEN, bool FIN>
__global__ __launch_bounds__(64, 2) void k_ps_rank(PartScanArgs a) {
    using C = Cfg<LPR, VPL>;
    const PartSearchArgs& w = a.s;
    const int64_t b = blockIdx.x;
    if (b >= w.B) return;
    const int lane = lane_id();
    const float inf = __int_as_float(0x7f800000);
    QReg<C> q;
    load_query(q, w.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    BList<R> L;
    bl_init(L);
    if constexpr (!FIN) {
        (void)ps_walk<C, G, R, SCREEN>(w, b, q, qn, L, 0, a.seed);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = r * 64 + lane;
            if (idx < w.k) {
                a.seed_d[b * w.k + idx] = L.d[r];
                a.seed_i[b * w.k + idx] = L.i[r];
            }
        }
        float wd;
        uint32_t wi;
        bl_at(L, w.k - 1, wd, wi);
        float t = __int_as_float(0x7fc00000);
        const float qi = a.qinv[b], qnb = a.qnorm[b];
        // (inclusive: a row at exactly wd with a lower id outranks the list's last entry)
        if (wi != EMPTY_ID && wd < inf && qi == qi && !(w.g.metric == COSINE && qnb == 0.f))
            t = cert_score_thr(w.g.metric, wd, qnb, a.c);
        if (lane == 0) {
            a.thr[b] = t;
            a.scnt[b] = 0u;
        }
        return;
    } else {
        const float t = a.thr[b];
        const uint32_t cnt = a.scnt[b];
        const bool walk = !(t == t) || cnt > (uint32_t)a.room;
        int ncand = 0;
        if (walk) {
            ncand = ps_walk<C, G, R, SCREEN>(w, b, q, qn, L, 0, w.nprobe);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int idx = r * 64 + lane;
                if (idx < w.k) {
                    L.d[r] = a.seed_d[b * w.k + idx];
                    L.i[r] = a.seed_i[b * w.k + idx];
                }
            }
            const uint32_t* sv = a.surv + (size_t)b * a.room;
            for (uint32_t base = 0; base < cnt; base += 64) {
                const uint32_t e = base + lane;
                const uint32_t id = e < cnt ? sv[e] : EMPTY_ID;
                int m;
                const uint32_t cid = compact(id, e < cnt && id < w.g.capn, m);
                if (m == 0) continue;
                eval_list<C, G>(w.g, q, qn, cid, m, w.g.metric, [&](float d, uint32_t u) { bl_insert(L, w.k, d, u); });
            }
            for (int t0 = lane; t0 < w.nprobe; t0 += 64) ncand += a.live[w.probe[b * w.nprobe + t0]];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) ncand += __shfl_xor(ncand, o, 64);
        }
        int nv = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = r * 64 + lane;
            const bool okr = idx < w.k && L.i[r] != EMPTY_ID;
            if (idx < w.k) {
                const uint32_t id = L.i[r] & ID_MASK;
                w.out_keys[b * w.k + idx] = okr ? w.g.keys[id] : (int64_t)-1;
                w.out_dist[b * w.k + idx] = okr ? L.d[r] : inf;
            }
            nv += __popcll(__ballot(okr));
        }
        if (lane == 0) {
            w.out_n[b] = nv;
            w.out_ncand[b] = ncand;
            if (w.stat) atomicAdd(w.stat, (unsigned long long)ncand);
            if (walk)
                atomicAdd(a.stat + 1, 1ull);
            else if (cnt)
                atomicAdd(a.stat, (unsigned long long)cnt);
        }
    }
}

template <int L_, int V_, int G_, int R, bool FIN>
static int launch_ps_rank_r(const PartScanArgs& a, hipStream_t s) {
    if (a.s.g.h16)
        hipLaunchKernelGGL((k_ps_rank<L_, V_, R, G_, true, FIN>), dim3((unsigned)a.s.B), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((k_ps_rank<L_, V_, R, G_, false, FIN>), dim3((unsigned)a.s.B), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <bool FIN>
static int launch_ps_rank(const PartScanArgs& a, int lpr, int vpl, hipStream_t s) {
    const PartSearchArgs& w = a.s;
    if (w.B <= 0) return 0;
    // (seed 0: k_ps_pick stands in for the seed launch, and one probe is enough)
    if (w.k < 1 || w.k > 256 || w.nprobe < 1 || w.nprobe > PART_MAX_PROBE || a.seed < (FIN ? 0 : 1) ||
        (a.seed > 0 && a.seed >= w.nprobe) || a.room < 1)
        return -4;
    return with_cfg(lpr, vpl, [&](auto c) {
        constexpr int GS = c.G < 4 ? c.G : 4;  // (k_part_search's limit on the rows in flight)
        if (w.k <= 64) return launch_ps_rank_r<c.L, c.V, GS, 1, FIN>(a, s);
        if (w.k <= 128) return launch_ps_rank_r<c.L, c.V, GS, 2, FIN>(a, s);
        return launch_ps_rank_r<c.L, c.V, GS, 4, FIN>(a, s);
    });
}

int launch_part_scan_seed(const PartScanArgs& a, int lpr, int vpl, hipStream_t s) { return launch_ps_rank<false>(a, lpr, vpl, s); }
int launch_part_scan_finish(const PartScanArgs& a, int lpr, int vpl, hipStream_t s) { return launch_ps_rank<true>(a, lpr, vpl, s); }

// ---- inversion ----
// one wave per partition: the rows of its list the walk would keep
__global__ __launch_bounds__(64) void k_ps_live(PartScanArgs a) {
    const PartSearchArgs& w = a.s;
    const int p = blockIdx.x, lane = lane_id();
    const uint32_t n = (uint32_t)w.n;
    const uint32_t lo = (uint32_t)w.off[p], ub = min((uint32_t)w.off[p + 1], n);
    int cnt = 0;
    for (uint32_t j = lo + lane; j < ub; j += 64) {
        const uint32_t id = w.sorted_id[j];
        cnt += id < n && id < w.g.capn && !is_dead(w.g, id) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) a.live[p] = cnt;
}

// the probes an inversion covers: [seed, nprobe), or probe 0 alone for the seed scan
__host__ __device__ __forceinline__ int ps_pair_probes(const PartScanArgs& a) { return a.seed_pass ? 1 : a.s.nprobe - a.seed; }

// Does query b take part in the seed scan?  It can have a threshold at all (k_ps_rank's own
// conditions) and its nearest list [lo, lo + m) fits the score row.
__device__ __forceinline__ bool ps_seed_takes(const PartScanArgs& a, int64_t b, uint32_t& lo, uint32_t& m) {
    const PartSearchArgs& w = a.s;
    const float qi = a.qinv[b];
    const uint32_t p = (uint32_t)w.probe[b * w.nprobe];
    lo = m = 0;
    if (!(qi == qi) || (w.g.metric == COSINE && a.qnorm[b] == 0.f) || p >= (uint32_t)a.P) return false;
    lo = (uint32_t)w.off[p];
    const uint32_t ub = min((uint32_t)w.off[p + 1], (uint32_t)w.n);
    m = ub > lo ? ub - lo : 0u;
    return m <= (uint32_t)a.seed_room;
}

__global__ void k_ps_pairs(PartScanArgs a) {
    const PartSearchArgs& w = a.s;
    const int m = ps_pair_probes(a);
    const int64_t total = w.B * m;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = e / m;
        const int t = a.seed_pass ? 0 : a.seed + (int)(e % m);
        bool in;
        if (a.seed_pass) {
            uint32_t lo, len;
            in = ps_seed_takes(a, b, lo, len);
        } else {
            const float thr = a.thr[b];
            in = thr == thr;
        }
        const uint32_t p = (uint32_t)w.probe[b * w.nprobe + t];
        a.pkey[e] = in && p < (uint32_t)a.P ? p : (uint32_t)a.P;
        a.pval[e] = (uint32_t)b;
    }
}

// One workgroup.  poff[t] = the first sorted pair with a key >= t, t in [0, P + 1]; ibase = the
// exclusive prefix of the partitions' items (query tiles x row tiles).
__global__ __launch_bounds__(1024) void k_ps_plan(PartScanArgs a) {
    __shared__ int sOff[PART_MAX_P + 2];
    __shared__ int sSum[1024];
    const PartSearchArgs& w = a.s;
    const int tid = threadIdx.x;
    const int64_t npairs = w.B * ps_pair_probes(a);
    for (int t = tid; t <= a.P + 1; t += 1024) {
        int64_t lo = 0, hi = npairs;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.skey[mid] < (uint32_t)t)
                lo = mid + 1;
            else
                hi = mid;
        }
        sOff[t] = (int)lo;
        a.poff[t] = (int)lo;
    }
    __syncthreads();
    constexpr int PER = PART_MAX_P / 1024;
    int items[PER], mine = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = tid * PER + i;
        items[i] = 0;
        if (p < a.P) {
            const int nq = sOff[p + 1] - sOff[p];
            const int64_t ub = w.off[p + 1] < w.n ? (int64_t)w.off[p + 1] : w.n;
            const int64_t rows = ub > w.off[p] ? ub - w.off[p] : 0;
            items[i] = ((nq + PSCAN_BM - 1) / PSCAN_BM) * (int)((rows + PSCAN_BN - 1) / PSCAN_BN);
        }
        mine += items[i];
    }
    sSum[tid] = mine;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? sSum[tid - o] : 0;
        __syncthreads();
        sSum[tid] += v;
        __syncthreads();
    }
    int run = sSum[tid] - mine;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = tid * PER + i;
        if (p < a.P) a.ibase[p] = run;
        run += items[i];
    }
    if (tid == 1023) a.ibase[a.P] = sSum[1023];
}

static int ps_key_bits(int P) {
    int bits = 1;
    while ((1 << bits) <= P) ++bits;  // keys in [0, P]
    return bits;
}

int part_scan_temp_bytes(int64_t pairs, size_t* bytes) {
    *bytes = 0;
    const hipError_t e =
        rocprim::radix_sort_pairs(nullptr, *bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)pairs, 0u, 32u, (hipStream_t) nullptr);
    return e == hipSuccess ? 0 : -1;
}

// (the radix sort is stable and the queries go in ascending: a partition's queries keep that order)
int launch_part_scan_invert(const PartScanArgs& a, hipStream_t s) {
    const int64_t pairs = a.s.B * ps_pair_probes(a);
    if (pairs <= 0 || a.P < 1 || a.P > PART_MAX_P || (a.seed_pass && (a.seed != 0 || a.seed_room < 1))) return -4;
    if (!a.seed_pass) hipLaunchKernelGGL(k_ps_live, dim3((unsigned)a.P), dim3(64), 0, s, a);
    const int grid = (int)std::min<int64_t>((pairs + 255) / 256, 4096);
    hipLaunchKernelGGL(k_ps_pairs, dim3(grid), dim3(256), 0, s, a);
    size_t tb = a.temp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs(a.temp, tb, a.pkey, a.skey, a.pval, a.sval, (size_t)pairs, 0u,
                                                   (unsigned)ps_key_bits(a.P), s);
    if (e != hipSuccess) return -1;
    hipLaunchKernelGGL(k_ps_plan, dim3(1), dim3(1024), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the scan ----
__global__ __launch_bounds__(256) void k_part_scan(PartScanArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sImg[2][PS_IMG];
    __shared__ uint32_t sRow[PSCAN_BN];  // the tile's row ids (EMPTY_ID: past the end, dead)
    __shared__ uint32_t sQ[PSCAN_BM];    // its queries (EMPTY_ID past the end)
    __shared__ float sXi[PSCAN_BN], sXn[PSCAN_BN], sQi[PSCAN_BM], sQn[PSCAN_BM], sQt[PSCAN_BM];
    __shared__ int sItem[3];
    const PartSearchArgs& w = a.s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int srow = tid >> 2, sc = tid & 3;  // staging: image row, 16-byte chunk of the slice
    const int nks = a.pitch / 32;
    const int total = a.ibase[a.P];
    const uint32_t n = (uint32_t)w.n;
    const float nan = __int_as_float(0x7fc00000);
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        if (tid == 0) {
            int lo = 0, hi = a.P - 1;  // the last partition whose first item is <= item (empty ones own none)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (a.ibase[mid] <= item)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            const int nq = a.poff[lo + 1] - a.poff[lo];
            const int nqt = (nq + PSCAN_BM - 1) / PSCAN_BM, local = item - a.ibase[lo];
            sItem[0] = lo;
            sItem[1] = local % nqt;
            sItem[2] = local / nqt;
        }
        __syncthreads();
        const int p = sItem[0], qt = sItem[1], rt = sItem[2];
        if (tid < PSCAN_BN) {
            const uint32_t j = (uint32_t)w.off[p] + (uint32_t)rt * PSCAN_BN + tid;
            const uint32_t ub = min((uint32_t)w.off[p + 1], n);
            uint32_t id = j < ub ? w.sorted_id[j] : EMPTY_ID;
            if (!(id < n && id < w.g.capn && (int64_t)id < a.ldX) || is_dead(w.g, id)) id = EMPTY_ID;
            sRow[tid] = id;
            sXi[tid] = id != EMPTY_ID ? a.xinv[id] : 0.f;
            sXn[tid] = id != EMPTY_ID ? w.g.norms[id] : 0.f;
        } else if (tid < PSCAN_BN + PSCAN_BM) {
            const int i = tid - PSCAN_BN;
            const int e = a.poff[p] + qt * PSCAN_BM + i;
            uint32_t b = e < a.poff[p + 1] ? a.sval[e] : EMPTY_ID;
            if (!((int64_t)b < w.B)) b = EMPTY_ID;
            sQ[i] = b;
            sQi[i] = b != EMPTY_ID ? a.qinv[b] : 0.f;
            sQn[i] = b != EMPTY_ID ? a.qnorm[b] : 0.f;
            sQt[i] = b != EMPTY_ID ? a.thr[b] : nan;  // (no score is <= NaN)
        }
        __syncthreads();
        // chunk sc of a slice: K-block sc / 2 of the slice, half sc % 2 of its 32-byte run
        // (a row past the end reads row 0: its scores are dropped, no select between addresses)
        const uint32_t qb = sQ[srow], r0 = sRow[srow], r1 = sRow[srow + 64];
        const size_t ko = (size_t)(sc >> 1), ho = (size_t)(sc & 1) * 8;
        const uint16_t* const gq = a.Qh + (ko * a.ldQ + (qb != EMPTY_ID ? qb : 0u)) * 16 + ho;
        const uint16_t* const g0 = a.Xh + (ko * a.ldX + (r0 != EMPTY_ID ? r0 : 0u)) * 16 + ho;
        const uint16_t* const g1 = a.Xh + (ko * a.ldX + (r1 != EMPTY_ID ? r1 : 0u)) * 16 + ho;
        const size_t sq = (size_t)a.ldQ * 32, sx = (size_t)a.ldX * 32;  // halves per slice (two K-blocks)
        uint4 vq, v0, v1;
        auto gload = [&](int ks) {
            vq = *reinterpret_cast<const uint4*>(gq + ks * sq);
            v0 = *reinterpret_cast<const uint4*>(g0 + ks * sx);
            v1 = *reinterpret_cast<const uint4*>(g1 + ks * sx);
        };
        auto lstore = [&](int buf) {
            *reinterpret_cast<uint4*>(&sImg[buf][srow * PS_RB + sc * 16]) = vq;
            *reinterpret_cast<uint4*>(&sImg[buf][(PSCAN_BM + srow) * PS_RB + sc * 16]) = v0;
            *reinterpret_cast<uint4*>(&sImg[buf][(PSCAN_BM + 64 + srow) * PS_RB + sc * 16]) = v1;
        };
        ps_f32x4 acc[2][4];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = ps_f32x4{0.f, 0.f, 0.f, 0.f};
        gload(0);
        lstore(0);
        __syncthreads();
        for (int ks = 0; ks < nks; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < nks) gload(ks + 1);
            // fragment of a 16-row block: row lane & 15, halves 8 (lane / 16) .. of the slice
            ps_f16x8 fa[2], fb[4];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
                fa[mb] = *reinterpret_cast<const ps_f16x8*>(&sImg[cur][(wm * 32 + mb * 16 + fr) * PS_RB + fq * 16]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                fb[nb] = *reinterpret_cast<const ps_f16x8*>(&sImg[cur][(PSCAN_BM + wn * 64 + nb * 16 + fr) * PS_RB + fq * 16]);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[mb], fb[nb], acc[mb][nb], 0, 0, 0);
            if (ks + 1 < nks) lstore(cur ^ 1);
            __syncthreads();
        }
        // epilogue: accumulator r of block (mb, nb) is query wm 32 + 16 mb + 4 fq + r, row wn 64 + 16 nb + fr
        uint32_t rid[4];
        float xi[4], xn[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int ro = wn * 64 + nb * 16 + fr;
            rid[nb] = sRow[ro];
            xi[nb] = sXi[ro];
            xn[nb] = sXn[ro];
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qo = wm * 32 + mb * 16 + 4 * fq + r;
                const float t = sQt[qo], qi = sQi[qo], qn = sQn[qo];
                bool pass[4];
                unsigned long long any = 0ull;
                uint32_t seg[4];
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    const float score = split_score(RING_H1, w.g.metric, acc[mb][nb][r], xi[nb], qi, qn, xn[nb]);
                    pass[nb] = rid[nb] != EMPTY_ID && score <= t;
                    const unsigned long long m = __ballot(pass[nb]);
                    any |= m;
                    seg[nb] = (uint32_t)(m >> (16 * fq)) & 0xFFFFu;  // this query's 16 rows
                }
                if (!any) continue;  // (uniform)
                const uint32_t tot = __popc(seg[0]) + __popc(seg[1]) + __popc(seg[2]) + __popc(seg[3]);
                const uint32_t b = sQ[qo];
                uint32_t base = 0;
                if (tot && fr == 0) base = atomicAdd(a.scnt + b, tot);
                base = shfl_u(base, lane & 48);
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    const uint32_t slot = base + __popc(seg[nb] & ((1u << fr) - 1u));
                    if (pass[nb] && slot < (uint32_t)a.room) a.surv[(size_t)b * a.room + slot] = rid[nb];
                    base += __popc(seg[nb]);
                }
            }
        __syncthreads();  // (the next item rewrites the tile's tables and image)
    }
}

// The seed scan (part_scan_seed = 0): k_part_scan's tile body restated -- sharing it as one
// __device__ body moved k_part_scan's register count, so that kernel is left as it is -- over the
// items of the seed inversion, with another epilogue: the scores themselves, into the queries'
// score rows.
__global__ __launch_bounds__(256) void k_part_seed_scan(PartScanArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sImg[2][PS_IMG];
    __shared__ uint32_t sRow[PSCAN_BN];  // the tile's row ids (EMPTY_ID: past the end, dead)
    __shared__ uint32_t sQ[PSCAN_BM];    // its queries (EMPTY_ID past the end)
    __shared__ float sXi[PSCAN_BN], sXn[PSCAN_BN], sQi[PSCAN_BM], sQn[PSCAN_BM];
    __shared__ int sItem[3];
    const PartSearchArgs& w = a.s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int srow = tid >> 2, sc = tid & 3;  // staging: image row, 16-byte chunk of the slice
    const int nks = a.pitch / 32;
    const int total = a.ibase[a.P];
    const uint32_t n = (uint32_t)w.n;
    const float inf = __int_as_float(0x7f800000);
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        if (tid == 0) {
            int lo = 0, hi = a.P - 1;  // the last partition whose first item is <= item (empty ones own none)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (a.ibase[mid] <= item)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            const int nq = a.poff[lo + 1] - a.poff[lo];
            const int nqt = (nq + PSCAN_BM - 1) / PSCAN_BM, local = item - a.ibase[lo];
            sItem[0] = lo;
            sItem[1] = local % nqt;
            sItem[2] = local / nqt;
        }
        __syncthreads();
        const int p = sItem[0], qt = sItem[1], rt = sItem[2];
        if (tid < PSCAN_BN) {
            const uint32_t j = (uint32_t)w.off[p] + (uint32_t)rt * PSCAN_BN + tid;
            const uint32_t ub = min((uint32_t)w.off[p + 1], n);
            uint32_t id = j < ub ? w.sorted_id[j] : EMPTY_ID;
            if (!(id < n && id < w.g.capn && (int64_t)id < a.ldX) || is_dead(w.g, id)) id = EMPTY_ID;
            sRow[tid] = id;
            sXi[tid] = id != EMPTY_ID ? a.xinv[id] : 0.f;
            sXn[tid] = id != EMPTY_ID ? w.g.norms[id] : 0.f;
        } else if (tid < PSCAN_BN + PSCAN_BM) {
            const int i = tid - PSCAN_BN;
            const int e = a.poff[p] + qt * PSCAN_BM + i;
            uint32_t b = e < a.poff[p + 1] ? a.sval[e] : EMPTY_ID;
            if (!((int64_t)b < w.B)) b = EMPTY_ID;
            sQ[i] = b;
            sQi[i] = b != EMPTY_ID ? a.qinv[b] : 0.f;
            sQn[i] = b != EMPTY_ID ? a.qnorm[b] : 0.f;
        }
        __syncthreads();
        // chunk sc of a slice: K-block sc / 2 of the slice, half sc % 2 of its 32-byte run
        // (a row past the end reads row 0: its scores are dropped, no select between addresses)
        const uint32_t qb = sQ[srow], r0 = sRow[srow], r1 = sRow[srow + 64];
        const size_t ko = (size_t)(sc >> 1), ho = (size_t)(sc & 1) * 8;
        const uint16_t* const gq = a.Qh + (ko * a.ldQ + (qb != EMPTY_ID ? qb : 0u)) * 16 + ho;
        const uint16_t* const g0 = a.Xh + (ko * a.ldX + (r0 != EMPTY_ID ? r0 : 0u)) * 16 + ho;
        const uint16_t* const g1 = a.Xh + (ko * a.ldX + (r1 != EMPTY_ID ? r1 : 0u)) * 16 + ho;
        const size_t sq = (size_t)a.ldQ * 32, sx = (size_t)a.ldX * 32;  // halves per slice (two K-blocks)
        uint4 vq, v0, v1;
        auto gload = [&](int ks) {
            vq = *reinterpret_cast<const uint4*>(gq + ks * sq);
            v0 = *reinterpret_cast<const uint4*>(g0 + ks * sx);
            v1 = *reinterpret_cast<const uint4*>(g1 + ks * sx);
        };
        auto lstore = [&](int buf) {
            *reinterpret_cast<uint4*>(&sImg[buf][srow * PS_RB + sc * 16]) = vq;
            *reinterpret_cast<uint4*>(&sImg[buf][(PSCAN_BM + srow) * PS_RB + sc * 16]) = v0;
            *reinterpret_cast<uint4*>(&sImg[buf][(PSCAN_BM + 64 + srow) * PS_RB + sc * 16]) = v1;
        };
        ps_f32x4 acc[2][4];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = ps_f32x4{0.f, 0.f, 0.f, 0.f};
        gload(0);
        lstore(0);
        __syncthreads();
        for (int ks = 0; ks < nks; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < nks) gload(ks + 1);
            // fragment of a 16-row block: row lane & 15, halves 8 (lane / 16) .. of the slice
            ps_f16x8 fa[2], fb[4];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
                fa[mb] = *reinterpret_cast<const ps_f16x8*>(&sImg[cur][(wm * 32 + mb * 16 + fr) * PS_RB + fq * 16]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                fb[nb] = *reinterpret_cast<const ps_f16x8*>(&sImg[cur][(PSCAN_BM + wn * 64 + nb * 16 + fr) * PS_RB + fq * 16]);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[mb], fb[nb], acc[mb][nb], 0, 0, 0);
            if (ks + 1 < nks) lstore(cur ^ 1);
            __syncthreads();
        }
        // epilogue: accumulator r of block (mb, nb) is query wm 32 + 16 mb + 4 fq + r, row wn 64 + 16 nb + fr
        uint32_t rid[4];
        float xi[4], xn[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int ro = wn * 64 + nb * 16 + fr;
            rid[nb] = sRow[ro];
            xi[nb] = sXi[ro];
            xn[nb] = sXn[ro];
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qo = wm * 32 + mb * 16 + 4 * fq + r;
                const float qi = sQi[qo], qn = sQn[qo];
                // position rt 128 + row in tile of the query's nearest list; the 16 lanes of a
                // group hold 16 consecutive positions of one query: a 64-byte run per store
                const uint32_t b = sQ[qo];
                float* const out = a.sscore + (size_t)(b != EMPTY_ID ? b : 0u) * a.seed_room;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    const uint32_t pos = (uint32_t)rt * PSCAN_BN + wn * 64 + nb * 16 + fr;
                    float score = split_score(RING_H1, w.g.metric, acc[mb][nb][r], xi[nb], qi, qn, xn[nb]);
                    if (rid[nb] == EMPTY_ID) score = inf;  // (a NaN score is +inf already)
                    if (b != EMPTY_ID && pos < (uint32_t)a.seed_room) out[pos] = score;
                }
            }
        __syncthreads();  // (the next item rewrites the tile's tables and image)
    }
}

int launch_part_scan_tiles(const PartScanArgs& a, hipStream_t s) {
    if (a.pitch % 32 || a.room < 1) return -4;
    hipLaunchKernelGGL(k_part_scan, dim3(PS_GRID), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_part_scan_seed_tiles(const PartScanArgs& a, hipStream_t s) {
    if (a.pitch % 32 || !a.seed_pass || a.seed_room < 1 || !a.sscore) return -4;
    hipLaunchKernelGGL(k_part_seed_scan, dim3(PS_GRID), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the pick (part_scan_seed = 0) ----
// order-preserving image of a score's bits (wide.hip wide_ord; the seed scan writes no NaN)
__device__ __forceinline__ uint32_t ps_ord(float d) {
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
constexpr uint32_t PS_ORD_INF = 0xFF800000u;  // ps_ord(+inf)

// One wave per query: the k best of the m scores of its nearest list by (score, position) -- a
// radix select of the k-th image from the top byte down (k_wide_radius' pattern, on one wave),
// then one pass that takes every position below it and the first of those equal to it --, their
// rows evaluated canonically.  The largest of the k distances is a radius the true k-th distance
// over the probed rows cannot exceed; the certificate turns it into the threshold as the seed
// walk's k-th distance is.  The list the finish reloads is empty.
template <int LPR, int VPL, int G>
__global__ __launch_bounds__(64, 2) void k_ps_pick(PartScanArgs a) {
    using C = Cfg<LPR, VPL>;
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[256];
    const PartSearchArgs& w = a.s;
    const int64_t b = blockIdx.x;
    if (b >= w.B) return;
    const int lane = lane_id();
    const float inf = __int_as_float(0x7f800000);
    const unsigned long long below = (1ull << lane) - 1ull;
    float t = __int_as_float(0x7fc00000);
    uint32_t lo, m;
    bool ok = ps_seed_takes(a, b, lo, m) && m >= (uint32_t)w.k;  // (wave-uniform from here on)
    const float* __restrict__ row = a.sscore + (size_t)b * a.seed_room;
    uint32_t prefix = 0, mask = 0, want = (uint32_t)w.k;
    if (ok) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = lane; i < 256; i += 64) hist[i] = 0u;
            __syncthreads();
            for (uint32_t i0 = 0; i0 < m; i0 += 64) {
                const uint32_t i = i0 + lane;
                const uint32_t key = i < m ? ps_ord(row[i]) : 0u;
                const bool in = i < m && (key & mask) == prefix;
                const uint32_t bin = (key >> shift) & 255u;
                const unsigned long long act = __ballot(in);
                if (!act) continue;
                // the lanes that share the first lane's bin in one atomic (a list's scores
                // mostly share their top bytes)
                const uint32_t b0 = shfl_u(bin, __builtin_ctzll(act));
                const unsigned long long same = __ballot(in && bin == b0);
                if (in && bin != b0)
                    atomicAdd(&hist[bin], 1u);
                else if (in && (same & below) == 0ull)
                    atomicAdd(&hist[b0], (uint32_t)__popcll(same));
            }
            __syncthreads();
            const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const uint32_t sum = c0 + c1 + c2 + c3;
            uint32_t inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = (uint32_t)__shfl_up((int)inc, o, 64);
                if (lane >= o) inc += v;
            }
            uint32_t before = inc - sum, bin = 4 * lane;  // the bin that holds the rank, in one lane
            const bool mine = before < want && want <= inc;
            if (want > before + c0) before += c0, bin = 4 * lane + 1;
            if (bin == 4 * lane + 1 && want > before + c1) before += c1, bin = 4 * lane + 2;
            if (bin == 4 * lane + 2 && want > before + c2) before += c2, bin = 4 * lane + 3;
            const int src = __builtin_ctzll(__ballot(mine) | (1ull << 63));  // (m >= want: some lane holds it)
            prefix |= shfl_u(bin, src) << shift;
            mask |= 0xFFu << shift;
            want -= shfl_u(before, src);
            __syncthreads();
        }
        ok = prefix < PS_ORD_INF;  // the k-th score is +inf: fewer than k live rows with a score
    }
    if (ok) {
        // `want` is now the k-th's rank among the positions whose image equals `prefix`
        uint32_t nt = 0, ne = 0;
        for (uint32_t i0 = 0; i0 < m; i0 += 64) {
            const uint32_t i = i0 + lane;
            const uint32_t key = i < m ? ps_ord(row[i]) : 0xFFFFFFFFu;
            const bool eq = i < m && key == prefix;
            const unsigned long long em = __ballot(eq);
            const bool take = (i < m && key < prefix) || (eq && ne + (uint32_t)__popcll(em & below) < want);
            const unsigned long long tm = __ballot(take);
            const uint32_t slot = nt + (uint32_t)__popcll(tm & below);
            if (take && slot < 256u) sel[slot] = w.sorted_id[lo + i];
            nt += (uint32_t)__popcll(tm);
            ne += (uint32_t)__popcll(em);
        }
        __syncthreads();
        QReg<C> q;
        load_query(q, w.q + (size_t)b * C::PITCH);
        const float qn = query_norm(q);
        float wd = -inf;
        bool bad = nt != (uint32_t)w.k;
        for (int base = 0; base < w.k; base += 64) {
            const int cnt = min(64, w.k - base);
            const uint32_t cid = lane < cnt ? sel[base + lane] : EMPTY_ID;
            eval_list<C, G>(w.g, q, qn, cid, cnt, w.g.metric, [&](float d, uint32_t) {
                bad |= !(d < inf);  // NaN or +inf: no radius
                wd = fmaxf(wd, d);
            });
        }
        // (inclusive, as the seed walk's: a row at exactly wd is a row of the true list)
        if (!bad) t = cert_score_thr(w.g.metric, wd, a.qnorm[b], a.c);
        for (int idx = lane; idx < w.k; idx += 64) {
            a.seed_d[b * w.k + idx] = inf;
            a.seed_i[b * w.k + idx] = EMPTY_ID;
        }
    }
    if (lane == 0) {
        a.thr[b] = t;
        a.scnt[b] = 0u;
    }
}

int launch_part_scan_pick(const PartScanArgs& a, int lpr, int vpl, hipStream_t s) {
    const PartSearchArgs& w = a.s;
    if (w.B <= 0) return 0;
    if (w.k < 1 || w.k > 256 || w.nprobe < 1 || w.nprobe > PART_MAX_PROBE || a.seed != 0 || a.seed_room < 1 || !a.sscore)
        return -4;
    return with_cfg(lpr, vpl, [&](auto c) {
        constexpr int GS = c.G < 4 ? c.G : 4;  // (k_part_search's limit on the rows in flight)
        hipLaunchKernelGGL((k_ps_pick<c.L, c.V, GS>), dim3((unsigned)w.B), dim3(64), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

}  // namespace mh
