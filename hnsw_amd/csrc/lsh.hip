// lsh.hip -- the LSH index (hnsw-extensions/hybrid/lsh.go) on the device: random-projection
// sign codes, sorted bucket tables and the bucket search (DESIGN.md §6 "LSH index").
//
//  k_lsh_hash       : rows x projections sums on the f32-input MFMA (v_mfma_f32_32x32x2_f32),
//                     64 x 64 block tile, 4 waves of 32 x 32, operands staged through LDS in
//                     K-blocks of 32 (k_scores' layout).  The sums are never written: the
//                     epilogue ballots their signs into 32-projection words in LDS and packs b
//                     of them into each table's code.  A sum too close to 0 for the MFMA's
//                     summation order to decide goes to a worklist.
//  k_lsh_hash_canon : the worklist's (row, projection) pairs with the row engine in the
//                     canonical order (og_dev_sum), one wave per pair: sets or clears the
//                     bit.  A worklist that overflowed: every pair of the launch.
//  k_lsh_keys + rocPRIM radix_sort_pairs: per table the row ids sorted by (code, id).
//  k_lsh_search     : one wave per query -- per table the query's bucket by binary search,
//                     walked 64 ids at a time; deleted rows and rows already met in an earlier
//                     table dropped, the rest ranked by the canonical distance in a register
//                     list (fp16 screen against the list's worst entry once it is full).
#include <rocprim/device/device_radix_sort.hpp>

#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

typedef float lsh_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LBM = 64, LBN = 64, LBK = 32, LLD = LBK + 4;  // rows x projections x K-block; padded LDS rows
static_assert(LBN == LSH_PPAD_UNIT, "the projection matrix is padded to whole tiles");

__global__ __launch_bounds__(256) void k_lsh_hash(LshHashArgs a) {
    __shared__ __attribute__((aligned(16))) float sX[2][LBM * LLD];
    __shared__ __attribute__((aligned(16))) float sP[2][LBN * LLD];
    __shared__ uint32_t sBits[LBM][LSH_MAX_P / 32];  // [row][word]: sign of projection 32 word + bit
    __shared__ float sXn[LBM];
    __shared__ uint32_t sRow[LBM];  // the tile's row ids (EMPTY_ID past the end)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t pos0 = a.r0 + (int64_t)blockIdx.x * LBM;
    const int P = a.T * a.b;
    if (tid < LBM) {
        const int64_t pos = pos0 + tid;
        const bool ok = pos < a.r1;
        const uint32_t row = ok ? (a.ids ? a.ids[pos] : (uint32_t)pos) : EMPTY_ID;
        sRow[tid] = row;
        sXn[tid] = ok ? a.xnorm[row] : 0.f;
    }
    __syncthreads();
    // staging: per K-step each thread moves 2 float4 of the row tile and 2 of the projection tile
    // (512 float4 slots each: slot e = tid + 256 t is row e / 8, float4 e % 8)
    const int srow = tid >> 3, sc4 = (tid & 7) * 4;
    const uint32_t rid0 = sRow[srow], rid1 = sRow[srow + 32];
    const float* const x0 = a.X + (size_t)(rid0 != EMPTY_ID ? rid0 : 0u) * a.pitch + sc4;
    const float* const x1 = a.X + (size_t)(rid1 != EMPTY_ID ? rid1 : 0u) * a.pitch + sc4;
    float4 rx0, rx1, rp0, rp1;
    const int nk = a.pitch / LBK;
    const int nchunk = (P + LBN - 1) / LBN;
    for (int pc = 0; pc < nchunk; ++pc) {
        lsh_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // (the projection matrix holds whole tiles: rows past P are zero)
        const float* const p0 = a.P + (size_t)(pc * LBN + srow) * a.pitch + sc4;
        const float* const p1 = p0 + (size_t)32 * a.pitch;
        auto gload = [&](int k0) {
            // (a row past the end reads row 0 and is zeroed by value: no select between addresses)
            rx0 = *reinterpret_cast<const float4*>(x0 + k0);
            rx1 = *reinterpret_cast<const float4*>(x1 + k0);
            if (rid0 == EMPTY_ID) rx0.x = rx0.y = rx0.z = rx0.w = 0.f;
            if (rid1 == EMPTY_ID) rx1.x = rx1.y = rx1.z = rx1.w = 0.f;
            rp0 = *reinterpret_cast<const float4*>(p0 + k0);
            rp1 = *reinterpret_cast<const float4*>(p1 + k0);
        };
        auto lstore = [&](int buf) {
            *reinterpret_cast<float4*>(&sX[buf][srow * LLD + sc4]) = rx0;
            *reinterpret_cast<float4*>(&sX[buf][(srow + 32) * LLD + sc4]) = rx1;
            *reinterpret_cast<float4*>(&sP[buf][srow * LLD + sc4]) = rp0;
            *reinterpret_cast<float4*>(&sP[buf][(srow + 32) * LLD + sc4]) = rp1;
        };
        gload(0);
        lstore(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nk) gload((kt + 1) * LBK);
#pragma unroll
            for (int kb = 0; kb < LBK / 8; ++kb) {
                const float4 fa = *reinterpret_cast<const float4*>(&sX[cur][(wm * 32 + li) * LLD + kb * 8 + lh * 4]);
                const float4 fb = *reinterpret_cast<const float4*>(&sP[cur][(wn * 32 + li) * LLD + kb * 8 + lh * 4]);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc, 0, 0, 0);
            }
            if (kt + 1 < nk) lstore(cur ^ 1);
            __syncthreads();
        }
        // epilogue: D col = lane & 31 (projection), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
        // One ballot per r: its low word is the 32 signs of row rl, its high word of row rl + 4.
        const int p = pc * LBN + wn * 32 + li;
        const float mp = a.margin * a.pnorm[p], pn = a.pnorm[p];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = wm * 32 + (r & 3) + 8 * (r >> 2);
            const int rin = rl + 4 * lh;
            const float s = acc[r];
            const float xn = sXn[rin];
            // !(>): a NaN sum or bound is not trusted either
            const float thr = fmaf(mp, xn, fmaf(a.abs_rel, pn + xn, a.abs_min));
            const bool unc = !(fabsf(s) > thr) && p < P && sRow[rin] != EMPTY_ID;
            const unsigned long long mpos = __builtin_amdgcn_ballot_w64(s > 0.f);
            const unsigned long long munc = __builtin_amdgcn_ballot_w64(unc);
            if (lane == 0) sBits[rl][pc * 2 + wn] = (uint32_t)mpos;
            if (lane == 32) sBits[rl + 4][pc * 2 + wn] = (uint32_t)(mpos >> 32);
            if (munc) {
                const int first = __ffsll((long long)munc) - 1;
                uint32_t base = 0;
                if (lane == first) base = atomicAdd(a.work_cnt, (uint32_t)__popcll(munc));
                base = shfl_u(base, first);
                if (unc) {
                    const uint32_t e = base + (uint32_t)__builtin_amdgcn_mbcnt_hi(
                                                  (uint32_t)(munc >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)munc, 0));
                    if (e < (uint32_t)a.work_cap) a.work[e] = make_uint2(sRow[rin], (uint32_t)p);
                }
            }
        }
    }
    __syncthreads();
    // table t's code: bits [t b, t b + b) of the row's sign string (at most two words)
    const uint32_t mask = a.b == 32 ? 0xFFFFFFFFu : (1u << a.b) - 1u;
    for (int idx = tid; idx < LBM * a.T; idx += 256) {
        const int row = idx / a.T, t = idx - row * a.T;
        if (sRow[row] == EMPTY_ID) continue;
        const int bit0 = t * a.b, w = bit0 >> 5, sh = bit0 & 31;
        uint32_t v = sBits[row][w] >> sh;
        if (sh + a.b > 32) v |= sBits[row][w + 1] << (32 - sh);
        a.codes[(size_t)sRow[row] * a.T + t] = v & mask;
    }
}

// the canonical sign of one (row, projection) pair into its bit
__device__ __forceinline__ void lsh_put_bit(const LshHashArgs& a, uint32_t row, int p, float s) {
    const int t = p / a.b, i = p - t * a.b;
    uint32_t* w = a.codes + (size_t)row * a.T + t;
    if (s > 0.f)
        atomicOr(w, 1u << i);
    else
        atomicAnd(w, ~(1u << i));
}

// The row is the engine's "query" and the projections its "rows": a product commutes, so the
// sum is og_dev_sum(x, p, d, 0) term for term.
template <class C>
__global__ __launch_bounds__(256) void k_lsh_hash_canon(LshHashArgs a) {
    const int lane = lane_id();
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const uint32_t cnt = *a.work_cnt;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.stat) atomicAdd(a.stat, (unsigned long long)cnt);
    const int P = a.T * a.b;
    if (cnt <= (uint32_t)a.work_cap) {
        for (int64_t e = gw; e < (int64_t)cnt; e += nw) {
            const uint2 pr = a.work[e];
            QReg<C> x;
            load_query(x, a.X + (size_t)pr.x * a.pitch);
            const uint32_t ids[1] = {pr.y};
            const bool valid[1] = {lane < C::LPR};
            const float s = eval_rows<C, 1, false>(x, a.P, a.pitch, ids, valid);
            if (lane == 0) lsh_put_bit(a, pr.x, (int)pr.y, s);
        }
        return;
    }
    // the worklist overflowed: every pair of the launch, RPI projections of a row per step
    for (int64_t pos = a.r0 + gw; pos < a.r1; pos += nw) {
        const uint32_t row = a.ids ? a.ids[pos] : (uint32_t)pos;
        QReg<C> x;
        load_query(x, a.X + (size_t)row * a.pitch);
        for (int p0 = 0; p0 < P; p0 += C::RPI) {
            const int p = p0 + lane / C::LPR;
            const uint32_t ids[1] = {(uint32_t)(p < P ? p : 0)};
            const bool valid[1] = {p < P};
            const float s = eval_rows<C, 1, false>(x, a.P, a.pitch, ids, valid);
            if (p < P && (lane & (C::LPR - 1)) == 0) lsh_put_bit(a, row, p, s);
        }
    }
}

__global__ void k_lsh_zero(uint32_t* p) { *p = 0u; }

int launch_lsh_hash(const LshHashArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.r1 <= a.r0) return 0;
    const int P = a.T * a.b;
    if (a.T < 1 || a.T > 32 || a.b < 1 || a.b > 32 || P > LSH_MAX_P || a.pitch % LBK || a.work_cap < 0) return -4;
    hipLaunchKernelGGL(k_lsh_zero, dim3(1), dim3(1), 0, s, a.work_cnt);  // (a kernel: the launch may be captured)
    hipLaunchKernelGGL(k_lsh_hash, dim3((unsigned)((a.r1 - a.r0 + LBM - 1) / LBM)), dim3(256), 0, s, a);
    return with_cfg(lpr, vpl, [&](auto c) {
        const int64_t rows = a.r1 - a.r0;
        const int grid = (int)std::min<int64_t>(std::max<int64_t>((rows + 3) / 4, 1), 1024);
        hipLaunchKernelGGL((k_lsh_hash_canon<Cfg<c.L, c.V>>), dim3(grid), dim3(256), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

// ---- tables: per table the row ids by (code, id) ----
__global__ void k_lsh_keys(const uint32_t* __restrict__ codes, int T, int t, int64_t n, uint32_t* __restrict__ key,
                           uint32_t* __restrict__ val) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        key[i] = codes[(size_t)i * T + t];
        val[i] = (uint32_t)i;
    }
}

int lsh_sort_temp_bytes(int64_t n, size_t* bytes) {
    *bytes = 0;
    const hipError_t e =
        rocprim::radix_sort_pairs(nullptr, *bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)n, 0u, 32u, (hipStream_t) nullptr);
    return e == hipSuccess ? 0 : -1;
}

// the radix sort is stable and the ids go in ascending: equal codes keep the id order
int launch_lsh_table(const uint32_t* codes, int T, int t, int bits, int64_t n, uint32_t* key, uint32_t* val,
                     uint32_t* sorted_code, uint32_t* sorted_id, void* temp, size_t temp_bytes, hipStream_t s) {
    if (n <= 0) return 0;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_lsh_keys, dim3(grid), dim3(256), 0, s, codes, T, t, n, key, val);
    const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, key, sorted_code + (size_t)t * n, val,
                                                   sorted_id + (size_t)t * n, (size_t)n, 0u, (unsigned)bits, s);
    return e == hipSuccess && hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- search ----
template <int LPR, int VPL, int R, int G, bool SCREEN>
__global__ __launch_bounds__(64, 2) void k_lsh_search(LshSearchArgs a) {
    using C = Cfg<LPR, VPL>;
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;
    const int lane = lane_id();
    const float inf = __int_as_float(0x7f800000);
    QReg<C> q;
    load_query(q, a.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    const bool screen = SCREEN && a.g.h16 && h16_query_ok(qn);
    float margin = 0.f;
    if constexpr (SCREEN) {
        const float e = a.g.h16err ? *a.g.h16err : 0.00048828125f;
        margin = (a.g.metric == EUCLIDEAN ? h16_margin_l2(e) : h16_margin_cos(e)) + MH_SCREEN_PAD;
    }
    BList<R> L;
    bl_init(L);
    int ncand = 0;
    unsigned long long s16 = 0;
    const uint32_t* qc = a.qcodes + (size_t)b * a.T;
    const uint32_t n = (uint32_t)a.n;  // (row ids are below 2^31)
    auto sink = [&](float d, uint32_t u) { bl_insert(L, a.k, d, u); };
    for (int t = 0; t < a.T; ++t) {
        const uint32_t code = qc[t];
        const uint32_t* sc = a.sorted_code + (size_t)t * n;
        uint32_t lo = 0, hi = n;  // the bucket [lo, ub): the first code >= and the first code > the query's
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sc[mid] < code)
                lo = mid + 1;
            else
                hi = mid;
        }
        uint32_t ub = lo;
        hi = n;
        while (ub < hi) {
            const uint32_t mid = (ub + hi) >> 1;
            if (sc[mid] <= code)
                ub = mid + 1;
            else
                hi = mid;
        }
        const uint32_t* si = a.sorted_id + (size_t)t * n;
        for (uint32_t j0 = lo; j0 < ub; j0 += 64) {
            const uint32_t j = j0 + lane;
            const uint32_t id = j < ub ? si[j] : EMPTY_ID;
            bool keep = j < ub && id < n && id < a.g.capn && !is_dead(a.g, id);
            if (keep) {  // met in an earlier table: that table's bucket held it
                const uint32_t* rc = a.codes + (size_t)id * a.T;
                for (int tp = 0; tp < t; ++tp) keep = keep && rc[tp] != qc[tp];
            }
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
    int nv = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int idx = r * 64 + lane;
        const bool okr = idx < a.k && L.i[r] != EMPTY_ID;
        if (idx < a.k) {
            const uint32_t id = L.i[r] & ID_MASK;
            a.out_keys[b * a.k + idx] = okr ? a.g.keys[id] : (int64_t)-1;
            a.out_dist[b * a.k + idx] = okr ? L.d[r] : inf;
        }
        nv += __popcll(__ballot(okr));
    }
    if (lane == 0) {
        a.out_n[b] = nv;
        a.out_ncand[b] = ncand;
        if (a.stat) atomicAdd(a.stat, (unsigned long long)ncand);
    }
}

template <int L_, int V_, int G_, int R>
static int launch_lsh_search_r(const LshSearchArgs& a, hipStream_t s) {
    if (a.g.h16)
        hipLaunchKernelGGL((k_lsh_search<L_, V_, R, G_, true>), dim3((unsigned)a.B), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((k_lsh_search<L_, V_, R, G_, false>), dim3((unsigned)a.B), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_lsh_search(const LshSearchArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.B <= 0) return 0;
    if (a.k < 1 || a.k > 256 || a.T < 1 || a.T > 32) return -4;
    return with_cfg(lpr, vpl, [&](auto c) {
        // at most 4 rows in flight (8 through the screen): the table's 8 keeps 16 uniform row
        // addresses live in the screen, more scalar registers than the kernel has
        constexpr int GS = c.G < 4 ? c.G : 4;
        if (a.k <= 64) return launch_lsh_search_r<c.L, c.V, GS, 1>(a, s);
        if (a.k <= 128) return launch_lsh_search_r<c.L, c.V, GS, 2>(a, s);
        return launch_lsh_search_r<c.L, c.V, GS, 4>(a, s);
    });
}

}  // namespace mh
