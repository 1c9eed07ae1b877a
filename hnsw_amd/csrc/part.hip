// part.hip -- the partitioner (hnsw-extensions/hybrid/partitioner.go) on the device: nearest-
// centroid assignment, the centroid update, the partitions' id lists and the probed search
// (DESIGN.md §6 "Partitions").  The reference's hybrid index never searches its partitions
// (hybrid.go:266-267, "Use the partition index in the future"): k_part_search is that future.
//
//  k_part_assign       : rows x centroids dots on the f32-input MFMA (v_mfma_f32_32x32x2_f32),
//                        64 x 64 block tile, 4 waves of 32 x 32, operands staged through LDS in
//                        double-buffered K-blocks of 32 (k_lsh_hash's layout), looping over the
//                        centroid tiles.  The dots are never written: the epilogue forms, per
//                        (row, centroid), an approximate distance and the interval that holds
//                        the canonical one, and keeps per row the lowest upper end with its
//                        index and the lowest lower end among the others.  A row whose best
//                        upper end is below every other lower end writes its partition; every
//                        other row (ties, near ties, NaN or infinite values, zero rows under
//                        cosine) goes to a worklist.
//  k_part_assign_canon : the worklist's rows, one wave each: all P centroids with the row
//                        engine in the canonical order, minimum by (distance, index).  A
//                        worklist that overflowed: every row of the launch.
//  k_part_probe        : the same scan keeping the m nearest in a register list (the probe
//                        order of mhnsw_part_assign and of the search's queries).
//  k_part_keys + rocPRIM radix_sort_pairs + k_part_offsets: the row ids by (partition, id).
//  k_part_sum / k_part_mean: the centroid update, f64 partials per (partition, 256 entries).
//  k_part_search       : one wave per query -- the probed partitions' lists walked 64 ids at a
//                        time, deleted rows dropped, the rest ranked by the canonical distance
//                        in a register list (fp16 screen against its worst entry once full).
#include <rocprim/device/device_radix_sort.hpp>

#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

typedef float part_f32x16 __attribute__((ext_vector_type(16)));

constexpr int PBM = 64, PBN = 64, PBK = 32, PLD = PBK + 4;  // rows x centroids x K-block; padded LDS rows
static_assert(PBN == PART_PAD_UNIT, "the centroid matrix is padded to whole tiles");

// part[row] = p; Rebalance counts the live rows that moved
__device__ __forceinline__ void part_put(const PartAssignArgs& a, uint32_t row, int p) {
    const int old = a.part[row];
    a.part[row] = p;
    if (a.moved && old != p && !(a.dead && a.dead[row])) atomicAdd(a.moved, 1ull);
}

__global__ __launch_bounds__(256) void k_part_assign(PartAssignArgs a) {
    __shared__ __attribute__((aligned(16))) float sX[2][PBM * PLD];
    __shared__ __attribute__((aligned(16))) float sC[2][PBN * PLD];
    __shared__ float sXn[PBM];
    __shared__ uint32_t sRow[PBM];  // the tile's row ids (EMPTY_ID past the end)
    __shared__ float4 sSt[2][PBM];  // per centroid half: {best upper end, its lower end, lowest other lower end, index}
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t pos0 = a.r0 + (int64_t)blockIdx.x * PBM;
    const float inf = __int_as_float(0x7f800000);
    if (tid < PBM) {
        const int64_t pos = pos0 + tid;
        const bool ok = pos < a.r1;
        const uint32_t row = ok ? (a.ids ? a.ids[pos] : (uint32_t)pos) : EMPTY_ID;
        sRow[tid] = row;
        sXn[tid] = ok ? a.xnorm[row] : 0.f;
    }
    __syncthreads();
    // staging: per K-step each thread moves 2 float4 of the row tile and 2 of the centroid tile
    // (512 float4 slots each: slot e = tid + 256 t is row e / 8, float4 e % 8)
    const int srow = tid >> 3, sc4 = (tid & 7) * 4;
    const uint32_t rid0 = sRow[srow], rid1 = sRow[srow + 32];
    const float* const x0 = a.X + (size_t)(rid0 != EMPTY_ID ? rid0 : 0u) * a.pitch + sc4;
    const float* const x1 = a.X + (size_t)(rid1 != EMPTY_ID ? rid1 : 0u) * a.pitch + sc4;
    float4 rx0, rx1, rc0, rc1;
    const int nk = a.pitch / PBK;
    const int ntile = (a.P + PBN - 1) / PBN;
    // per lane and accumulator row, over the centroids wn * 32 + li of every tile
    float hi1[16], lo1[16], lo2[16];
    int idx[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        hi1[r] = lo1[r] = lo2[r] = inf;
        idx[r] = 0;
    }
    for (int pc = 0; pc < ntile; ++pc) {
        part_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // (the centroid matrix holds whole tiles: rows past P are zero)
        const float* const c0 = a.Cn + (size_t)(pc * PBN + srow) * a.pitch + sc4;
        const float* const c1 = c0 + (size_t)32 * a.pitch;
        auto gload = [&](int k0) {
            // (a row past the end reads row 0 and is zeroed by value: no select between addresses)
            rx0 = *reinterpret_cast<const float4*>(x0 + k0);
            rx1 = *reinterpret_cast<const float4*>(x1 + k0);
            if (rid0 == EMPTY_ID) rx0.x = rx0.y = rx0.z = rx0.w = 0.f;
            if (rid1 == EMPTY_ID) rx1.x = rx1.y = rx1.z = rx1.w = 0.f;
            rc0 = *reinterpret_cast<const float4*>(c0 + k0);
            rc1 = *reinterpret_cast<const float4*>(c1 + k0);
        };
        auto lstore = [&](int buf) {
            *reinterpret_cast<float4*>(&sX[buf][srow * PLD + sc4]) = rx0;
            *reinterpret_cast<float4*>(&sX[buf][(srow + 32) * PLD + sc4]) = rx1;
            *reinterpret_cast<float4*>(&sC[buf][srow * PLD + sc4]) = rc0;
            *reinterpret_cast<float4*>(&sC[buf][(srow + 32) * PLD + sc4]) = rc1;
        };
        gload(0);
        lstore(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nk) gload((kt + 1) * PBK);
#pragma unroll
            for (int kb = 0; kb < PBK / 8; ++kb) {
                const float4 fa = *reinterpret_cast<const float4*>(&sX[cur][(wm * 32 + li) * PLD + kb * 8 + lh * 4]);
                const float4 fb = *reinterpret_cast<const float4*>(&sC[cur][(wn * 32 + li) * PLD + kb * 8 + lh * 4]);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc, 0, 0, 0);
            }
            if (kt + 1 < nk) lstore(cur ^ 1);
            __syncthreads();
        }
        // epilogue: D col = lane & 31 (centroid), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const int p = pc * PBN + wn * 32 + li;
        const float cn = a.cnorm[p];
        const bool real = p < a.P;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float xn = sXn[wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
            const float s = acc[r];
            float hi, lo;
            bool ok;  // (every test is false on a NaN)
            if (a.metric == EUCLIDEAN) {
                const float w = fmaf(xn, xn, cn * cn);
                const float A = fmaf(-2.f, s, w), E = fmaf(a.e_rel, w, a.e_abs);
                hi = (A + E) * (1.f + a.e_mul);
                lo = (A - E) * (1.f - a.e_mul);
                ok = hi < inf && lo > -inf;
            } else {
                const float den = xn * cn;
                const float A = 1.f - s / den;
                hi = A + a.e_abs;
                lo = A - a.e_abs;
                ok = den >= a.den_min && den < inf && hi < inf && lo > -inf;
            }
            if (!ok) hi = inf, lo = -inf;  // never the certain best, and nothing is certain beside it
            if (!real) hi = lo = inf;
            if (hi < hi1[r]) {
                lo2[r] = fminf(lo2[r], lo1[r]);
                hi1[r] = hi;
                lo1[r] = lo;
                idx[r] = p;
            } else {
                lo2[r] = fminf(lo2[r], lo);
            }
        }
    }
    // over the 32 lanes of a row, then over the two centroid halves through LDS
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const float ohi = __shfl_xor(hi1[r], o, 64), olo1 = __shfl_xor(lo1[r], o, 64);
            const float olo2 = __shfl_xor(lo2[r], o, 64);
            const int oidx = __shfl_xor(idx[r], o, 64);
            const bool mine = hi1[r] < ohi || (hi1[r] == ohi && idx[r] < oidx);
            lo2[r] = fminf(fminf(lo2[r], olo2), mine ? olo1 : lo1[r]);
            if (!mine) {
                hi1[r] = ohi;
                lo1[r] = olo1;
                idx[r] = oidx;
            }
        }
        if (li == 0)
            sSt[wn][wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = make_float4(hi1[r], lo1[r], lo2[r], __int_as_float(idx[r]));
    }
    __syncthreads();
    if (tid >= PBM) return;
    const float4 s0 = sSt[0][tid], s1 = sSt[1][tid];  // (half 0 holds the lower indices of a tile, not of all)
    const int i0 = __float_as_int(s0.w), i1 = __float_as_int(s1.w);
    const bool first = s0.x < s1.x || (s0.x == s1.x && i0 < i1);
    const float bhi = first ? s0.x : s1.x;
    const float olo = fminf(fminf(s0.z, s1.z), first ? s1.y : s0.y);
    const int best = first ? i0 : i1;
    const uint32_t row = sRow[tid];
    const bool live = row != EMPTY_ID;
    const bool certain = bhi < olo && !a.force;
    if (live && certain) part_put(a, row, best);
    const bool unc = live && !certain;
    const unsigned long long munc = __builtin_amdgcn_ballot_w64(unc);
    if (munc) {
        const int firstl = __ffsll((long long)munc) - 1;
        uint32_t base = 0;
        if (lane == firstl) base = atomicAdd(a.work_cnt, (uint32_t)__popcll(munc));
        base = shfl_u(base, firstl);
        if (unc) {
            const uint32_t e = base + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(munc >> 32),
                                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)munc, 0));
            if (e < (uint32_t)a.work_cap) a.work[e] = (uint32_t)(pos0 + tid - a.r0);
        }
    }
}

// the centroids as the row engine's store: the vector is its "query" (a distance commutes term
// for term: (x - c)^2 = (c - x)^2, x c = c x, |x| |c| = |c| |x|)
__device__ __forceinline__ GraphDev part_view(const float* Cn, const float* cnorm, int pitch, int P) {
    GraphDev g = {};
    g.vecs = Cn;
    g.norms = cnorm;
    g.pitch = pitch;
    g.capn = (uint32_t)P;
    return g;
}

// sink(distance, centroid) for the P centroids in ascending index, uniformly
template <class C, int G, class Sink>
__device__ __forceinline__ void part_scan(const GraphDev& g, const QReg<C>& x, float xn, int P, int metric, Sink&& sink) {
    const int lane = lane_id();
    for (int p0 = 0; p0 < P; p0 += 64) {
        const int cnt = min(64, P - p0);
        eval_list<C, G>(g, x, xn, (uint32_t)(p0 + (lane < cnt ? lane : 0)), cnt, metric, sink);
    }
}

template <class C, int G>
__global__ __launch_bounds__(256) void k_part_assign_canon(PartAssignArgs a) {
    const int lane = lane_id();
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const uint32_t cnt = *a.work_cnt;
    const bool all = cnt > (uint32_t)a.work_cap;  // the worklist overflowed: every row of the launch
    const int64_t m = all ? a.r1 - a.r0 : (int64_t)cnt;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.stat) atomicAdd(a.stat, (unsigned long long)cnt);
    const GraphDev g = part_view(a.Cn, a.cnorm, a.pitch, a.P);
    for (int64_t e = gw; e < m; e += nw) {
        const int64_t pos = a.r0 + (all ? e : (int64_t)a.work[e]);
        const uint32_t row = a.ids ? a.ids[pos] : (uint32_t)pos;
        QReg<C> x;
        load_query(x, a.X + (size_t)row * a.pitch);
        const float xn = query_norm(x);
        bool have = false;
        float bd = 0.f;
        uint32_t bi = 0;  // (every distance NaN: partition 0)
        part_scan<C, G>(g, x, xn, a.P, a.metric, [&](float d, uint32_t u) {
            if (d == d && (!have || d < bd)) bd = d, bi = u, have = true;
        });
        if (lane == 0) part_put(a, row, (int)bi);
    }
}

struct PartProbeArgs {
    const float* X;
    int64_t n;
    int pitch, metric;
    const float* Cn;
    const float* cnorm;
    int P, m;
    int32_t* out;
};

template <class C, int G, int R>
__global__ __launch_bounds__(256) void k_part_probe(PartProbeArgs a) {
    const int lane = lane_id();
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const GraphDev g = part_view(a.Cn, a.cnorm, a.pitch, a.P);
    for (int64_t j = gw; j < a.n; j += nw) {
        QReg<C> x;
        load_query(x, a.X + (size_t)j * a.pitch);
        const float xn = query_norm(x);
        BList<R> L;
        bl_init(L);
        int fin = 0;  // centroids at a distance that is a number
        part_scan<C, G>(g, x, xn, a.P, a.metric, [&](float d, uint32_t u) {
            bl_insert(L, a.m, d, u);
            fin += d == d ? 1 : 0;
        });
        if (fin < a.m) {  // the NaN distances follow, by index
            int at = fin;
            part_scan<C, G>(g, x, xn, a.P, a.metric, [&](float d, uint32_t u) {
                if (d == d || at >= a.m) return;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r * 64 + lane == at) L.i[r] = u;
                ++at;
            });
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r * 64 + lane < a.m) a.out[j * a.m + r * 64 + lane] = (int32_t)(L.i[r] & ID_MASK);
    }
}

__global__ void k_part_zero(uint32_t* p) { *p = 0u; }

int launch_part_assign(const PartAssignArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.r1 <= a.r0) return 0;
    if (a.P < 1 || a.P > PART_MAX_P || a.pitch % PBK || a.work_cap < 0) return -4;
    hipLaunchKernelGGL(k_part_zero, dim3(1), dim3(1), 0, s, a.work_cnt);  // (a kernel: the launch may be captured)
    hipLaunchKernelGGL(k_part_assign, dim3((unsigned)((a.r1 - a.r0 + PBM - 1) / PBM)), dim3(256), 0, s, a);
    return with_cfg(lpr, vpl, [&](auto c) {
        const int64_t rows = a.r1 - a.r0;
        const int grid = (int)std::min<int64_t>(std::max<int64_t>((rows + 3) / 4, 1), 2048);
        hipLaunchKernelGGL((k_part_assign_canon<Cfg<c.L, c.V>, c.G>), dim3(grid), dim3(256), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

int launch_part_probe(const float* X, int64_t n, int pitch, int metric, const float* Cn, const float* cnorm, int P, int m,
                      int32_t* out, int lpr, int vpl, hipStream_t s) {
    if (n <= 0) return 0;
    if (P < 1 || P > PART_MAX_P || m < 1 || m > P || m > PART_MAX_PROBE) return -4;
    const PartProbeArgs a{X, n, pitch, metric, Cn, cnorm, P, m, out};
    const int grid = (int)std::min<int64_t>((n + 3) / 4, 4096);
    return with_cfg(lpr, vpl, [&](auto c) {
        using CC = Cfg<c.L, c.V>;
        if (m <= 64)
            hipLaunchKernelGGL((k_part_probe<CC, c.G, 1>), dim3(grid), dim3(256), 0, s, a);
        else if (m <= 128)
            hipLaunchKernelGGL((k_part_probe<CC, c.G, 2>), dim3(grid), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((k_part_probe<CC, c.G, 4>), dim3(grid), dim3(256), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

// ---- lists: the row ids by (partition, id), the deleted rows behind partition P - 1 ----
__global__ void k_part_keys(const int32_t* __restrict__ part, const uint8_t* __restrict__ dead, int P, int64_t n,
                            uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t p = (uint32_t)part[i];
        key[i] = (dead && dead[i]) || p >= (uint32_t)P ? (uint32_t)P : p;
        val[i] = (uint32_t)i;
    }
}

// off[t] = the first entry with a key >= t, t in [0, P + 1]
__global__ void k_part_offsets(const uint32_t* __restrict__ skey, int64_t n, int P, int32_t* __restrict__ off) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > P + 1) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skey[mid] < (uint32_t)t)
            lo = mid + 1;
        else
            hi = mid;
    }
    off[t] = (int32_t)lo;
}

int part_sort_temp_bytes(int64_t n, size_t* bytes) {
    *bytes = 0;
    const hipError_t e =
        rocprim::radix_sort_pairs(nullptr, *bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)n, 0u, 32u, (hipStream_t) nullptr);
    return e == hipSuccess ? 0 : -1;
}

// the radix sort is stable and the ids go in ascending: equal partitions keep the id order
int launch_part_lists(const int32_t* part, const uint8_t* dead, int P, int64_t n, uint32_t* key, uint32_t* val,
                      uint32_t* sorted_key, uint32_t* sorted_id, int32_t* off, void* temp, size_t temp_bytes, hipStream_t s) {
    if (n <= 0) return 0;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_part_keys, dim3(grid), dim3(256), 0, s, part, dead, P, n, key, val);
    int bits = 1;
    while ((1 << bits) <= P) ++bits;  // keys in [0, P]
    const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, key, sorted_key, val, sorted_id, (size_t)n, 0u,
                                                   (unsigned)bits, s);
    if (e != hipSuccess) return -1;
    hipLaunchKernelGGL(k_part_offsets, dim3((P + 2 + 255) / 256), dim3(256), 0, s, sorted_key, n, P, off);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

__global__ void k_part_stats(const int32_t* __restrict__ part, const uint8_t* __restrict__ dead, int64_t n, int P,
                             unsigned long long* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t p = (uint32_t)part[i];
        if (!(dead && dead[i]) && p < (uint32_t)P) atomicAdd(out + p, 1ull);
    }
}

int launch_part_stats(const int32_t* part, const uint8_t* dead, int64_t n, int P, unsigned long long* out, hipStream_t s) {
    if (n <= 0) return 0;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_part_stats, dim3(grid), dim3(256), 0, s, part, dead, n, P, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- centroid update ----
// One workgroup per (partition, chunk of PART_CHUNK list entries), threads across the dimension:
// the chunk's rows in list order (ascending row id), each element summed sequentially in f64.
__global__ __launch_bounds__(256) void k_part_sum(const float* __restrict__ X, int pitch,
                                                  const uint32_t* __restrict__ sorted_id, const int32_t* __restrict__ off,
                                                  const int32_t* __restrict__ cbase, int P, double* __restrict__ partial) {
    __shared__ uint32_t sId[PART_CHUNK];
    const int c = blockIdx.x, tid = threadIdx.x;
    int lo = 0, hi = P;  // the last partition whose first chunk is <= c (empty partitions own no chunk)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cbase[mid] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int p = lo;
    const int j0 = off[p] + (c - cbase[p]) * PART_CHUNK;
    const int cnt = min(PART_CHUNK, off[p + 1] - j0);
    static_assert(PART_CHUNK == 256, "one list entry per thread");
    if (tid < cnt) sId[tid] = sorted_id[j0 + tid];
    __syncthreads();
    for (int e = tid; e < pitch; e += 256) {
        double acc = 0.0;
        for (int j = 0; j < cnt; ++j) acc += (double)X[(size_t)sId[j] * pitch + e];
        partial[(size_t)c * pitch + e] = acc;
    }
}

// the partials in ascending chunk order; a partition without a live row keeps its centroid
__global__ __launch_bounds__(256) void k_part_mean(const double* __restrict__ partial, int pitch,
                                                   const int32_t* __restrict__ off, const int32_t* __restrict__ cbase,
                                                   float* __restrict__ Cn) {
    const int p = blockIdx.x;
    const int cnt = off[p + 1] - off[p];
    if (cnt <= 0) return;
    for (int e = threadIdx.x; e < pitch; e += 256) {
        double acc = 0.0;
        for (int c = cbase[p]; c < cbase[p + 1]; ++c) acc += partial[(size_t)c * pitch + e];
        Cn[(size_t)p * pitch + e] = (float)(acc / (double)cnt);
    }
}

int launch_part_update(const float* X, int pitch, const uint32_t* sorted_id, const int32_t* off, const int32_t* cbase,
                       int P, int chunks, double* partial, float* Cn, hipStream_t s) {
    if (chunks <= 0) return 0;
    hipLaunchKernelGGL(k_part_sum, dim3((unsigned)chunks), dim3(256), 0, s, X, pitch, sorted_id, off, cbase, P, partial);
    hipLaunchKernelGGL(k_part_mean, dim3((unsigned)P), dim3(256), 0, s, partial, pitch, off, cbase, Cn);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- search ----
// (k_lsh_search's ranking body, restated: that kernel is left as it is.  A row lies in one
// partition, so nothing is met twice.)
template <int LPR, int VPL, int R, int G, bool SCREEN>
__global__ __launch_bounds__(64, 2) void k_part_search(PartSearchArgs a) {
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
    const uint32_t n = (uint32_t)a.n;  // (row ids are below 2^31)
    auto sink = [&](float d, uint32_t u) { bl_insert(L, a.k, d, u); };
    for (int t = 0; t < a.nprobe; ++t) {
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
static int launch_part_search_r(const PartSearchArgs& a, hipStream_t s) {
    if (a.g.h16)
        hipLaunchKernelGGL((k_part_search<L_, V_, R, G_, true>), dim3((unsigned)a.B), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((k_part_search<L_, V_, R, G_, false>), dim3((unsigned)a.B), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_part_search(const PartSearchArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.B <= 0) return 0;
    if (a.k < 1 || a.k > 256 || a.nprobe < 1 || a.nprobe > PART_MAX_PROBE) return -4;
    return with_cfg(lpr, vpl, [&](auto c) {
        constexpr int GS = c.G < 4 ? c.G : 4;  // (k_lsh_search's limit on the rows in flight)
        if (a.k <= 64) return launch_part_search_r<c.L, c.V, GS, 1>(a, s);
        if (a.k <= 128) return launch_part_search_r<c.L, c.V, GS, 2>(a, s);
        return launch_part_search_r<c.L, c.V, GS, 4>(a, s);
    });
}

}  // namespace mh
