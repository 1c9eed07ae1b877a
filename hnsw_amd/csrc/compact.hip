// compact.hip -- mhnsw_compact's device work (api.cpp): the deleted rows leave the store in
// place.  The map (new id of every row, -1 for a deleted one, and its inverse, the ascending
// list of the live rows) comes from the `dead` bytes by a rank per row and a prefix over
// blocks; rows move as gathers through the list, into their destination or into a staging
// buffer (the host decides which, chunk by chunk: api.cpp mhnsw_compact); every adjacency id
// then goes through the map, and the filter bitmaps are repacked to the new row numbers.
// Bandwidth kernels: every byte of a moved row is read once and written once (measured
// rates: DESIGN.md §6 "Compaction").
#include <algorithm>

#include "block_scan.hpp"
#include "engine.hpp"

namespace mh {

// Pass 1: live rows per block of 256 rows.
__global__ __launch_bounds__(256) void k_compact_count(const uint8_t* __restrict__ dead, int64_t n,
                                                       uint32_t* __restrict__ block_cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t total;
    (void)rs_block_scan(i < n && !dead[i] ? 1u : 0u, total);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// Pass 2, one block: the exclusive prefix of the per-block counts, in place.
__global__ __launch_bounds__(256) void k_compact_offsets(uint32_t* __restrict__ block_cnt, int64_t nblocks) {
    rs_offsets_inplace(block_cnt, nblocks);
}

// Pass 3: newid[i] = live rows below i (-1: i is deleted), src[newid[i]] = i.
__global__ __launch_bounds__(256) void k_compact_map(const uint8_t* __restrict__ dead, int64_t n,
                                                     const uint32_t* __restrict__ block_off,
                                                     int32_t* __restrict__ newid, uint32_t* __restrict__ src) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n && !dead[i];
    uint32_t total;
    const uint32_t pos = block_off[blockIdx.x] + rs_block_scan(live ? 1u : 0u, total);
    if (i < n) newid[i] = live ? (int32_t)pos : -1;
    if (live) src[pos] = (uint32_t)i;  // pos < the live count <= n
}

int64_t compact_blocks(int64_t n) { return (n + 255) / 256; }

int launch_compact_map(const uint8_t* dead, int64_t n, uint32_t* block_cnt, int32_t* newid, uint32_t* src,
                       hipStream_t s) {
    if (n <= 0) return 0;
    const int64_t nblocks = compact_blocks(n);
    hipLaunchKernelGGL(k_compact_count, dim3((unsigned)nblocks), dim3(256), 0, s, dead, n, block_cnt);
    hipLaunchKernelGGL(k_compact_offsets, dim3(1), dim3(256), 0, s, block_cnt, nblocks);
    hipLaunchKernelGGL(k_compact_map, dim3((unsigned)nblocks), dim3(256), 0, s, dead, n, block_cnt, newid, src);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Row ids[j] of `base` (wpr words of type W per row) -> row j of dst, j < rows.  Consecutive
// threads take consecutive words of a row: a row of vectors is read and written in whole lines.
// member (nullable): a layer's deg array -- the adjacency row of a row that is not in the
// layer (deg < 0) is never read, so it is not moved.
template <class W>
__global__ __launch_bounds__(256) void k_compact_rows(const W* __restrict__ base, W* __restrict__ dst,
                                                      const uint32_t* __restrict__ ids, int64_t rows, int wpr,
                                                      const int32_t* __restrict__ member) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = t / wpr;
    if (j >= rows) return;
    const int64_t id = ids[j];
    if (member && member[id] < 0) return;
    const int w = (int)(t - j * wpr);
    dst[j * wpr + w] = base[id * wpr + w];
}

// dst must not overlap the rows read (the caller's chunk rule, or a staging buffer)
int launch_compact_rows(const void* base, void* dst, const uint32_t* ids, int64_t rows, size_t row_bytes,
                        const int32_t* member, hipStream_t s) {
    if (rows <= 0 || row_bytes == 0) return 0;
    if (row_bytes % 4) return -5;
    const bool wide = row_bytes % 16 == 0 && (uintptr_t)base % 16 == 0 && (uintptr_t)dst % 16 == 0;
    const int wpr = (int)(row_bytes / (wide ? 16 : 4));
    // pieces of at most 2^30 threads (a chunk's rows are independent of each other)
    const int64_t step = std::max<int64_t>(1, ((int64_t)1 << 30) / wpr);
    for (int64_t r0 = 0; r0 < rows; r0 += step) {
        const int64_t nr = std::min(step, rows - r0);
        const unsigned grid = (unsigned)((nr * wpr + 255) / 256);
        char* d = static_cast<char*>(dst) + (size_t)r0 * row_bytes;
        if (wide)
            hipLaunchKernelGGL(k_compact_rows<uint4>, dim3(grid), dim3(256), 0, s, static_cast<const uint4*>(base),
                               reinterpret_cast<uint4*>(d), ids + r0, nr, wpr, member);
        else
            hipLaunchKernelGGL(k_compact_rows<uint32_t>, dim3(grid), dim3(256), 0, s,
                               static_cast<const uint32_t*>(base), reinterpret_cast<uint32_t*>(d), ids + r0, nr, wpr, member);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// One thread per row of a layer, after the move: every neighbour id through the map, the
// order inside the row kept.  An edge to a deleted row (the batched repair leaves none) is
// dropped, the row closes up and its degree shrinks; *dangling counts them.
__global__ __launch_bounds__(256) void k_compact_adj(int32_t* __restrict__ deg, int32_t* __restrict__ adj,
                                                     float* __restrict__ adjd, int cap, int64_t rows,
                                                     const int32_t* __restrict__ newid, int64_t n_old,
                                                     unsigned long long* __restrict__ dangling) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int d = min(deg[r], cap);
    if (d <= 0) return;  // absent (-2), nil (-1) or empty
    int32_t* a = adj + r * cap;
    float* ad = adjd + r * cap;
    int w = 0;
    for (int j = 0; j < d; ++j) {
        const int32_t id = a[j];
        const int32_t m = id >= 0 && id < n_old ? newid[id] : -1;
        if (m < 0) continue;
        a[w] = m;
        if (w != j) ad[w] = ad[j];
        ++w;
    }
    if (w == d) return;
    for (int j = w; j < d; ++j) {
        a[j] = -1;
        ad[j] = 0.f;
    }
    deg[r] = w;
    atomicAdd(dangling, (unsigned long long)(d - w));
}

int launch_compact_adj(int32_t* deg, int32_t* adj, float* adjd, int cap, int64_t rows, const int32_t* newid,
                       int64_t n_old, unsigned long long* dangling, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(k_compact_adj, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, deg, adj, adjd, cap, rows,
                       newid, n_old, dangling);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// One thread builds one 32-bit output word: bit j of out = bit src[j] of old for j < live,
// 0 past the live rows (a row added later inherits no stale bit).  out is not old.
__global__ __launch_bounds__(256) void k_compact_filter(const uint32_t* __restrict__ old, uint32_t* __restrict__ out,
                                                        int64_t nwords, const uint32_t* __restrict__ src,
                                                        int64_t live) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    uint32_t bits = 0;
    const int64_t j0 = w * 32;
    for (int b = 0; b < 32 && j0 + b < live; ++b) {
        const uint32_t sr = src[j0 + b];  // < the old row count <= 32 nwords
        bits |= ((old[sr >> 5] >> (sr & 31)) & 1u) << b;
    }
    out[w] = bits;
}

int launch_compact_filter(const uint32_t* old, uint32_t* out, int64_t nwords, const uint32_t* src, int64_t live,
                          hipStream_t s) {
    if (nwords <= 0) return 0;
    hipLaunchKernelGGL(k_compact_filter, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, s, old, out, nwords, src,
                       live);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mh
