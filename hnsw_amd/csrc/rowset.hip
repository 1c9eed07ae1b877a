// rowset.hip -- the filtered exact search's row set (search_host.cpp exact_run): a filter's
// bitmap and the skipped-row bytes become the ascending list of the allowed row ids, and the
// list's rows of the exact path's fp16 plane a dense plane of the same K-blocked layout, so
// that every stage of the exact pipeline sees a matrix without masked rows.  Bandwidth
// kernels: a bit test and a rank per row, 16-byte moves per row and K-block.
#include <algorithm>

#include "block_scan.hpp"
#include "engine.hpp"

namespace mh {

constexpr int RS_WORDS = 256;  // bitmap words (of 32 rows) per block of the compaction kernels

// the 32 skipped-row bytes of bitmap word w as bits (rows >= n read as skipped)
__device__ __forceinline__ uint32_t rs_dead_bits(const uint8_t* __restrict__ dead, int64_t w, int64_t n) {
    const int64_t r0 = w * 32;
    uint32_t bits = 0;
    if (r0 + 32 <= n) {
        if (!dead) return 0u;
        const uint4 a = *reinterpret_cast<const uint4*>(dead + r0), b = *reinterpret_cast<const uint4*>(dead + r0 + 16);
        const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) bits |= ((v[j] >> (8 * c)) & 0xffu) ? 1u << (j * 4 + c) : 0u;
        return bits;
    }
    for (int j = 0; j < 32; ++j)  // the tail word: byte by byte, inside [0, n)
        if (r0 + j >= n || (dead && dead[r0 + j])) bits |= 1u << j;
    return bits;
}

// Pass 1, one thread per bitmap word: the word's allowed rows (filter bit set, row below n and
// not skipped) into words[w], the same as 32 skip bytes into mask (1 = not allowed: the
// fallback's row mask), and the block's count of allowed rows.  A bitmap of fwords words may
// be shorter than the rows: the rows past it are not allowed.
__global__ __launch_bounds__(256) void k_rowset_words(const uint32_t* __restrict__ filter, int64_t fwords,
                                                      const uint8_t* __restrict__ dead, int64_t n, int64_t nwords,
                                                      uint32_t* __restrict__ words, uint8_t* __restrict__ mask,
                                                      uint32_t* __restrict__ block_cnt) {
    const int64_t w = (int64_t)blockIdx.x * RS_WORDS + threadIdx.x;
    uint32_t allow = 0;
    if (w < nwords) {
        allow = (w < fwords ? filter[w] : 0u) & ~rs_dead_bits(dead, w, n);
        words[w] = allow;
        uint32_t m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            m[j] = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) m[j] |= ((allow >> (j * 4 + c)) & 1u) ? 0u : 1u << (8 * c);
        }
        // (mask holds nwords * 32 bytes: the tail word's stores stay inside it)
        *reinterpret_cast<uint4*>(mask + w * 32) = make_uint4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<uint4*>(mask + w * 32 + 16) = make_uint4(m[4], m[5], m[6], m[7]);
    }
    uint32_t total;
    (void)rs_block_scan((uint32_t)__popc(allow), total);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// Pass 2, one block: the exclusive prefix of the per-block counts, in place
__global__ __launch_bounds__(256) void k_rowset_offsets(uint32_t* __restrict__ block_cnt, int64_t nblocks) {
    rs_offsets_inplace(block_cnt, nblocks);
}

// Pass 3: a word's allowed rows at the block's offset + the word's rank in the block, in
// ascending order.  ids holds cap entries (the host's count of the same bits).
__global__ __launch_bounds__(256) void k_rowset_ids(const uint32_t* __restrict__ words, int64_t nwords,
                                                    const uint32_t* __restrict__ block_off, uint32_t* __restrict__ ids,
                                                    int64_t cap) {
    const int64_t w = (int64_t)blockIdx.x * RS_WORDS + threadIdx.x;
    uint32_t allow = w < nwords ? words[w] : 0u;
    uint32_t total;
    int64_t pos = (int64_t)block_off[blockIdx.x] + rs_block_scan((uint32_t)__popc(allow), total);
    while (allow) {
        const int j = __ffs((int)allow) - 1;
        allow &= allow - 1;
        if (pos < cap) ids[pos] = (uint32_t)(w * 32 + j);
        ++pos;
    }
}

int launch_rowset_compact(const uint32_t* filter, int64_t fwords, const uint8_t* dead, int64_t n, uint32_t* words,
                          uint8_t* mask, uint32_t* block_cnt, uint32_t* ids, int64_t cap, hipStream_t s) {
    if (n <= 0) return 0;
    const int64_t nwords = (n + 31) / 32, nblocks = (nwords + RS_WORDS - 1) / RS_WORDS;
    hipLaunchKernelGGL(k_rowset_words, dim3((unsigned)nblocks), dim3(256), 0, s, filter, fwords, dead, n, nwords, words,
                       mask, block_cnt);
    hipLaunchKernelGGL(k_rowset_offsets, dim3(1), dim3(256), 0, s, block_cnt, nblocks);
    hipLaunchKernelGGL(k_rowset_ids, dim3((unsigned)nblocks), dim3(256), 0, s, words, nwords, block_cnt, ids, cap);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int64_t rowset_blocks(int64_t n) { return ((n + 31) / 32 + RS_WORDS - 1) / RS_WORDS; }

// Row ids[j] of a K-blocked plane of ld_src rows per K-block (k_split_rows' layout: element
// (row, k) at ((k / 16) * ld + row) * 16 + k % 16) becomes row j of a plane of ld_dst rows.
// Two threads per (row, K-block), 16 bytes each: a wave writes 1 KiB in one run.  The rows'
// unscale and norm (what k_h1_rowconst and the score epilogues read) go with K-block 0.
__global__ __launch_bounds__(256) void k_rowset_gather(const uint16_t* __restrict__ src, int64_t ld_src,
                                                       const uint32_t* __restrict__ ids, int64_t m,
                                                       uint16_t* __restrict__ dst, int64_t ld_dst,
                                                       const float* __restrict__ xinv, const float* __restrict__ xnorm,
                                                       float* __restrict__ xinv_out, float* __restrict__ xnorm_out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = t >> 1;
    if (j >= m) return;
    const int half = (int)(t & 1);
    const int64_t kb = blockIdx.y, id = ids[j];
    const uint4 v = *reinterpret_cast<const uint4*>(src + (kb * ld_src + id) * 16 + half * 8);
    *reinterpret_cast<uint4*>(dst + (kb * ld_dst + j) * 16 + half * 8) = v;
    if (kb == 0 && half == 0) {
        xinv_out[j] = xinv[id];
        xnorm_out[j] = xnorm[id];
    }
}

int launch_rowset_gather(const uint16_t* src, int64_t ld_src, const uint32_t* ids, int64_t m, int pitch, uint16_t* dst,
                         int64_t ld_dst, const float* xinv, const float* xnorm, float* xinv_out, float* xnorm_out,
                         hipStream_t s) {
    if (m <= 0) return 0;
    if (pitch % 16 || m > ld_dst || pitch / 16 > 65535) return -5;
    hipLaunchKernelGGL(k_rowset_gather, dim3((unsigned)((2 * m + 255) / 256), (unsigned)(pitch / 16)), dim3(256), 0, s,
                       src, ld_src, ids, m, dst, ld_dst, xinv, xnorm, xinv_out, xnorm_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the preselection's candidates (positions in the compact plane) as row ids
__global__ void k_rowset_remap(uint32_t* __restrict__ cand, int64_t total, const uint32_t* __restrict__ ids,
                               int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t c = cand[i];
    if (c != EMPTY_ID) cand[i] = c < m ? ids[c] : EMPTY_ID;
}

int launch_rowset_remap(uint32_t* cand, int64_t total, const uint32_t* ids, int64_t m, hipStream_t s) {
    if (total <= 0) return 0;
    hipLaunchKernelGGL(k_rowset_remap, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cand, total, ids, m);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mh
