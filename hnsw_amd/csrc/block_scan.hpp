// block_scan.hpp -- the prefix sum over a 256-thread block that the bitmap compactions share
// (rowset.hip: a filter's allowed rows; compact.hip: the live rows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mh {

// exclusive prefix of v over the block's 256 threads (4 waves) and the block's total
__device__ __forceinline__ uint32_t rs_block_scan(uint32_t v, uint32_t& total) {
    __shared__ uint32_t wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int i = 0; i < w; ++i) base += wsum[i];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return base + inc - v;
}

// One block: the exclusive prefix of cnt[0 .. n), in place.
__device__ __forceinline__ void rs_offsets_inplace(uint32_t* __restrict__ cnt, int64_t n) {
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < n; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const uint32_t v = b < n ? cnt[b] : 0u;
        uint32_t total;
        const uint32_t ex = rs_block_scan(v, total);
        if (b < n) cnt[b] = carry + ex;
        carry += total;
        __syncthreads();  // (rs_block_scan's LDS is reused by the next round)
    }
}

}  // namespace mh
