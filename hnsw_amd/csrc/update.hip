// update.hip -- mhnsw_update's own device work (api.cpp): stored rows are re-embedded in place.
// A call works in chunks U of at most a batch of rows (the batched insert's bound), each in
// three steps on the handle's stream:
//   detach     U's rows are marked in the `dead` bytes (UPDATE_MARK), k_delete_repair
//              (build_batch.hpp) rebuilds every live row that points at one -- the Delete path's
//              ranking, over the old vectors -- and k_update_detach takes U's own rows out of
//              every layer they belong to (deg 0, adj -1, adjd 0) and drops the edges that
//              deleted rows still held into U; the marks are then cleared.
//   overwrite  the new vectors go to U's rows (k_update_scatter), and their norms, fp16
//              screening rows and exact-path planes are recomputed by row list (the id-list
//              forms of k_norms, k_h16_rows, k_split_rows and k_split_h16): work proportional
//              to the rows updated, not to the store.
//   re-insert  the batched insert's descend, search and commit over U at its existing ids and
//              levels (BatchBuildArgs::rows, run_batch_layers), from an entry outside U.
// Not applied to update chunks: the link pass (option batch_link, build_link.hpp) -- its
// batch-mate test is n0 <= c < n1 and its staging is indexed by u - n0, both of a contiguous
// batch.  The kernels here are bandwidth kernels over ids and adjacency rows; no distance is
// computed in this file.
#include <algorithm>

#include "engine.hpp"

namespace mh {

__global__ __launch_bounds__(256) void k_update_mark(uint8_t* __restrict__ dead, const uint32_t* __restrict__ ids,
                                                     int64_t m, uint8_t v) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m) dead[ids[j]] = v;  // ids are rows of the store (the host built the list from its key map)
}

int launch_update_mark(uint8_t* dead, const uint32_t* ids, int64_t m, uint8_t v, hipStream_t s) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_update_mark, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, dead, ids, m, v);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// One thread per row of a layer.  After the repair no live row points at a marked row, so only
// the marked rows themselves and the deleted rows (whose adjacency nothing reads again, but the
// export shows) are written.
__global__ __launch_bounds__(256) void k_update_detach(int32_t* __restrict__ deg, int32_t* __restrict__ adj,
                                                       float* __restrict__ adjd, int cap, int64_t rows,
                                                       const uint8_t* __restrict__ dead) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const uint8_t mark = dead[r];
    if (mark == 0) return;
    const int d = min(deg[r], cap);
    if (d <= 0) return;  // absent (-2), nil (-1) or empty
    int32_t* a = adj + r * cap;
    float* ad = adjd + r * cap;
    int w = 0;
    if (mark != UPDATE_MARK) {  // a deleted row keeps its edges to unmarked rows, in order
        for (int j = 0; j < d; ++j) {
            const int32_t id = a[j];
            if (id < 0 || id >= rows || dead[id] == UPDATE_MARK) continue;
            a[w] = id;
            if (w != j) ad[w] = ad[j];
            ++w;
        }
        if (w == d) return;
    }
    for (int j = w; j < d; ++j) {
        a[j] = -1;
        ad[j] = 0.f;
    }
    deg[r] = w;
}

int launch_update_detach(int32_t* deg, int32_t* adj, float* adjd, int cap, int64_t rows, const uint8_t* dead,
                         hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(k_update_detach, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, deg, adj, adjd, cap, rows,
                       dead);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Consecutive threads take consecutive 16-byte words of a row (pitch is a multiple of 64 floats).
// Row from[j] of src (the call's padded vectors) -> row ids[j] of the store.
__global__ __launch_bounds__(256) void k_update_scatter(const float4* __restrict__ src, const uint32_t* __restrict__ ids,
                                                        const uint32_t* __restrict__ from, int64_t m, int wpr,
                                                        float4* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = t / wpr;
    if (j >= m) return;
    const int w = (int)(t - j * wpr);
    dst[(int64_t)ids[j] * wpr + w] = src[(int64_t)from[j] * wpr + w];
}

int launch_update_scatter(const float* src, const uint32_t* ids, const uint32_t* from, int64_t m, int pitch, float* dst,
                          hipStream_t s) {
    if (m <= 0) return 0;
    if (pitch % 4 || (uintptr_t)src % 16 || (uintptr_t)dst % 16) return -5;
    const int wpr = pitch / 4;
    // pieces of at most 2^30 threads
    const int64_t step = std::max<int64_t>(1, ((int64_t)1 << 30) / wpr);
    for (int64_t r0 = 0; r0 < m; r0 += step) {
        const int64_t nr = std::min(step, m - r0);
        hipLaunchKernelGGL(k_update_scatter, dim3((unsigned)((nr * wpr + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(src), ids + r0, from + r0, nr, wpr,
                           reinterpret_cast<float4*>(dst));
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mh
